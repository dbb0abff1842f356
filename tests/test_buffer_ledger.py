"""The device-buffer ledger (raytracer.glsl_amd/csrc/rt_buffers.hpp), without a GPU.
  * tests/cpp/buffer_ledger_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a
    child process: a fixed script of ledger operations against a counting allocator, clean and with every n-th allocation failing.
  * rtgl_amd.hip allocates and frees device memory in ONE place each: the ledger's two adapters."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ledger_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buffer_ledger_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "buffer_ledger_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_one_allocator_and_one_free_in_the_library():
    with open(os.path.join(ROOT, "raytracer.glsl_amd", "csrc", "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    assert len(re.findall(r"\bhipMalloc\(", code)) == 1
    assert len(re.findall(r"\bhipFree\(", code)) == 1
