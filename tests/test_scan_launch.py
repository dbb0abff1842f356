"""The launch policy of the kernel-4 scan (raytracer.glsl_amd/csrc/rt_scan_launch.hpp), without a GPU.
  * tests/cpp/scan_launch_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: sixteen anchored launches, and a sweep in which every launch must fit the buffers sized from the same mesh and options.
  * rtgl_amd.hip keeps no copy of that arithmetic: the quads that hold triangles are counted in the header alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")


def test_scan_launch_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_launch_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "scan_launch_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_header_is_host_only_and_the_library_keeps_no_copy():
    with open(os.path.join(CSRC, "rt_scan_launch.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<algorithm>", "<cstddef>", "<cstdint>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "rt_scan_launch::real_quads(" in code
    assert not re.search(r"n_tri_visits\s*\+\s*\(uint32_t\)kMfQuadTris", code)      # the written-out count of the quads that hold triangles
    assert not re.search(r"\bsolo_(chunks|regions|dynamic)\b", code)
