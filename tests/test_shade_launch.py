"""The rule that picks the form of a shade launch (raytracer.glsl_amd/csrc/rt_shade_launch.hpp), without a GPU.
  * tests/cpp/shade_launch_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: a one-pass grid covers queue 0 at every listed size, and the rule never gives the one-pass form a grid from the estimate.
  * the header is host-only, and rtgl_amd.hip computes no shade grid of its own: the one-pass kernel is launched through the rule alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")


def test_shade_launch_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shade_launch_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "shade_launch_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_header_is_host_only_and_the_library_launches_shade_through_it():
    with open(os.path.join(CSRC, "rt_shade_launch.hpp")) as f:
        header = f.read()
    assert re.findall(r"#include\s+(\S+)", header) == ["<cstdint>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    # one call of the rule, and the one launch site of the two kernels takes its grid from what the rule returned
    assert len(re.findall(r"rt_shade_launch::launch\(", code)) == 1
    assert not re.search(r"hipLaunchKernelGGL\(\(shade_(stride_)?kernel<", code)
    launches = re.findall(r"hipLaunchKernelGGL\(kKernels\[L\.one_pass\][^;]*;", code)
    assert len(launches) == 1 and "dim3(L.blocks)" in launches[0], launches
