"""When the kept bits of the camera-ray bounce serve a frame (raytracer.glsl_amd/csrc/rt_camera_keep.hpp), without a GPU.
  * tests/cpp/camera_keep_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: the standing camera, every field of the key and of the camera, the frames the cache does not cover, the jitter bound
    (its limits, the five far cameras at which its first version was too small, monotonicity in |pos|, the benchmark camera's growth).
  * rtgl_amd.hip keeps no second definition: the scan's launch and the lean camera bounce take one decision per frame."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")


def test_camera_keep_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "camera_keep_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "camera_keep_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_header_is_host_only_and_the_library_decides_once():
    with open(os.path.join(CSRC, "rt_camera_keep.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<cmath>", "<cstdint>", "<cstring>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    assert len(re.findall(r"rt_camera_keep::decide\(", code)) == 1
    assert len(re.findall(r"camera_keep_decide\(ctx", code)) == 1           # called once per frame, by launch_wavefront
    assert len(re.findall(r"rt_camera_keep::lean\(", code)) == 1
    assert not re.search(r"\bsame_camera\(", code)                            # the comparison lives in the header alone
