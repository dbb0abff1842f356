"""The post-process half of the C++ facade (include/rtgl/renderer.h) without a device: the driver of tests/test_gpu_facade_post.py
compiles warning-free with both language standards, and a Renderer that got no context answers every post-process method with
false / empty / -1 / 0 frames / a zeroed summary -- run under the address and undefined-behaviour sanitizers, which are on the
stand-alone executable only (the library is linked as it is built; nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracer.glsl_amd")
WARNINGS = ["-O1", "-Wall", "-Werror"]


def build_program(rt, tmp, name, std="c++17", extra=()):
    """tests/cpp/<name>.cpp against include/ and librtgl_amd.so, as tests/test_facade.py builds facade_demo"""
    rt.host.build_library()
    exe = os.path.join(str(tmp), f"{name}_{std.replace('+', 'x')}")
    subprocess.check_call(["g++", "-std=" + std] + WARNINGS + list(extra) + ["-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L" + PKG, "-lrtgl_amd", "-lz", "-Wl,-rpath," + PKG])
    return exe


@pytest.mark.parametrize("std", ["c++17", "c++20"])
def test_the_driver_compiles_without_warnings(tmp_path, rt, std):
    assert os.path.exists(build_program(rt, tmp_path, "facade_post", std, ["-Wextra"]))


def test_a_renderer_without_a_context_refuses_everything_under_the_sanitizers(tmp_path, rt):
    """tests/cpp/facade_null_check.cpp asks for a device index that exists nowhere, so it runs the same with and without a GPU"""
    exe = build_program(rt, tmp_path, "facade_null_check", extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = subprocess.run([exe, str(tmp_path)], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    if out.returncode == 127 or "error while loading shared libraries" in out.stderr:
        pytest.skip("librtgl_amd.so cannot be loaded on this machine: " + out.stderr.strip()[-200:])
    assert out.returncode == 0, f"exit {out.returncode}\n{out.stdout}\n{out.stderr}"
    assert "checks passed" in out.stdout and "ERROR: " not in out.stderr and "runtime error" not in out.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith((".pfm", ".png"))]          # a refused save writes no file
