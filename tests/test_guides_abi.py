"""rtgl_guides_frame (include/rtgl_amd.h, "guide pass") at the ABI level, without a GPU: the header, the Python binding, the facade and the
library agree on the entry point; the call rejects a NULL context before touching a device; a C99 program compiles against the header
and the facade's methods with the host compilers; the host half (rt_guides_plan.hpp) is host-only, is what the library goes by, and passes
its stand-alone program under the address and undefined-behaviour sanitizers; the kernel header uses only the shared device functions and
stores through store_through; and the two kernels spill nothing and use neither scratch nor LDS (compiler resource report)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from resource_report import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtgl_amd.h")
FACADE = os.path.join(ROOT, "include", "rtgl", "renderer.h")
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
ERR_INVALID = -1


def text_of(path):
    with open(path) as f:
        return f.read()


def code_of(path):
    return "".join(re.sub(r"//.*", "", line) for line in text_of(path).splitlines(True))


def test_header_declares_the_entry_point_and_its_contract(rt):
    text = text_of(HEADER)
    assert re.search(r"\bint\s+rtgl_guides_frame\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    assert "rtgl_guides_frame" in rt.host.ABI_SYMBOLS
    at = text.index("-- guide pass")
    assert text.index("-- first-hit planes") < at < text.index("-- denoiser")
    section = text[at:text.index("int rtgl_guides_frame")]
    for phrase in ("max_bounce == 0", "a mesh wins a tie", "(x + prev * (n - 1)) / n", "ends no session", "bit-identical", "RTGL_ERR_INVALID", "RTGL_ERR_STATE",
                   "multi-device", "kept camera bits", "empty footprint"):
        assert phrase in section, phrase


def test_library_exports_the_entry_point_and_the_binding_matches(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    assert hasattr(lib, "rtgl_guides_frame")
    fn = lib.rtgl_guides_frame
    assert list(fn.argtypes) == [C.c_void_p] and fn.restype is C.c_int
    assert callable(rt.host.Context.guides_frame) and callable(rt.host.HeadlessRenderer.render_guides)


def test_call_rejects_a_null_context(rt):
    lib = rt.host.load_library()
    assert lib.rtgl_guides_frame(None) == ERR_INVALID


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    int (*fn)(rtgl_context *) = rtgl_guides_frame;
    return fn((rtgl_context *)0) == RTGL_ERR_INVALID ? 0 : 1;
}
"""

FACADE_GUIDES = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALL);
    bool ok = r.guides_frame();
    ok = r.render_guides(3) == 3 && ok;
    const std::vector<float> normal = r.read_aov(RTGL_AOV_NORMAL);
    const std::vector<int32_t> ids = r.read_aov<int32_t>(RTGL_AOV_IDS);
    return ok && normal.size() == ids.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "guides.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_guides_methods.cpp"
    src.write_text(FACADE_GUIDES)
    for path in (str(src), os.path.join(ROOT, "tests", "cpp", "facade_guides.cpp")):      # the methods alone, and the device test's driver
        out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", inc, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]


def test_guides_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "guides_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "guides_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    header = text_of(os.path.join(CSRC, "rt_guides_plan.hpp"))
    assert set(re.findall(r"#include\s+(\S+)", header)) == {"<cstddef>", "<cstdint>"}
    library, host = code_of(os.path.join(CSRC, "rtgl_amd.hip")), code_of(os.path.join(CSRC, "rt_guides_host.hpp"))
    assert library.count('#include "rt_guides_host.hpp"') == 1 and "hipMalloc" not in host
    code = library + host                                  # (the entry point and its refusals; the pass behind them)
    for name in ("refused", "after_pass", "stage", "stage_kernel", "generates_rays", "blocks", "wave_bounces", "enqueues", "writes"):
        assert f"rt_guides_plan::{name}(" in code, name
    entry = library[library.index('extern "C" int rtgl_guides_frame('):]
    entry = entry[:entry.index("\n}\n")]
    assert "rt_guides_plan::refused(" in entry and entry.count("guides_pass(ctx)") == 1 and "ENTER(ctx)" in entry
    body = host[host.index("static int guides_pass("):]
    body = body[:body.index("\n}\n")]
    mesh = code[code.index("static int launch_guides_mesh("):]
    mesh = mesh[:mesh.index("\n}\n")]
    # the stages are the existing ones, the wave buffers come from the one function that sizes them, every buffer from the ledger
    assert mesh.count("launch_intersect_solo(") == 1 and mesh.count("launch_intersect_split(") == 1 and mesh.count("generate_rays_kernel") == 1
    assert "ensure_wave_buffers(ctx, n0, bounces, false)" in mesh and "hipMalloc" not in mesh + body
    assert "guides_kernel<true>" in mesh and "guides_kernel<false>" in body
    # the relaxation is the fold's own: the refusal of the post-process calls is the one of before
    for plan in ("rt_bucket_guide_plan.hpp", "rt_temporal_plan.hpp"):
        assert "no frame has been rendered since the first-hit planes last restarted" in text_of(os.path.join(CSRC, plan))


def test_kernel_header_uses_the_shared_device_functions_only():
    kernels = code_of(os.path.join(CSRC, "rt_guides.hpp"))
    assert "#pragma clang fp contract(off)" in kernels
    for name in ("camera_slot_pixel(", "camera_slot_ray(", "sphere_pass_id(", "aov_write(", "tri_planes[", "env_lookup("):
        assert name in kernels, name
    for name in ("atomic", "__shared__", "__syncthreads", "shade_hit", "finish_path", "store_ray", "load_ray", "counters", "__ballot", "rng_out", "im.pixels"):
        assert name not in kernels, name
    assert not re.findall(r"^\s*(?:\w+(?:\.\w+)*\[[^\]]*\]|\*\s*\w+)\s*=[^=]", kernels, re.M)      # no store of its own: aov_write's go through store_through
    assert kernels.count("__global__") == 1 and "template <bool kMesh>" in kernels


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_guides_kernels_spill_nothing_and_hold_no_lds(resource_report):
    """no spill, no scratch, no LDS, and at least 6 waves per SIMD (a latency-bound gather: DESIGN.md 5.17 reports the build's figures)"""
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt\d+guides_kernelILb([01])EEEv", name)
        if m:
            found[int(m.group(1))] = r
    assert sorted(found) == [0, 1], sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, f"{key}: {r}"
        assert r["Occupancy"] >= 6, f"{key}: {r}"
