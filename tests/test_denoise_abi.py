"""The denoiser (rtgl_denoise, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the library agree on
the four entry points and on the parameter block, the defaults are the documented ones, the calls reject a NULL context before touching
a device, the C++ facade's methods compile with the host compiler, and the new kernel instances spill nothing (compiler resource report;
hipcc cross-compiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from resource_report import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtgl_amd.h")
ENTRY_POINTS = ["rtgl_denoise_defaults", "rtgl_denoise", "rtgl_read_denoised_f32", "rtgl_device_denoised"]
ERR_INVALID = -1


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_denoise_entry_points_and_the_parameter_block(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_denoise_defaults\s*\(\s*rtgl_denoise_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_denoise\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*const\s+rtgl_denoise_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_read_denoised_f32\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bvoid\s*\*\s*rtgl_device_denoised\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    m = re.search(r"\bRTGL_DENOISE_DEMODULATE\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == rt.host.DENOISE_DEMODULATE == 1
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the block: the header's fields in the binding's order, 32 bytes
    body = re.search(r"typedef\s+struct\s+rtgl_denoise_params\s*\{(.*?)\}\s*rtgl_denoise_params\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("uint32_t", "passes", 1), ("float", "sigma_color", 1), ("float", "sigma_normal", 1),
                                                         ("float", "sigma_position", 1), ("uint32_t", "flags", 1), ("uint32_t", "reserved", 3)]
    assert [n for n, _ in rt.host.CDenoiseParams._fields_] == [n for _, n, _ in fields]
    assert C.sizeof(rt.host.CDenoiseParams) == 32


def test_library_exports_the_denoise_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_defaults_are_the_documented_ones_and_need_no_device(rt):
    lib = rt.host.load_library()
    p = rt.host.CDenoiseParams(passes=99, sigma_color=-1, flags=7, reserved=(1, 2, 3))
    assert lib.rtgl_denoise_defaults(C.byref(p)) == 0
    assert (p.passes, p.flags, list(p.reserved)) == (5, rt.host.DENOISE_DEMODULATE, [0, 0, 0])
    assert (np.float32(p.sigma_color), np.float32(p.sigma_normal), np.float32(p.sigma_position)) == (np.float32(16), np.float32(0.3), np.float32(0.05))
    assert lib.rtgl_denoise_defaults(None) == ERR_INVALID
    d = rt.host.DENOISE_DEFAULTS
    assert (d["passes"], d["sigma_color"], d["sigma_normal"], d["sigma_position"], d["demodulate"]) == (5, 16.0, 0.3, 0.05, True)
    # ... and the header's comment states the same values
    assert re.search(r"passes 5, sigma_color 16, sigma_normal 0\.3, sigma_position 0\.05, demodulate on", header_text())


def test_denoise_calls_reject_a_null_context(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    buf = np.zeros(64, np.float32)
    p = rt.host.CDenoiseParams()
    lib.rtgl_denoise_defaults(C.byref(p))
    assert lib.rtgl_denoise(None, None) == ERR_INVALID
    assert lib.rtgl_denoise(None, C.byref(p)) == ERR_INVALID
    assert lib.rtgl_read_denoised_f32(None, buf.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    assert lib.rtgl_device_denoised(None) is None


def test_the_mirror_and_the_binding_state_the_same_defaults(rt):
    import denoise_mirror
    assert denoise_mirror.DEFAULTS == rt.host.DENOISE_DEFAULTS


FACADE_DENOISE = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    r.set_frame_budget(4);
    r.run();
    bool ok = r.denoise();
    rtgl_denoise_params p;
    rtgl_denoise_defaults(&p);
    p.passes = 3; p.flags &= ~(uint32_t)RTGL_DENOISE_DEMODULATE;
    ok = r.denoise(&p) && ok;
    const std::vector<float> img = r.read_denoised();
    ok = r.save_denoised_pfm("denoised.pfm") && r.save_pfm("beauty.pfm") && ok;
    return ok && img.size() == (size_t)64 * 48 * 4 ? 0 : 1;
}
"""


def test_facade_denoise_methods_compile_with_the_host_compiler(tmp_path):
    src = tmp_path / "facade_denoise.cpp"
    src.write_text(FACADE_DENOISE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_atrous_kernel_instances_spill_nothing(resource_report):
    """atrous_kernel<first pass demodulates, last pass remodulates, wide segments> and the two instances of passes = 0"""
    passes, identity = {}, {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt13atrous_kernelILb([01])ELb([01])ELb([01])EEEvNS_10AtrousArgsE$", name)
        if m:
            passes[tuple(int(g) for g in m.groups())] = r
        m = re.match(r"_ZN2rt22atrous_identity_kernelILb([01])EEEvNS_10AtrousArgsE$", name)
        if m:
            identity[int(m.group(1))] = r
    assert sorted(passes) == [(d, r, w) for d in (0, 1) for r in (0, 1) for w in (0, 1)], sorted(resource_report)
    assert sorted(identity) == [0, 1]
    for key, r in list(passes.items()) + list(identity.items()):
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        assert r["LDS Size"] == 0, f"{key}: the segments are dynamic shared memory: {r}"
    for key, r in passes.items():
        # four blocks of four waves per CU need four waves per SIMD: the barrier of one block is hidden behind the others
        assert r["Occupancy"] >= 4, f"atrous_kernel{key}: {r}"
