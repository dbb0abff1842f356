"""Temporal luminance moments (options "temporal_moments" and "denoise_variance", include/rtgl_amd.h) at the ABI level, without a GPU: the
header, the library, the Python binding and the facade agree on the two read-out calls; the calls reject a NULL context before touching a
device; the facade's method compiles with the host compiler; and the kernel instances with the options on spill nothing and keep the
occupancy of the option-off ones (compiler resource report; hipcc cross-compiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from resource_report import report

from test_temporal_abi import ERR_INVALID, FACADE, HEADER, ROOT, header_text

ENTRY_POINTS = ["rtgl_read_temporal_moments_f32", "rtgl_device_temporal_moments"]


def test_header_declares_the_calls_and_the_options(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_read_temporal_moments_f32\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bvoid\s*\*\s*rtgl_device_temporal_moments\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    assert '"temporal_moments"' in text and '"denoise_variance"' in text
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the parameter blocks are the ones they were: the switches are options
    assert C.sizeof(rt.host.CTemporalParams) == 32 and C.sizeof(rt.host.CDenoiseGuidedParams) == 32


def test_library_exports_the_calls(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_binding_has_the_methods_on_both_classes(rt):
    for cls in (rt.host.Context, rt.host.HeadlessRenderer):
        for name in ("read_temporal_moments", "device_temporal_moments_ptr"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)


def test_calls_reject_a_null_context(rt):
    lib = rt.host.load_library()
    buf = np.zeros(64, np.float32)
    assert lib.rtgl_read_temporal_moments_f32(None, buf.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    assert lib.rtgl_read_temporal_moments_f32(None, None) == ERR_INVALID
    assert lib.rtgl_device_temporal_moments(None) is None
    for key in (b"temporal_moments", b"denoise_variance"):
        assert lib.rtgl_set_option(None, key, 1) == ERR_INVALID
        assert lib.rtgl_get_option(None, key, C.byref(C.c_int(0))) == ERR_INVALID


FACADE_MOMENTS = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    r.set_frame_budget(2);
    r.run();
    bool ok = rtgl_set_option(r.context(), "temporal_moments", 2) == RTGL_OK;
    ok = r.temporal_accumulate() && ok;
    const std::vector<float> moments = r.read_temporal_moments();
    ok = rtgl_set_option(r.context(), "denoise_source", 1) == RTGL_OK && rtgl_set_option(r.context(), "denoise_variance", 1) == RTGL_OK && ok;
    float *on_device = (float *)rtgl_device_temporal_moments(r.context());
    return ok && on_device && moments.size() == (size_t)64 * 48 * 4 ? 0 : 1;
}
"""


def test_facade_method_compiles_with_the_host_compiler(tmp_path):
    with open(FACADE) as f:
        assert re.search(r"std::vector<float>\s+read_temporal_moments\s*\(\s*\)\s*const", f.read())
    src = tmp_path / "facade_temporal_moments.cpp"
    src.write_text(FACADE_MOMENTS)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_temporal_moments_kernel_instances_spill_nothing(resource_report):
    """temporal_kernel<history, static shortcut, normal test, position test, moments mode> with mode 1 or 2 (demodulation = mode - 1): the
    two instances without history and all sixteen with it"""
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt15temporal_kernelILb([01])ELb([01])ELb([01])ELb([01])ELi([12])EEEv", name)
        if m:
            found[tuple(int(g) for g in m.groups()[:4]) + (int(m.group(5)) - 1,)] = r
    want = [(0, 0, 0, 0, d) for d in (0, 1)] + [(1, s, n, p, d) for s in (0, 1) for n in (0, 1) for p in (0, 1) for d in (0, 1)]
    assert sorted(found) == sorted(want), sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        assert r["LDS Size"] == 0, f"{key}: {r}"
        assert r["Occupancy"] >= 8, f"{key}: {r}"              # (a gather kernel: every wave slot the SIMD has, like temporal_kernel)


def test_prepare_variant_spills_nothing(resource_report):
    r = resource_report.get("_ZN2rt26guided_prepare_tvar_kernelENS_14GuidedTvarArgsE")
    assert r is not None, sorted(resource_report)
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= 4, r                              # (by registers; its 37.4 KB of LDS are requested at launch, like its sibling's)
    # the sibling and the option-off temporal instances are still there
    assert "_ZN2rt21guided_prepare_kernelENS_10GuidedArgsE" in resource_report
    assert any(re.match(r"_ZN2rt15temporal_kernelILb1ELb0ELb1ELb1ELi0EEEv", name) for name in resource_report)
