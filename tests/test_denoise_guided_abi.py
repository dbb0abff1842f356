"""The variance-guided denoiser (rtgl_denoise_guided, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding
and the library agree on the entry points and on the parameter block; header, binding, facade and mirror state the same defaults; the calls
reject a NULL context before touching a device; the facade's methods compile with the host compiler; and the new kernel instances spill
nothing (compiler resource report; hipcc cross-compiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from resource_report import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtgl_amd.h")
FACADE = os.path.join(ROOT, "include", "rtgl", "renderer.h")
ENTRY_POINTS = ["rtgl_denoise_guided_defaults", "rtgl_denoise_guided", "rtgl_read_denoise_variance_f32", "rtgl_device_denoise_variance"]
DEFAULTS_TEXT = r"passes 5, sigma_lum (\d+), sigma_normal 0\.3, sigma_position 0\.05, firefly_ratio 1,\s+(?:\*\s+|//\s+)?demodulate on"
ERR_INVALID = -1


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_parameter_block(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_denoise_guided_defaults\s*\(\s*rtgl_denoise_guided_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_denoise_guided\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*const\s+rtgl_denoise_guided_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_read_denoise_variance_f32\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bvoid\s*\*\s*rtgl_device_denoise_variance\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the block: the header's fields in the binding's order, 32 bytes
    body = re.search(r"typedef\s+struct\s+rtgl_denoise_guided_params\s*\{(.*?)\}\s*rtgl_denoise_guided_params\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("uint32_t", "passes", 1), ("float", "sigma_lum", 1), ("float", "sigma_normal", 1), ("float", "sigma_position", 1),
                      ("float", "firefly_ratio", 1), ("uint32_t", "flags", 1), ("uint32_t", "reserved", 2)]
    assert 4 * sum(k for _, _, k in fields) == 32
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in fields] == list(rt.host.CDenoiseGuidedParams._fields_)
    assert C.sizeof(rt.host.CDenoiseGuidedParams) == 32
    assert [getattr(rt.host.CDenoiseGuidedParams, n).offset for _, n, _ in fields] == [0, 4, 8, 12, 16, 20, 24]


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS + ["rtgl_denoise", "rtgl_read_denoised_f32"]:
        assert hasattr(lib, name), name


def test_header_binding_facade_and_mirror_state_the_same_defaults(rt):
    import denoise_guided_mirror
    lib = rt.host.load_library()
    p = rt.host.CDenoiseGuidedParams(passes=99, sigma_lum=-1, firefly_ratio=-3, flags=7, reserved=(1, 2))
    assert lib.rtgl_denoise_guided_defaults(C.byref(p)) == 0
    assert lib.rtgl_denoise_guided_defaults(None) == ERR_INVALID
    d = rt.host.DENOISE_GUIDED_DEFAULTS
    assert (p.passes, p.flags, list(p.reserved)) == (d["passes"], rt.host.DENOISE_DEMODULATE if d["demodulate"] else 0, [0, 0]) == (5, 1, [0, 0])
    for name in ("sigma_lum", "sigma_normal", "sigma_position", "firefly_ratio"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert (d["sigma_normal"], d["sigma_position"], d["firefly_ratio"]) == (0.3, 0.05, 1.0) and d["sigma_lum"] in (2.0, 4.0, 8.0)
    assert denoise_guided_mirror.DEFAULTS == d
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m and float(m.group(1)) == d["sigma_lum"], path


def test_calls_reject_a_null_context(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    buf = np.zeros(64, np.float32)
    p = rt.host.CDenoiseGuidedParams()
    lib.rtgl_denoise_guided_defaults(C.byref(p))
    assert lib.rtgl_denoise_guided(None, None) == ERR_INVALID
    assert lib.rtgl_denoise_guided(None, C.byref(p)) == ERR_INVALID
    assert lib.rtgl_read_denoise_variance_f32(None, buf.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    assert lib.rtgl_device_denoise_variance(None) is None


FACADE_DENOISE = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    r.set_frame_budget(4);
    r.run();
    bool ok = r.denoise_guided();
    rtgl_denoise_guided_params p;
    rtgl_denoise_guided_defaults(&p);
    p.passes = 3; p.firefly_ratio = 0.0f; p.flags &= ~(uint32_t)RTGL_DENOISE_DEMODULATE;
    ok = r.denoise_guided(&p) && ok;
    const std::vector<float> img = r.read_denoised(), var = r.read_denoise_variance();
    ok = r.save_denoised_pfm("denoised.pfm") && ok;
    return ok && img.size() == (size_t)64 * 48 * 4 && var.size() == img.size() ? 0 : 1;
}
"""


def test_facade_methods_compile_with_the_host_compiler(tmp_path):
    src = tmp_path / "facade_denoise_guided.cpp"
    src.write_text(FACADE_DENOISE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_guided_kernel_instances_spill_nothing(resource_report):
    """guided_kernel<last pass, remodulates, wide segments> and the prepare kernel"""
    passes, prepare = {}, None
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt13guided_kernelILb([01])ELb([01])ELb([01])EEEvNS_10GuidedArgsE$", name)
        if m:
            passes[tuple(int(g) for g in m.groups())] = r
        if re.match(r"_ZN2rt21guided_prepare_kernelENS_10GuidedArgsE$", name):
            prepare = r
    assert sorted(passes) == [(l, r, w) for (l, r) in ((0, 0), (1, 0), (1, 1)) for w in (0, 1)], sorted(resource_report)
    assert prepare is not None
    for key, r in list(passes.items()) + [("prepare", prepare)]:
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        assert r["LDS Size"] == 0, f"{key}: the staged arrays are dynamic shared memory: {r}"
        # four blocks of four waves per CU need four waves per SIMD: the barrier of one block is hidden behind the others.  The remark
        # is the bound by registers alone: the staged arrays are dynamic shared memory, which the compiler does not see, so this does
        # NOT check what LDS allows at launch (the prepare kernel 4 waves per SIMD, a wide pass at step 128 only 3)
        assert r["Occupancy"] >= 4, f"{key}: {r}"
