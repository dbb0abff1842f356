"""The temporal clip (rtgl_temporal_clip, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the
library agree on the entry points and on the parameter block; header, binding, facade and mirror state the same defaults; the calls reject
a NULL context, whatever the record, before touching a device (the record's rules: tests/test_post_plans.py); a C program compiles against the header and the facade's method with the
host compiler; and the eight kernel instances spill nothing and hold the LDS they were designed for (compiler resource report; hipcc
cross-compiles)."""
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
ENTRY_POINTS = ["rtgl_temporal_clip_defaults", "rtgl_temporal_clip"]
DEFAULTS_TEXT = r"sigma_scale (\d+), clip_history (\d+), sigma_normal 0\.3, sigma_position 0\.05"
ERR_INVALID = -1


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_parameter_block(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_temporal_clip_defaults\s*\(\s*rtgl_temporal_clip_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_temporal_clip\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*const\s+rtgl_temporal_clip_params\s*\*\s*\w+\s*\)\s*;", text)
    assert "CORRECTLY ROUNDED SQUARE ROOT" in text
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the block: the header's fields in the binding's order, 32 bytes
    body = re.search(r"typedef\s+struct\s+rtgl_temporal_clip_params\s*\{(.*?)\}\s*rtgl_temporal_clip_params\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("float", "sigma_scale", 1), ("float", "clip_history", 1), ("float", "sigma_normal", 1), ("float", "sigma_position", 1),
                      ("uint32_t", "flags", 1), ("uint32_t", "reserved", 3)]
    assert 4 * sum(k for _, _, k in fields) == 32
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in fields] == list(rt.host.CTemporalClipParams._fields_)
    assert C.sizeof(rt.host.CTemporalClipParams) == 32
    assert [getattr(rt.host.CTemporalClipParams, n).offset for _, n, _ in fields] == [0, 4, 8, 12, 16, 20]


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_and_mirror_state_the_same_defaults(rt):
    import temporal_clip_mirror
    lib = rt.host.load_library()
    p = rt.host.CTemporalClipParams(sigma_scale=-7, clip_history=0, sigma_normal=-1, sigma_position=9, flags=7, reserved=(1, 2, 3))
    assert lib.rtgl_temporal_clip_defaults(C.byref(p)) == 0
    assert lib.rtgl_temporal_clip_defaults(None) == ERR_INVALID
    d = rt.host.TEMPORAL_CLIP_DEFAULTS
    assert (p.flags, list(p.reserved)) == (0, [0, 0, 0])
    for name in ("sigma_scale", "clip_history", "sigma_normal", "sigma_position"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(sigma_scale=2.0, clip_history=3.0, sigma_normal=0.3, sigma_position=0.05)
    assert temporal_clip_mirror.DEFAULTS == d
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m and float(m.group(1)) == d["sigma_scale"] and float(m.group(2)) == d["clip_history"], path
    # a clipped pixel falls under the threshold at which "denoise_variance" = 1 trusts the temporal variance
    import temporal_moments_mirror
    assert d["clip_history"] < float(temporal_moments_mirror.MIN_HISTORY)


def test_calls_reject_a_null_context(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    p = rt.host.CTemporalClipParams()
    lib.rtgl_temporal_clip_defaults(C.byref(p))
    assert lib.rtgl_temporal_clip(None, None) == ERR_INVALID
    assert lib.rtgl_temporal_clip(None, C.byref(p)) == ERR_INVALID
    p.sigma_scale = float("nan")
    assert lib.rtgl_temporal_clip(None, C.byref(p)) == ERR_INVALID


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_temporal_clip_params p;
    int rc = rtgl_temporal_clip_defaults(&p);
    p.sigma_scale = 1.5f; p.clip_history = 2.0f; p.sigma_normal = 0.0f; p.sigma_position = 0.1f; p.flags = 0u; p.reserved[2] = 0u;
    rc |= rtgl_temporal_clip((rtgl_context *)0, &p);
    rc |= rtgl_temporal_clip((rtgl_context *)0, (const rtgl_temporal_clip_params *)0);
    return rc + (int)(sizeof p != 32);
}
"""

FACADE_CLIP = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    r.set_frame_budget(2);
    r.run();
    bool ok = r.temporal_accumulate() && r.temporal_clip();
    rtgl_temporal_clip_params p;
    rtgl_temporal_clip_defaults(&p);
    p.sigma_scale = 3.0f; p.sigma_normal = 0.0f;
    ok = r.temporal_clip(&p) && ok;
    const std::vector<float> hist = r.read_temporal();
    return ok && hist.size() == (size_t)64 * 48 * 4 ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "clip.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_clip.cpp"
    src.write_text(FACADE_CLIP)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


# temporal_clip_kernel<normal term, position term, moments>: VGPRs as the build gives them
VGPRS = {(0, 0, 0): 26, (0, 0, 1): 28, (0, 1, 0): 34, (0, 1, 1): 36, (1, 0, 0): 32, (1, 0, 1): 34, (1, 1, 0): 44, (1, 1, 1): 46}
LDS_TILE = 70 * 10             # the tile of 64 x 4 and a halo of 3


def test_temporal_clip_kernel_instances_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt20temporal_clip_kernelILb([01])ELb([01])ELb([01])EEEv", name)
        if m:
            found[tuple(int(g) for g in m.groups())] = r
    assert sorted(found) == [(n, p, m) for n in (0, 1) for p in (0, 1) for m in (0, 1)], sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        # one float array per staged component (I.rgb, N.xyz and P.xyz where their term is on) and a byte per pixel for its kind: 25.9 KB at most
        arrays = 3 + 3 * key[0] + 3 * key[1]
        assert r["LDS Size"] == 4 * arrays * LDS_TILE + LDS_TILE, f"{key}: {r}"
        assert r["LDS Size"] <= 25900
        assert r["VGPRs"] == VGPRS[key], f"{key}: {r}"
        # 160 KB of LDS hold six blocks of 25.9 KB, 24 waves a CU: the registers must not be what limits it further
        assert r["Occupancy"] >= 6, f"{key}: {r}"
