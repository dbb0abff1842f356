"""The display transform (rtgl_tonemap, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the library
agree on the entry points and on the parameter block; header, binding, facade and mirror state the same defaults; the calls reject a NULL
context, whatever the record, before touching a device (the record's rules: tests/test_post_plans.py); a C program compiles against the header and the facade's methods with the host
compiler; and the kernels spill nothing and hold the LDS they were designed for (compiler resource report; hipcc cross-compiles)."""
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
ENTRY_POINTS = ["rtgl_tonemap_defaults", "rtgl_tonemap", "rtgl_tonemap_reset", "rtgl_read_display_u8", "rtgl_device_display",
                "rtgl_read_tonemap_exposure", "rtgl_read_tonemap_histogram"]
DEFAULTS_TEXT = (r"source (\d+), op (\d+), auto exposure on,\s+(?://\s+)?exposure (\d+), key ([\d.]+), white (\d+), adapt (\d+),\s+(?:\*\s+|//\s+)?"
                 r"exposure_min 2\^-(\d+), exposure_max 2\^(\d+), low_permille (\d+), high_permille (\d+)")
ERR_INVALID = -1


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_parameter_block(rt):
    text = header_text()
    ctx, par = r"rtgl_context\s*\*\s*\w+", r"const\s+rtgl_tonemap_params\s*\*\s*\w+"
    for decl in (r"\bint\s+rtgl_tonemap_defaults\s*\(\s*rtgl_tonemap_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_tonemap\s*\(\s*{ctx}\s*,\s*{par}\s*\)\s*;",
                 rf"\bint\s+rtgl_tonemap_reset\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_read_display_u8\s*\(\s*{ctx}\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;",
                 rf"\bvoid\s*\*\s*rtgl_device_display\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_read_tonemap_exposure\s*\(\s*{ctx}\s*,\s*float\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_tonemap_histogram\s*\(\s*{ctx}\s*,\s*uint32_t\s+\w+\[256\]\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;"):
        assert re.search(decl, text), decl
    assert "NO TRANSCENDENTAL FUNCTION" in text
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the block: the header's fields in the binding's order, 64 bytes
    body = re.search(r"typedef\s+struct\s+rtgl_tonemap_params\s*\{(.*?)\}\s*rtgl_tonemap_params\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("uint32_t", "source", 1), ("uint32_t", "op", 1), ("uint32_t", "flags", 1), ("float", "exposure", 1), ("float", "key", 1),
                      ("float", "white", 1), ("float", "adapt", 1), ("float", "exposure_min", 1), ("float", "exposure_max", 1),
                      ("uint32_t", "low_permille", 1), ("uint32_t", "high_permille", 1), ("uint32_t", "reserved", 5)]
    assert 4 * sum(k for _, _, k in fields) == 64
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in fields] == list(rt.host.CTonemapParams._fields_)
    assert C.sizeof(rt.host.CTonemapParams) == 64
    assert [getattr(rt.host.CTonemapParams, n).offset for _, n, _ in fields] == [4 * k for k in range(12)]
    # the enumerators the binding's integers stand for
    for name, value in (("RTGL_TONEMAP_SOURCE_IMAGE", 0), ("RTGL_TONEMAP_SOURCE_DENOISED", 1), ("RTGL_TONEMAP_SOURCE_TEMPORAL", 2),
                        ("RTGL_TONEMAP_LINEAR", 0), ("RTGL_TONEMAP_REINHARD", 1), ("RTGL_TONEMAP_ACES", 2), ("RTGL_TONEMAP_AUTO_EXPOSURE", 1)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", text), name
    assert rt.host.TONEMAP_AUTO_EXPOSURE == 1


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_and_mirror_state_the_same_defaults(rt):
    import tonemap_mirror
    lib = rt.host.load_library()
    p = rt.host.CTonemapParams(source=9, op=9, flags=6, exposure=-1, key=-1, white=0, adapt=7, exposure_min=3, exposure_max=2,
                               low_permille=999, high_permille=999, reserved=(1, 2, 3, 4, 5))
    assert lib.rtgl_tonemap_defaults(C.byref(p)) == 0
    assert lib.rtgl_tonemap_defaults(None) == ERR_INVALID
    d = rt.host.TONEMAP_DEFAULTS
    assert list(p.reserved) == [0] * 5
    assert (p.source, p.op, p.low_permille, p.high_permille) == (d["source"], d["op"], d["low_permille"], d["high_permille"])
    assert bool(p.flags & 1) == d["auto"] and p.flags in (0, 1)
    for name in ("exposure", "key", "white", "adapt", "exposure_min", "exposure_max"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(source=0, op=1, auto=True, exposure=1.0, key=0.18, white=4.0, adapt=1.0, exposure_min=2.0 ** -16, exposure_max=2.0 ** 16,
                     low_permille=100, high_permille=20)
    assert tonemap_mirror.DEFAULTS == d
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (int(g[0]), int(g[1]), float(g[2]), float(g[3]), float(g[4]), float(g[5]), 2.0 ** -int(g[6]), 2.0 ** int(g[7]), int(g[8]), int(g[9])) == \
            (d["source"], d["op"], d["exposure"], d["key"], d["white"], d["adapt"], d["exposure_min"], d["exposure_max"], d["low_permille"], d["high_permille"]), path


def invalid_blocks(rt):
    lib = rt.host.load_library()

    def block(**kw):
        p = rt.host.CTonemapParams()
        lib.rtgl_tonemap_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return [block(source=3), block(op=3), block(flags=2), block(flags=3), block(exposure=nan), block(exposure=0.0), block(exposure=-1.0),
            block(key=inf), block(key=0.0), block(white=nan), block(white=-4.0), block(adapt=0.0), block(adapt=1.5), block(adapt=nan),
            block(exposure_min=0.0), block(exposure_max=inf), block(exposure_min=4.0, exposure_max=2.0),
            block(low_permille=500, high_permille=500), block(low_permille=1000, high_permille=0), block(low_permille=0xFFFFFFFF, high_permille=1),
            block(reserved=(0, 0, 0, 0, 1))]


def test_calls_reject_a_null_context_and_null_outputs(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    p = rt.host.CTonemapParams()
    lib.rtgl_tonemap_defaults(C.byref(p))
    assert lib.rtgl_tonemap(None, None) == ERR_INVALID
    assert lib.rtgl_tonemap(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_blocks(rt):
        assert lib.rtgl_tonemap(None, C.byref(bad)) == ERR_INVALID
    assert lib.rtgl_tonemap_reset(None) == ERR_INVALID
    px, e, hist, ign = (C.c_uint8 * 4)(), C.c_float(), (C.c_uint32 * 256)(), C.c_uint32()
    assert lib.rtgl_read_display_u8(None, px, 0) == ERR_INVALID
    assert lib.rtgl_read_tonemap_exposure(None, C.byref(e)) == ERR_INVALID
    assert lib.rtgl_read_tonemap_histogram(None, hist, C.byref(ign)) == ERR_INVALID
    assert not lib.rtgl_device_display(None)


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_tonemap_params p;
    uint8_t px[4];
    uint32_t hist[256], ignored;
    float e;
    int rc = rtgl_tonemap_defaults(&p);
    p.source = RTGL_TONEMAP_SOURCE_TEMPORAL; p.op = RTGL_TONEMAP_ACES; p.flags = RTGL_TONEMAP_AUTO_EXPOSURE;
    p.exposure = 2.0f; p.key = 0.25f; p.white = 8.0f; p.adapt = 0.5f; p.exposure_min = 0.125f; p.exposure_max = 64.0f;
    p.low_permille = 50u; p.high_permille = 50u; p.reserved[4] = 0u;
    rc |= rtgl_tonemap((rtgl_context *)0, &p);
    rc |= rtgl_tonemap((rtgl_context *)0, (const rtgl_tonemap_params *)0);
    rc |= rtgl_tonemap_reset((rtgl_context *)0);
    rc |= rtgl_read_display_u8((rtgl_context *)0, px, 1);
    rc |= rtgl_read_tonemap_exposure((rtgl_context *)0, &e);
    rc |= rtgl_read_tonemap_histogram((rtgl_context *)0, hist, &ignored);
    rc |= rtgl_device_display((rtgl_context *)0) != (void *)0;
    return rc + (int)(sizeof p != 64);
}
"""

FACADE_TONEMAP = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_frame_budget(2);
    r.run();
    bool ok = r.tonemap();
    rtgl_tonemap_params p;
    rtgl_tonemap_defaults(&p);
    p.op = RTGL_TONEMAP_ACES; p.flags = 0u; p.exposure = 0.5f;
    ok = r.tonemap(&p) && ok;
    const std::vector<uint8_t> px = r.read_display(), top_first = r.read_display(true);
    ok = r.save_display_png("display.png") && ok;
    return ok && px.size() == (size_t)64 * 48 * 4 && top_first.size() == px.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "tonemap.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_tonemap.cpp"
    src.write_text(FACADE_TONEMAP)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_tonemap_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt(\d+)(tonemap_\w+?_kernel)(?:ILi([012])EEEv)?", name)
        if m:
            found[(m.group(2), m.group(3))] = r
    assert sorted(found) == [("tonemap_histogram_kernel", None), ("tonemap_map_kernel", "0"), ("tonemap_map_kernel", "1"), ("tonemap_map_kernel", "2"),
                             ("tonemap_solve_kernel", None)], sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        # four per-wave histograms of 256 bins and the `ignored` word; none; the 256 thresholds
        lds = {"tonemap_histogram_kernel": 4 * 257 * 4, "tonemap_solve_kernel": 0, "tonemap_map_kernel": 256 * 4}[key[0]]
        assert r["LDS Size"] == lds, f"{key}: {r}"
        # streaming kernels: nothing but the registers may limit the waves per SIMD, and they must not (8 is the most the report states)
        assert r["Occupancy"] >= 8, f"{key}: {r}"
        assert r["VGPRs"] <= 64, f"{key}: {r}"
