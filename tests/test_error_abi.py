"""The error estimate (rtgl_error_estimate, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the
library agree on the entry points and on the three layouts; header, binding, facade, library and mirror state the same defaults; the calls
reject a NULL context, whatever the record, before touching a device (the record's rules: tests/test_post_plans.py); a C99 program compiles against the header and the facade's methods
with the host compilers; and the kernels spill nothing and hold the LDS they were designed for (compiler resource report)."""
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
ENTRY_POINTS = ["rtgl_error_defaults", "rtgl_error_estimate", "rtgl_error_reset", "rtgl_read_error_summary", "rtgl_read_error_tiles",
                "rtgl_device_error_tiles"]
DEFAULTS_TEXT = r"threshold ([\d.]+), floor ([\d.]+),\s+(?:\*\s+|//\s+)?quantile_permille (\d+), first_frames (\d+), flags (\d+)"
ERR_INVALID = -1
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}


def header_text():
    with open(HEADER) as f:
        return f.read()


def struct_fields(text, name):
    body = re.search(rf"typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|int32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]


def test_header_declares_the_entry_points_and_the_three_layouts(rt):
    text = header_text()
    ctx = r"rtgl_context\s*\*\s*\w+"
    for decl in (r"\bint\s+rtgl_error_defaults\s*\(\s*rtgl_error_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_error_estimate\s*\(\s*{ctx}\s*,\s*const\s+rtgl_error_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_error_reset\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_read_error_summary\s*\(\s*{ctx}\s*,\s*rtgl_error_summary\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_error_tiles\s*\(\s*{ctx}\s*,\s*rtgl_error_tile\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bvoid\s*\*\s*rtgl_device_error_tiles\s*\(\s*{ctx}\s*\)\s*;"):
        assert re.search(decl, text), decl
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    H_ = rt.host
    params = struct_fields(text, "rtgl_error_params")
    assert params == [("float", "threshold", 1), ("float", "floor", 1), ("uint32_t", "quantile_permille", 1), ("int32_t", "first_frames", 1),
                      ("uint32_t", "flags", 1), ("uint32_t", "reserved", 3)]
    summary = struct_fields(text, "rtgl_error_summary")
    assert summary == [("uint32_t", "valid", 1), ("uint32_t", "converged", 1), ("int32_t", "frames_now", 1), ("int32_t", "frames_snapshot", 1),
                       ("uint32_t", "tiles_valid", 1), ("uint32_t", "tiles_converged", 1), ("uint32_t", "pixels_ignored", 1), ("float", "scale", 1),
                       ("float", "mse", 1), ("float", "max_tile_mse", 1), ("uint32_t", "reserved", 6)]
    tile = struct_fields(text, "rtgl_error_tile")
    assert tile == [("float", "sum", 1), ("float", "mse", 1), ("uint32_t", "count", 1), ("uint32_t", "converged", 1)]
    for fields, ctype, size in ((params, H_.CErrorParams, 32), (summary, H_.CErrorSummary, 64)):
        assert 4 * sum(k for _, _, k in fields) == size == C.sizeof(ctype)
        assert [(n, CTYPE[t] * k if k > 1 else CTYPE[t]) for t, n, k in fields] == list(ctype._fields_)
        offsets, at = [], 0
        for _, _, k in fields:
            offsets.append(at)
            at += 4 * k
        assert [getattr(ctype, n).offset for _, n, _ in fields] == offsets
    assert H_.ERROR_TILE_DTYPE.itemsize == 16 == 4 * len(tile)
    assert [(n, H_.ERROR_TILE_DTYPE.fields[n][0], H_.ERROR_TILE_DTYPE.fields[n][1]) for _, n, _ in tile] == \
        [("sum", np.dtype(np.float32), 0), ("mse", np.dtype(np.float32), 4), ("count", np.dtype(np.uint32), 8), ("converged", np.dtype(np.uint32), 12)]
    assert re.search(r"\bRTGL_ERROR_KEEP_SNAPSHOT\s*=\s*1\b", text) and H_.ERROR_KEEP_SNAPSHOT == 1


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import error_mirror
    lib = rt.host.load_library()
    p = rt.host.CErrorParams(threshold=-1, floor=0, quantile_permille=0, first_frames=-5, flags=6, reserved=(1, 2, 3))
    assert lib.rtgl_error_defaults(C.byref(p)) == 0
    assert lib.rtgl_error_defaults(None) == ERR_INVALID
    d = rt.host.ERROR_DEFAULTS
    assert list(p.reserved) == [0] * 3 and p.flags == 0 and d["keep_snapshot"] is False
    assert (p.quantile_permille, p.first_frames) == (d["quantile_permille"], d["first_frames"])
    for name in ("threshold", "floor"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(threshold=0.05, floor=0.01, quantile_permille=950, first_frames=1, keep_snapshot=False)
    assert error_mirror.DEFAULTS == d
    assert error_mirror.TILE_DTYPE == rt.host.ERROR_TILE_DTYPE
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (float(g[0]), float(g[1]), int(g[2]), int(g[3]), bool(int(g[4]))) == \
            (d["threshold"], d["floor"], d["quantile_permille"], d["first_frames"], d["keep_snapshot"]), path


def invalid_blocks(rt):
    lib = rt.host.load_library()

    def block(**kw):
        p = rt.host.CErrorParams()
        lib.rtgl_error_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return [block(threshold=nan), block(threshold=inf), block(threshold=0.0), block(threshold=-0.05), block(floor=nan), block(floor=inf),
            block(floor=0.0), block(floor=-0.01), block(quantile_permille=0), block(quantile_permille=1001), block(quantile_permille=0xFFFFFFFF),
            block(first_frames=-1), block(flags=2), block(flags=3), block(reserved=(0, 0, 1)), block(reserved=(1, 0, 0))]


def test_calls_reject_a_null_context_and_null_outputs(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    p = rt.host.CErrorParams()
    lib.rtgl_error_defaults(C.byref(p))
    assert lib.rtgl_error_estimate(None, None) == ERR_INVALID
    assert lib.rtgl_error_estimate(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_blocks(rt):
        assert lib.rtgl_error_estimate(None, C.byref(bad)) == ERR_INVALID
    assert lib.rtgl_error_reset(None) == ERR_INVALID
    s, tiles, tx, ty = rt.host.CErrorSummary(), (C.c_uint32 * 4)(), C.c_uint32(), C.c_uint32()
    assert lib.rtgl_read_error_summary(None, C.byref(s)) == ERR_INVALID
    assert lib.rtgl_read_error_tiles(None, tiles, C.byref(tx), C.byref(ty)) == ERR_INVALID
    assert not lib.rtgl_device_error_tiles(None)


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_error_params p;
    rtgl_error_summary s;
    rtgl_error_tile tiles[4];
    uint32_t tx, ty;
    int rc = rtgl_error_defaults(&p);
    p.threshold = 0.02f; p.floor = 0.001f; p.quantile_permille = 990u; p.first_frames = 0; p.flags = RTGL_ERROR_KEEP_SNAPSHOT; p.reserved[2] = 0u;
    rc |= rtgl_error_estimate((rtgl_context *)0, &p);
    rc |= rtgl_error_estimate((rtgl_context *)0, (const rtgl_error_params *)0);
    rc |= rtgl_error_reset((rtgl_context *)0);
    rc |= rtgl_read_error_summary((rtgl_context *)0, &s);
    rc |= rtgl_read_error_tiles((rtgl_context *)0, tiles, &tx, &ty);
    rc |= rtgl_device_error_tiles((rtgl_context *)0) != (void *)0;
    return rc + (int)(sizeof p != 32) + (int)(sizeof s != 64) + (int)(sizeof tiles[0] != 16);
}
"""

FACADE_ERROR = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_frame_budget(8);
    r.run();
    bool ok = r.error_estimate();
    r.run();
    rtgl_error_params p;
    rtgl_error_defaults(&p);
    p.flags = RTGL_ERROR_KEEP_SNAPSHOT; p.threshold = 0.1f;
    ok = r.error_estimate(&p) && ok;
    rtgl_error_summary s = r.read_error_summary();
    const long frames = r.render_until(0.2f, 64);
    const long more = r.render_until(0.1f, 256, 32, &p, &s);
    return ok && frames <= 64 && more <= 256 && s.frames_now >= s.frames_snapshot ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "error.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_error.cpp"
    src.write_text(FACADE_ERROR)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_error_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt(\d+)(error_\w+?_kernel)(?:ILb([01])ELb([01])EEEv)?", name)
        if m:
            found[(m.group(2), m.group(3), m.group(4))] = r
    assert sorted(found, key=str) == sorted([("error_solve_kernel", None, None), ("error_tiles_kernel", "0", "0"), ("error_tiles_kernel", "1", "0"),
                                             ("error_tiles_kernel", "1", "1")], key=str), sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        # the four waves' partial sums and counts; none where the records are only zeroed; the solve's four partial sums, a 64-bit count and
        # three 32-bit words
        lds = {("error_tiles_kernel", "1"): 32, ("error_tiles_kernel", "0"): 0, ("error_solve_kernel", None): 40}[key[:2]]
        assert r["LDS Size"] == lds, f"{key}: {r}"
        # streaming kernels: the registers must not limit the waves per SIMD (8 is the most the report states)
        assert r["Occupancy"] >= 8, f"{key}: {r}"
        assert r["VGPRs"] <= (64 if key[0] == "error_solve_kernel" else 16), f"{key}: {r}"     # (the solve holds 32 words of records in flight)
