"""The robust error estimate (rtgl_robust_error_estimate, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding
and the library agree on the entry points and on the layout; header, binding, facade, library and mirror state the same defaults; the
calls reject a NULL context and invalid arguments before touching a device; a C99 program compiles against the header and the facade's
methods with the host compilers; the host half (rt_spread_plan.hpp) passes its stand-alone program under the address and
undefined-behaviour sanitizers; and the three kernels spill nothing, use no scratch and hold 32 bytes of LDS (compiler resource report)."""
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
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
ENTRY_POINTS = ["rtgl_robust_error_defaults", "rtgl_robust_error_estimate", "rtgl_read_robust_error_summary", "rtgl_read_robust_error_tiles",
                "rtgl_device_robust_error_tiles"]
DEFAULTS_TEXT = r"threshold ([\d.]+),\s+(?:\*\s+|//\s+)?floor ([\d.]+), (?:the resolve's )?gain ([\d.]+), quantile(?:_permille)? (\d+), flags (\d+)"
ERR_INVALID = -1
CTYPE = {"uint32_t": C.c_uint32, "float": C.c_float}


def header_text():
    with open(HEADER) as f:
        return f.read()


def struct_fields(text, name):
    body = re.search(rf"typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]


def test_header_declares_the_entry_points_and_the_layout(rt):
    text = header_text()
    ctx = r"rtgl_context\s*\*\s*\w+"
    for decl in (r"\bint\s+rtgl_robust_error_defaults\s*\(\s*rtgl_robust_error_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_error_estimate\s*\(\s*{ctx}\s*,\s*const\s+rtgl_robust_error_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_error_summary\s*\(\s*{ctx}\s*,\s*rtgl_error_summary\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_error_tiles\s*\(\s*{ctx}\s*,\s*rtgl_error_tile\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bvoid\s*\*\s*rtgl_device_robust_error_tiles\s*\(\s*{ctx}\s*\)\s*;"):
        assert re.search(decl, text), decl
    H_ = rt.host
    assert set(ENTRY_POINTS) <= set(H_.ABI_SYMBOLS)
    assert text.index("robust error estimate") > text.index("robust accumulation")      # behind the robust section
    fields = struct_fields(text, "rtgl_robust_error_params")
    assert fields == [("float", "threshold", 1), ("float", "floor", 1), ("float", "gain", 1), ("uint32_t", "quantile_permille", 1), ("uint32_t", "flags", 1),
                      ("uint32_t", "reserved", 3)]
    ctype = H_.CRobustErrorParams
    assert 4 * sum(k for _, _, k in fields) == 32 == C.sizeof(ctype)
    assert [(n, CTYPE[t] * k if k > 1 else CTYPE[t]) for t, n, k in fields] == list(ctype._fields_)
    offsets, at = [], 0
    for _, _, k in fields:
        offsets.append(at)
        at += 4 * k
    assert [getattr(ctype, n).offset for _, n, _ in fields] == offsets


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import robust_error_mirror
    lib = rt.host.load_library()
    p = rt.host.CRobustErrorParams(threshold=-1, floor=0, gain=-3, quantile_permille=0, flags=6, reserved=(1, 2, 3))
    assert lib.rtgl_robust_error_defaults(C.byref(p)) == 0
    assert lib.rtgl_robust_error_defaults(None) == ERR_INVALID
    d = rt.host.ROBUST_ERROR_DEFAULTS
    assert list(p.reserved) == [0] * 3 and p.flags == 0 and p.quantile_permille == d["quantile_permille"]
    for name in ("threshold", "floor", "gain"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950)
    assert robust_error_mirror.DEFAULTS == d and robust_error_mirror.TILE_DTYPE == rt.host.ERROR_TILE_DTYPE
    assert robust_error_mirror.valid_params(**d)
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (float(g[0]), float(g[1]), float(g[2]), int(g[3]), int(g[4])) == (d["threshold"], d["floor"], d["gain"], d["quantile_permille"], 0), path


def invalid_blocks(rt):
    lib = rt.host.load_library()

    def block(**kw):
        p = rt.host.CRobustErrorParams()
        lib.rtgl_robust_error_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return [block(threshold=nan), block(threshold=inf), block(threshold=0.0), block(threshold=-0.05), block(floor=nan), block(floor=inf), block(floor=0.0),
            block(floor=-0.01), block(gain=nan), block(gain=inf), block(gain=-inf), block(gain=-1.0), block(gain=-1e-30), block(quantile_permille=0),
            block(quantile_permille=1001), block(quantile_permille=0xFFFFFFFF), block(flags=1), block(flags=0x80000000), block(reserved=(0, 0, 1)),
            block(reserved=(1, 0, 0))]


def test_calls_reject_a_null_context_and_null_outputs(rt):
    lib = rt.host.load_library()
    p = rt.host.CRobustErrorParams()
    lib.rtgl_robust_error_defaults(C.byref(p))
    assert lib.rtgl_robust_error_estimate(None, None) == ERR_INVALID and lib.rtgl_robust_error_estimate(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_blocks(rt):
        assert lib.rtgl_robust_error_estimate(None, C.byref(bad)) == ERR_INVALID
    s, tiles, tx, ty = rt.host.CErrorSummary(), (C.c_uint32 * 4)(), C.c_uint32(), C.c_uint32()
    assert lib.rtgl_read_robust_error_summary(None, C.byref(s)) == ERR_INVALID and lib.rtgl_read_robust_error_summary(None, None) == ERR_INVALID
    assert lib.rtgl_read_robust_error_tiles(None, tiles, C.byref(tx), C.byref(ty)) == ERR_INVALID
    assert not lib.rtgl_device_robust_error_tiles(None)


def test_the_mirror_refuses_what_the_library_refuses(rt):
    """the records the device test sends to a live context are the ones the mirror's validation refuses"""
    import robust_error_mirror
    for bad in invalid_blocks(rt):
        assert not robust_error_mirror.valid_params(bad.threshold, bad.floor, bad.gain, bad.quantile_permille, bad.flags, tuple(bad.reserved))


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_robust_error_params p;
    rtgl_error_summary s;
    rtgl_error_tile tiles[4];
    uint32_t tx, ty;
    int rc = rtgl_robust_error_defaults(&p);
    p.threshold = 0.02f; p.floor = 0.001f; p.gain = 0.5f; p.quantile_permille = 990u; p.flags = 0u; p.reserved[2] = 0u;
    rc |= rtgl_robust_error_estimate((rtgl_context *)0, &p);
    rc |= rtgl_robust_error_estimate((rtgl_context *)0, (const rtgl_robust_error_params *)0);
    rc |= rtgl_read_robust_error_summary((rtgl_context *)0, &s);
    rc |= rtgl_read_robust_error_tiles((rtgl_context *)0, tiles, &tx, &ty);
    rc |= rtgl_device_robust_error_tiles((rtgl_context *)0) != (void *)0;
    return rc + (int)(sizeof p != 32) + (int)(sizeof s != 64) + (int)(sizeof tiles[0] != 16);
}
"""

FACADE_ROBUST_ERROR = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    bool ok = r.robust_begin();
    for (int k = 0; k < 8; ++k) ok = r.robust_frame() && ok;
    ok = r.robust_error_estimate() && ok;
    rtgl_robust_error_params p;
    rtgl_robust_error_defaults(&p);
    p.gain = 0.0f; p.threshold = 0.1f;
    ok = r.robust_error_estimate(&p) && ok;
    rtgl_error_summary s = r.read_robust_error_summary();
    const long frames = r.render_robust_until(0.2f, 64);
    const long more = r.render_robust_until(0.1f, 256, 32, 16, 0.5f, true, &p, &s);
    return ok && frames <= 64 && more <= 256 && s.frames_snapshot == 0 ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "robust_error.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_robust_error.cpp"
    src.write_text(FACADE_ROBUST_ERROR)
    for path in (str(src), os.path.join(ROOT, "tests", "cpp", "facade_robust_until.cpp")):      # the methods alone, and the device test's driver
        out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", inc, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]


def test_spread_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "spread_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "spread_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    with open(os.path.join(CSRC, "rt_spread_plan.hpp")) as f:
        header = f.read()
    assert set(re.findall(r"#include\s+(\S+)", header)) == {"<cmath>", "<cstddef>", "<cstdint>"}
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for name in ("default_params", "invalid", "refused", "footprint_side", "footprint", "footprint_fits", "tiles_along", "record_bytes"):
        assert f"rt_spread_plan::{name}(" in code, name
    with open(os.path.join(CSRC, "rt_spread.hpp")) as f:
        kernels = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "#pragma clang fp contract(off)" in kernels and "atomic" not in kernels and "error_wave_tree(" in kernels and "store_through(" in kernels


@pytest.fixture(scope="module")
def resource_report():
    return report()


# VGPRs and waves per SIMD as the build gives them: K -> (VGPRs, occupancy)
SPREAD_PINS = {4: (21, 8), 8: (36, 8), 16: (74, 6)}


def test_spread_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt\d+spread_tiles_kernelILi(\d+)EEEvNS_\d+SpreadTilesArgsE$", name)
        if m:
            found[int(m.group(1))] = r
        else:
            assert "spread" not in name, name                      # exactly these: nothing else carries the name
    assert sorted(found) == sorted(SPREAD_PINS), sorted(resource_report)
    for K, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{K}: {r}"
        assert r["LDS Size"] == 32, f"{K}: {r}"                    # the four waves' partial sums and counts
        assert (r["VGPRs"], r["Occupancy"]) == SPREAD_PINS[K], f"{K}: {r}"
