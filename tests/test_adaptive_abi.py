"""Adaptive sampling (rtgl_adaptive_*, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the library
agree on the entry points and on the three layouts; header, binding, facade, library and mirror state the same defaults; the calls reject a
NULL context and invalid arguments before touching a device; a C99 program compiles against the header and the facade's methods with the
host compilers; the host half (rt_adaptive_plan.hpp) passes its stand-alone program under the address and undefined-behaviour sanitizers;
and the three kernels spill nothing, use no scratch and hold the LDS they were designed for (compiler resource report)."""
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
ENTRY_POINTS = ["rtgl_adaptive_defaults", "rtgl_adaptive_begin", "rtgl_adaptive_frame", "rtgl_adaptive_update", "rtgl_adaptive_set_mask",
                "rtgl_adaptive_get_mask", "rtgl_read_adaptive_tiles", "rtgl_device_adaptive_tiles"]
DEFAULTS_TEXT = r"threshold ([\d.]+), floor ([\d.]+), min_samples (\d+), max_samples\s+(?:\*\s+|//\s+)?(\d+), flags (\d+)"
ERR_INVALID = -1
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float, "uint64_t": C.c_uint64}
SIZE = {"uint32_t": 4, "int32_t": 4, "float": 4, "uint64_t": 8}


def header_text():
    with open(HEADER) as f:
        return f.read()


def struct_fields(text, name):
    body = re.search(rf"typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|int32_t|uint64_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]


def test_header_declares_the_entry_points_and_the_three_layouts(rt):
    text = header_text()
    ctx = r"rtgl_context\s*\*\s*\w+"
    for decl in (r"\bint\s+rtgl_adaptive_defaults\s*\(\s*rtgl_adaptive_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_adaptive_begin\s*\(\s*{ctx}\s*,\s*const\s+rtgl_adaptive_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_adaptive_frame\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_adaptive_update\s*\(\s*{ctx}\s*,\s*rtgl_adaptive_summary\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_adaptive_set_mask\s*\(\s*{ctx}\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_adaptive_get_mask\s*\(\s*{ctx}\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_adaptive_tiles\s*\(\s*{ctx}\s*,\s*rtgl_adaptive_tile\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bvoid\s*\*\s*rtgl_device_adaptive_tiles\s*\(\s*{ctx}\s*\)\s*;"):
        assert re.search(decl, text), decl
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    H_ = rt.host
    params = struct_fields(text, "rtgl_adaptive_params")
    assert params == [("float", "threshold", 1), ("float", "floor", 1), ("uint32_t", "min_samples", 1), ("uint32_t", "max_samples", 1),
                      ("uint32_t", "flags", 1), ("uint32_t", "reserved", 3)]
    summary = struct_fields(text, "rtgl_adaptive_summary")
    assert summary == [("uint32_t", "tiles_total", 1), ("uint32_t", "tiles_active", 1), ("uint32_t", "tiles_converged", 1), ("uint32_t", "tiles_capped", 1),
                       ("uint32_t", "blocks_active", 1), ("uint32_t", "samples_min", 1), ("uint32_t", "samples_max", 1), ("uint32_t", "converged", 1),
                       ("uint64_t", "samples_total", 1), ("float", "max_tile_mse", 1), ("uint32_t", "reserved", 5)]
    tile = struct_fields(text, "rtgl_adaptive_tile")
    assert tile == [("float", "sum", 1), ("float", "mse", 1), ("uint32_t", "count", 1), ("uint32_t", "converged", 1), ("uint32_t", "samples", 1),
                    ("uint32_t", "samples_snapshot", 1), ("uint32_t", "reserved", 2)]
    for fields, ctype, size in ((params, H_.CAdaptiveParams, 32), (summary, H_.CAdaptiveSummary, 64)):
        assert sum(SIZE[t] * k for t, _, k in fields) == size == C.sizeof(ctype)
        assert [(n, CTYPE[t] * k if k > 1 else CTYPE[t]) for t, n, k in fields] == list(ctype._fields_)
        offsets, at = [], 0
        for t, _, k in fields:
            assert at % SIZE[t] == 0                          # (no padding anywhere: the sizes add up)
            offsets.append(at)
            at += SIZE[t] * k
        assert [getattr(ctype, n).offset for _, n, _ in fields] == offsets
    dt = H_.ADAPTIVE_TILE_DTYPE
    assert dt.itemsize == 32 == 4 * sum(k for _, _, k in tile)
    assert [(n, dt.fields[n][1]) for _, n, _ in tile] == [("sum", 0), ("mse", 4), ("count", 8), ("converged", 12), ("samples", 16), ("samples_snapshot", 20), ("reserved", 24)]
    assert dt.fields["sum"][0] == dt.fields["mse"][0] == np.dtype(np.float32) and dt.fields["samples"][0] == np.dtype(np.uint32)


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import adaptive_mirror
    lib = rt.host.load_library()
    p = rt.host.CAdaptiveParams(threshold=-1, floor=0, min_samples=0, max_samples=0, flags=6, reserved=(1, 2, 3))
    assert lib.rtgl_adaptive_defaults(C.byref(p)) == 0
    assert lib.rtgl_adaptive_defaults(None) == ERR_INVALID
    d = rt.host.ADAPTIVE_DEFAULTS
    assert list(p.reserved) == [0] * 3 and p.flags == 0
    assert (p.min_samples, p.max_samples) == (d["min_samples"], d["max_samples"])
    for name in ("threshold", "floor"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(threshold=0.05, floor=0.01, min_samples=16, max_samples=1024)
    assert adaptive_mirror.DEFAULTS == d
    assert adaptive_mirror.TILE_DTYPE == rt.host.ADAPTIVE_TILE_DTYPE
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (float(g[0]), float(g[1]), int(g[2]), int(g[3]), int(g[4])) == (d["threshold"], d["floor"], d["min_samples"], d["max_samples"], 0), path


def invalid_blocks(rt):
    lib = rt.host.load_library()

    def block(**kw):
        p = rt.host.CAdaptiveParams()
        lib.rtgl_adaptive_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return [block(threshold=nan), block(threshold=inf), block(threshold=0.0), block(threshold=-0.05), block(floor=nan), block(floor=inf),
            block(floor=0.0), block(floor=-0.01), block(min_samples=0), block(min_samples=17, max_samples=16), block(max_samples=0),
            block(flags=1), block(flags=0x80000000), block(reserved=(0, 0, 1)), block(reserved=(1, 0, 0))]


def test_calls_reject_a_null_context_and_null_outputs(rt):
    lib = rt.host.load_library()
    p = rt.host.CAdaptiveParams()
    lib.rtgl_adaptive_defaults(C.byref(p))
    assert lib.rtgl_adaptive_begin(None, None) == ERR_INVALID
    assert lib.rtgl_adaptive_begin(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_blocks(rt):
        assert lib.rtgl_adaptive_begin(None, C.byref(bad)) == ERR_INVALID
    s, tiles, mask, tx, ty = rt.host.CAdaptiveSummary(), (C.c_uint32 * 8)(), (C.c_uint8 * 4)(), C.c_uint32(), C.c_uint32()
    assert lib.rtgl_adaptive_frame(None) == ERR_INVALID
    assert lib.rtgl_adaptive_update(None, C.byref(s)) == ERR_INVALID
    assert lib.rtgl_adaptive_update(None, None) == ERR_INVALID
    assert lib.rtgl_adaptive_set_mask(None, mask) == ERR_INVALID
    assert lib.rtgl_adaptive_get_mask(None, mask) == ERR_INVALID
    assert lib.rtgl_read_adaptive_tiles(None, tiles, C.byref(tx), C.byref(ty)) == ERR_INVALID
    assert not lib.rtgl_device_adaptive_tiles(None)


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_adaptive_params p;
    rtgl_adaptive_summary s;
    rtgl_adaptive_tile tiles[4];
    uint8_t mask[4] = {1, 0, 0, 1};
    uint32_t tx, ty;
    int rc = rtgl_adaptive_defaults(&p);
    p.threshold = 0.02f; p.floor = 0.001f; p.min_samples = 8u; p.max_samples = 256u; p.flags = 0u; p.reserved[2] = 0u;
    rc |= rtgl_adaptive_begin((rtgl_context *)0, &p);
    rc |= rtgl_adaptive_set_mask((rtgl_context *)0, mask);
    rc |= rtgl_adaptive_frame((rtgl_context *)0);
    rc |= rtgl_adaptive_update((rtgl_context *)0, &s);
    rc |= rtgl_adaptive_get_mask((rtgl_context *)0, mask);
    rc |= rtgl_read_adaptive_tiles((rtgl_context *)0, tiles, &tx, &ty);
    rc |= rtgl_device_adaptive_tiles((rtgl_context *)0) != (void *)0;
    return rc + (int)(sizeof p != 32) + (int)(sizeof s != 64) + (int)(sizeof tiles[0] != 32);
}
"""

FACADE_ADAPTIVE = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    bool ok = r.adaptive_begin();
    std::vector<uint8_t> mask = r.adaptive_get_mask();
    ok = r.adaptive_set_mask(mask) && ok;
    ok = r.adaptive_frame() && ok;
    rtgl_adaptive_summary s;
    ok = r.adaptive_update(&s) && ok;
    std::vector<rtgl_adaptive_tile> tiles = r.read_adaptive_tiles();
    const long frames = r.render_adaptive(0.1f, 64);
    const long more = r.render_adaptive(0.05f, 256, 8, 32, &s);
    return ok && frames >= 0 && more >= 0 && s.samples_max >= s.samples_min && tiles.size() == mask.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "adaptive.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_adaptive.cpp"
    src.write_text(FACADE_ADAPTIVE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


def test_adaptive_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "adaptive_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "adaptive_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    with open(os.path.join(CSRC, "rt_adaptive_plan.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<cstddef>", "<cstdint>", "<vector>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for name in ("shape", "explicit_mask", "build_lists", "active", "summary"):
        assert f"rt_adaptive_plan::{name}(" in code, name


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_adaptive_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt\d+(generate_rays_masked_kernel|adaptive_merge_kernel|adaptive_tiles_kernel)E", name)
        if m:
            found[m.group(1)] = r
    assert sorted(found) == ["adaptive_merge_kernel", "adaptive_tiles_kernel", "generate_rays_masked_kernel"], sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        # the update: the four waves' partial sums and counts; the other two hold none
        assert r["LDS Size"] == (32 if key == "adaptive_tiles_kernel" else 0), f"{key}: {r}"
        # streaming kernels: the registers must not limit the waves per SIMD (8 is the most the report states)
        assert r["Occupancy"] >= 8, f"{key}: {r}"
        assert r["VGPRs"] <= (16 if key == "adaptive_tiles_kernel" else 32), f"{key}: {r}"
