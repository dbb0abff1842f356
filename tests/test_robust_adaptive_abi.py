"""A robust adaptive session (rtgl_robust_adaptive_*, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding
and the library agree on the entry points and on the layout; header, binding, facade, library and mirror state the same defaults; the calls
reject a NULL context and invalid records before touching a device; a C99 program compiles against the header and the facade's methods with
the host compilers; the host half (rt_robust_tiles_plan.hpp) passes its stand-alone program under the address and undefined-behaviour
sanitizers; and the three kernels spill nothing, use no scratch and hold the LDS they were designed for (compiler resource report)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import robust_adaptive_inputs as rai
from resource_report import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtgl_amd.h")
FACADE = os.path.join(ROOT, "include", "rtgl", "renderer.h")
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
ENTRY_POINTS = ["rtgl_robust_adaptive_defaults", "rtgl_robust_adaptive_begin", "rtgl_robust_adaptive_frame", "rtgl_robust_adaptive_accumulate",
                "rtgl_robust_adaptive_update", "rtgl_robust_adaptive_set_mask", "rtgl_robust_adaptive_get_mask", "rtgl_robust_adaptive_resolve",
                "rtgl_robust_adaptive_end", "rtgl_read_robust_adaptive_f32", "rtgl_read_robust_adaptive_bucket_f32", "rtgl_read_robust_adaptive_tiles",
                "rtgl_device_robust_adaptive_tiles"]
DEFAULTS_TEXT = r"buckets (\d+), threshold ([\d.]+), floor ([\d.]+), gain ([\d.]+), min_samples (\d+),\s+(?:\*\s+|//\s+)?max_samples (\d+), flags (\d+)"
ERR_INVALID = -1
SIZE = {"uint32_t": 4, "float": 4}
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
    for decl in (r"\bint\s+rtgl_robust_adaptive_defaults\s*\(\s*rtgl_robust_adaptive_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_begin\s*\(\s*{ctx}\s*,\s*const\s+rtgl_robust_adaptive_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_frame\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_accumulate\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_update\s*\(\s*{ctx}\s*,\s*rtgl_adaptive_summary\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_set_mask\s*\(\s*{ctx}\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_get_mask\s*\(\s*{ctx}\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_resolve\s*\(\s*{ctx}\s*,\s*const\s+rtgl_robust_resolve_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_adaptive_end\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_adaptive_f32\s*\(\s*{ctx}\s*,\s*float\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_adaptive_bucket_f32\s*\(\s*{ctx}\s*,\s*uint32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_adaptive_tiles\s*\(\s*{ctx}\s*,\s*rtgl_adaptive_tile\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bvoid\s*\*\s*rtgl_device_robust_adaptive_tiles\s*\(\s*{ctx}\s*\)\s*;"):
        assert re.search(decl, text), decl
    H_ = rt.host
    assert set(ENTRY_POINTS) <= set(H_.ABI_SYMBOLS)
    params = struct_fields(text, "rtgl_robust_adaptive_params")
    assert params == [("uint32_t", "buckets", 1), ("float", "threshold", 1), ("float", "floor", 1), ("float", "gain", 1), ("uint32_t", "min_samples", 1),
                      ("uint32_t", "max_samples", 1), ("uint32_t", "flags", 1), ("uint32_t", "reserved", 1)]
    ctype = H_.CRobustAdaptiveParams
    assert sum(SIZE[t] * k for t, _, k in params) == 32 == C.sizeof(ctype)
    assert [(n, CTYPE[t]) for t, n, _ in params] == list(ctype._fields_)
    assert [getattr(ctype, n).offset for _, n, _ in params] == [4 * i for i in range(8)]


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import robust_adaptive_mirror
    lib = rt.host.load_library()
    p = rt.host.CRobustAdaptiveParams(buckets=3, threshold=-1, floor=0, gain=-2, min_samples=0, max_samples=0, flags=6, reserved=9)
    assert lib.rtgl_robust_adaptive_defaults(C.byref(p)) == 0
    assert lib.rtgl_robust_adaptive_defaults(None) == ERR_INVALID
    d = rt.host.ROBUST_ADAPTIVE_DEFAULTS
    assert (p.buckets, p.min_samples, p.max_samples, p.flags, p.reserved) == (d["buckets"], d["min_samples"], d["max_samples"], 0, 0)
    for name in ("threshold", "floor", "gain"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(buckets=8, threshold=0.05, floor=0.01, gain=1.0, min_samples=32, max_samples=1024)
    assert robust_adaptive_mirror.DEFAULTS == d and robust_adaptive_mirror.TILE_DTYPE == rt.host.ADAPTIVE_TILE_DTYPE
    assert robust_adaptive_mirror.valid_params(**d)
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (int(g[0]), float(g[1]), float(g[2]), float(g[3]), int(g[4]), int(g[5]), int(g[6])) == (d["buckets"], d["threshold"], d["floor"], d["gain"],
                                                                                                     d["min_samples"], d["max_samples"], 0), path


def invalid_records(rt):
    lib = rt.host.load_library()
    out = []
    for bad in rai.invalid_params():
        p = rt.host.CRobustAdaptiveParams()
        lib.rtgl_robust_adaptive_defaults(C.byref(p))
        for k, v in bad.items():
            setattr(p, k, v)
        out.append(p)
    return out


def test_calls_reject_a_null_context_and_null_arguments(rt):
    lib = rt.host.load_library()
    p, r = rt.host.CRobustAdaptiveParams(), rt.host.CRobustResolveParams()
    lib.rtgl_robust_adaptive_defaults(C.byref(p))
    lib.rtgl_robust_defaults(None, C.byref(r))
    assert lib.rtgl_robust_adaptive_begin(None, None) == ERR_INVALID and lib.rtgl_robust_adaptive_begin(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_records(rt):
        assert lib.rtgl_robust_adaptive_begin(None, C.byref(bad)) == ERR_INVALID
    s, tiles, mask, tx, ty, px = rt.host.CAdaptiveSummary(), (C.c_uint32 * 8)(), (C.c_uint8 * 4)(), C.c_uint32(), C.c_uint32(), (C.c_float * 4)()
    assert lib.rtgl_robust_adaptive_frame(None) == ERR_INVALID and lib.rtgl_robust_adaptive_accumulate(None) == ERR_INVALID
    assert lib.rtgl_robust_adaptive_update(None, C.byref(s)) == ERR_INVALID and lib.rtgl_robust_adaptive_update(None, None) == ERR_INVALID
    assert lib.rtgl_robust_adaptive_set_mask(None, mask) == ERR_INVALID and lib.rtgl_robust_adaptive_get_mask(None, mask) == ERR_INVALID
    assert lib.rtgl_robust_adaptive_resolve(None, C.byref(r)) == ERR_INVALID and lib.rtgl_robust_adaptive_resolve(None, None) == ERR_INVALID
    assert lib.rtgl_robust_adaptive_end(None) == ERR_INVALID
    assert lib.rtgl_read_robust_adaptive_f32(None, px) == ERR_INVALID and lib.rtgl_read_robust_adaptive_f32(None, None) == ERR_INVALID
    assert lib.rtgl_read_robust_adaptive_bucket_f32(None, 0, px) == ERR_INVALID and lib.rtgl_read_robust_adaptive_bucket_f32(None, 99, None) == ERR_INVALID
    assert lib.rtgl_read_robust_adaptive_tiles(None, tiles, C.byref(tx), C.byref(ty)) == ERR_INVALID
    assert not lib.rtgl_device_robust_adaptive_tiles(None)


def test_the_mirror_refuses_what_the_library_refuses(rt):
    """the records the device tests send to a live context (tests/test_gpu_robust_adaptive.py) are the ones the mirror's validation refuses"""
    import robust_adaptive_mirror
    for bad in invalid_records(rt):
        assert not robust_adaptive_mirror.valid_params(bad.buckets, bad.threshold, bad.floor, bad.gain, bad.min_samples, bad.max_samples, bad.flags, bad.reserved)


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_robust_adaptive_params p;
    rtgl_robust_resolve_params r;
    rtgl_adaptive_summary s;
    rtgl_adaptive_tile tiles[4];
    uint8_t mask[4] = {1, 0, 0, 1};
    float px[4];
    uint32_t tx, ty;
    int rc = rtgl_robust_adaptive_defaults(&p);
    rc |= rtgl_robust_defaults((rtgl_robust_params *)0, &r);
    p.buckets = 16u; p.threshold = 0.02f; p.floor = 0.001f; p.gain = 0.5f; p.min_samples = 16u; p.max_samples = 256u; p.flags = 0u; p.reserved = 0u;
    r.dest = RTGL_ROBUST_DEST_IMAGE;
    rc |= rtgl_robust_adaptive_begin((rtgl_context *)0, &p);
    rc |= rtgl_robust_adaptive_set_mask((rtgl_context *)0, mask);
    rc |= rtgl_robust_adaptive_frame((rtgl_context *)0);
    rc |= rtgl_robust_adaptive_accumulate((rtgl_context *)0);
    rc |= rtgl_robust_adaptive_update((rtgl_context *)0, &s);
    rc |= rtgl_robust_adaptive_get_mask((rtgl_context *)0, mask);
    rc |= rtgl_robust_adaptive_resolve((rtgl_context *)0, &r);
    rc |= rtgl_read_robust_adaptive_f32((rtgl_context *)0, px);
    rc |= rtgl_read_robust_adaptive_bucket_f32((rtgl_context *)0, 3u, px);
    rc |= rtgl_read_robust_adaptive_tiles((rtgl_context *)0, tiles, &tx, &ty);
    rc |= rtgl_device_robust_adaptive_tiles((rtgl_context *)0) != (void *)0;
    rc |= rtgl_robust_adaptive_end((rtgl_context *)0);
    return rc + (int)(sizeof p != 32) + (int)(sizeof s != 64) + (int)(sizeof tiles[0] != 32);
}
"""

FACADE_ROBUST_ADAPTIVE = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    bool ok = r.robust_adaptive_begin();
    std::vector<uint8_t> mask = r.robust_adaptive_get_mask();
    ok = r.robust_adaptive_set_mask(mask) && ok;
    ok = r.robust_adaptive_frame() && ok;
    ok = r.robust_adaptive_accumulate() && ok;
    rtgl_adaptive_summary s;
    ok = r.robust_adaptive_update(&s) && ok;
    ok = r.robust_adaptive_resolve() && ok;
    rtgl_robust_resolve_params rp;
    rtgl_robust_defaults(nullptr, &rp);
    rp.dest = RTGL_ROBUST_DEST_IMAGE;
    ok = r.robust_adaptive_resolve(&rp) && ok;
    std::vector<rtgl_adaptive_tile> tiles = r.read_robust_adaptive_tiles();
    std::vector<float> out = r.read_robust_adaptive(), bucket = r.read_robust_adaptive_bucket(1);
    ok = r.robust_adaptive_end() && ok;
    const long frames = r.render_robust_adaptive(0.1f, 64);
    const long more = r.render_robust_adaptive(0.05f, 256, 16, 32, 16, 0.5f, true, &s);
    return ok && frames >= 0 && more >= 0 && s.samples_max >= s.samples_min && tiles.size() == mask.size() && out.size() == bucket.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "robust_adaptive.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_robust_adaptive.cpp"
    src.write_text(FACADE_ROBUST_ADAPTIVE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, os.path.join(ROOT, "tests", "cpp", "facade_robust_adaptive.cpp")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


def test_robust_tiles_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "robust_tiles_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "robust_tiles_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    with open(os.path.join(CSRC, "rt_robust_tiles_plan.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<cmath>", "<cstddef>", "<cstdint>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for name in ("invalid", "default_params", "plane_pixels", "plane_bytes", "bucket_bytes", "count_bytes", "record_bytes", "list_bytes"):
        assert f"rt_robust_tiles_plan::{name}(" in code, name
    # the session's shapes, mask rule, lists and summary are adaptive sampling's, each used in one place that serves both kinds of session
    for name in ("shape", "explicit_mask", "active", "summary", "build_lists"):
        assert f"rt_adaptive_plan::{name}(" in code, name
    for name in ("build_lists", "active", "summary"):
        assert code.count(f"rt_adaptive_plan::{name}(") == 1, name
    # the shared host bodies: defined once, taking the session, and called by the entry points of both kinds and by nothing else
    def callers(helper):
        assert len(re.findall(rf"^static int {helper}\(rtgl_context \*ctx, (?:const )?TileSession &s[,)]", code, re.M)) == 1, helper
        found = []
        for m in re.finditer(rf"\b{helper}\(ctx, ctx->(\w+)[,)]", code):
            found.append((re.findall(r'^(?:extern "C" |static )\S+ \*?(\w+)\(', code[:m.start()], re.M)[-1], m.group(1)))
        return sorted(found)
    assert callers("tile_session_update") == [("rtgl_adaptive_update", "ad"), ("rtgl_robust_adaptive_update", "ra")]
    assert callers("tile_session_set_mask") == [("rtgl_adaptive_set_mask", "ad"), ("rtgl_robust_adaptive_set_mask", "ra")]
    assert callers("tile_session_get_mask") == [("rtgl_adaptive_get_mask", "ad"), ("rtgl_robust_adaptive_get_mask", "ra")]
    assert callers("tile_session_read_tiles") == [("rtgl_read_adaptive_tiles", "ad"), ("rtgl_read_robust_adaptive_tiles", "ra")]
    for helper in ("tile_session_update", "tile_session_set_mask", "tile_session_get_mask", "tile_session_read_tiles"):
        assert len(re.findall(rf"\b{helper}\(", code)) == 3, helper      # (the definition and the two calls)
    # neither kind keeps a mask, lists or shared buffers of its own beside the two sessions
    assert len(re.findall(r"^\s*TileSession (ad|ra);", code, re.M)) == 2 and not re.search(r"\b(ad|ra)_(mask|blocks|tiles|active)\b|\bd_(ad|ra)_(samples|records|counts|lists)\b", code)
    assert len(re.findall(r"\bmasked_frame\(ctx,", code)) == 2 and len(re.findall(r"\blaunch_wavefront\(ctx, sc, frames, im, n0, nullptr, nullptr, list\)", code)) == 1
    with open(os.path.join(CSRC, "rt_robust_tiles.hpp")) as f:
        kernels = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "#pragma clang fp contract(off)" in kernels and "atomicAdd" not in kernels and "atomicCAS" not in kernels and "error_wave_tree(" in kernels
    # every store to global memory goes through store_through
    assert not re.search(r"\ba\.(buckets|out|records|n|m)\s*\[[^\]]*\]\s*=[^=]", kernels) and kernels.count("store_through(") >= 7


@pytest.fixture(scope="module")
def resource_report():
    return report()


# VGPRs and waves per SIMD as the build gives them
FOLD_PIN = (28, 8)
RESOLVE_PINS = {(4, 0): (30, 8), (4, 1): (33, 8), (8, 0): (52, 8), (8, 1): (58, 8), (16, 0): (90, 5), (16, 1): (101, 4)}      # (K, dest) -> (VGPRs, occupancy)
ESTIMATE_PINS = {4: (23, 8), 8: (38, 8), 16: (70, 7)}                                                                       # K -> (VGPRs, occupancy)


def test_the_three_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        if "tile_buckets" not in name:
            continue
        m = re.match(r"_ZN2rt\d+tile_buckets_(fold)_kernelENS_\d+TileBucketsFoldArgsE$", name) \
            or re.match(r"_ZN2rt\d+tile_buckets_(resolve)_kernelILi(\d+)ELi(\d+)EEEvNS_\d+TileBucketsResolveArgsE$", name) \
            or re.match(r"_ZN2rt\d+tile_buckets_(estimate)_kernelILi(\d+)EEEvNS_\d+TileBucketsEstimateArgsE$", name)
        assert m, name                                       # exactly these: nothing else carries the name
        found[(m.group(1),) + tuple(int(g) for g in m.groups()[1:])] = r
    want = [("fold",)] + [("resolve",) + k for k in RESOLVE_PINS] + [("estimate", K) for K in ESTIMATE_PINS]
    assert sorted(found) == sorted(want), sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        # the estimate: the four waves' partial sums and counts; the other two hold none
        assert r["LDS Size"] == (32 if key[0] == "estimate" else 0), f"{key}: {r}"
        pin = FOLD_PIN if key[0] == "fold" else RESOLVE_PINS[key[1:]] if key[0] == "resolve" else ESTIMATE_PINS[key[1]]
        assert (r["VGPRs"], r["Occupancy"]) == pin, f"{key}: {r}"
    assert found[("fold",)]["Occupancy"] >= 8                # the fold streams: the registers must not limit the waves per SIMD (8 is the most the report states)
