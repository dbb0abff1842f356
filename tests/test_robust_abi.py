"""Robust accumulation (rtgl_robust_*, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and the library
agree on the entry points and on the two layouts; header, binding, facade, library and mirror state the same defaults; the calls reject a
NULL context and invalid arguments before touching a device; a C99 program compiles against the header and the facade's methods with the
host compilers; the host half (rt_robust_plan.hpp) passes its stand-alone program under the address and undefined-behaviour sanitizers;
and the seven kernels spill nothing, use no scratch and no LDS (compiler resource report)."""
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
ENTRY_POINTS = ["rtgl_robust_defaults", "rtgl_robust_begin", "rtgl_robust_accumulate", "rtgl_robust_resolve", "rtgl_robust_end", "rtgl_robust_frames",
                "rtgl_read_robust_f32", "rtgl_read_robust_bucket_f32"]
DEFAULTS_TEXT = (r"buckets (\d+), flags (\d+)", r"gain ([\d.]+), dest (\d+), flags (\d+)")
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


def test_header_declares_the_entry_points_and_the_two_layouts(rt):
    text = header_text()
    ctx = r"rtgl_context\s*\*\s*\w+"
    for decl in (r"\bint\s+rtgl_robust_defaults\s*\(\s*rtgl_robust_params\s*\*\s*\w+\s*,\s*rtgl_robust_resolve_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_begin\s*\(\s*{ctx}\s*,\s*const\s+rtgl_robust_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_accumulate\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_resolve\s*\(\s*{ctx}\s*,\s*const\s+rtgl_robust_resolve_params\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_end\s*\(\s*{ctx}\s*\)\s*;",
                 rf"\bint\s+rtgl_robust_frames\s*\(\s*{ctx}\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_f32\s*\(\s*{ctx}\s*,\s*float\s*\*\s*\w+\s*\)\s*;",
                 rf"\bint\s+rtgl_read_robust_bucket_f32\s*\(\s*{ctx}\s*,\s*uint32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;"):
        assert re.search(decl, text), decl
    assert re.search(r"enum\s*\{\s*RTGL_ROBUST_DEST_BUFFER\s*=\s*0\s*,\s*RTGL_ROBUST_DEST_IMAGE\s*=\s*1\s*\}\s*;", text)
    H_ = rt.host
    assert set(ENTRY_POINTS) <= set(H_.ABI_SYMBOLS)
    assert (H_.ROBUST_DEST_BUFFER, H_.ROBUST_DEST_IMAGE) == (0, 1)
    params = struct_fields(text, "rtgl_robust_params")
    assert params == [("uint32_t", "buckets", 1), ("uint32_t", "flags", 1), ("uint32_t", "reserved", 6)]
    resolve = struct_fields(text, "rtgl_robust_resolve_params")
    assert resolve == [("float", "gain", 1), ("uint32_t", "dest", 1), ("uint32_t", "flags", 1), ("uint32_t", "reserved", 5)]
    for fields, ctype in ((params, H_.CRobustParams), (resolve, H_.CRobustResolveParams)):
        assert sum(SIZE[t] * k for t, _, k in fields) == 32 == C.sizeof(ctype)
        assert [(n, CTYPE[t] * k if k > 1 else CTYPE[t]) for t, n, k in fields] == list(ctype._fields_)
        offsets, at = [], 0
        for t, _, k in fields:
            offsets.append(at)
            at += SIZE[t] * k
        assert [getattr(ctype, n).offset for _, n, _ in fields] == offsets


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import robust_mirror
    lib = rt.host.load_library()
    p = rt.host.CRobustParams(buckets=3, flags=6, reserved=(1, 2, 3, 4, 5, 6))
    r = rt.host.CRobustResolveParams(gain=-1, dest=7, flags=9, reserved=(1, 2, 3, 4, 5))
    assert lib.rtgl_robust_defaults(C.byref(p), C.byref(r)) == 0
    assert lib.rtgl_robust_defaults(None, None) == ERR_INVALID
    d = rt.host.ROBUST_DEFAULTS
    assert (p.buckets, p.flags, list(p.reserved)) == (d["buckets"], 0, [0] * 6)
    assert (np.float32(r.gain), r.dest, r.flags, list(r.reserved)) == (np.float32(d["gain"]), d["dest"], 0, [0] * 5)
    p2, r2 = rt.host.CRobustParams(buckets=3), rt.host.CRobustResolveParams(gain=-1)      # either alone
    assert lib.rtgl_robust_defaults(C.byref(p2), None) == 0 and lib.rtgl_robust_defaults(None, C.byref(r2)) == 0
    assert bytes(p2) == bytes(p) and bytes(r2) == bytes(r)
    assert d == dict(buckets=8, gain=1.0, dest=0)
    assert robust_mirror.DEFAULTS == d and robust_mirror.BUCKETS == (4, 8, 16)
    for path in (HEADER, FACADE):
        with open(path) as f:
            text = f.read()
        begin, resolve = (re.search(t, text) for t in DEFAULTS_TEXT)
        assert begin and resolve, path
        assert (int(begin.group(1)), int(begin.group(2))) == (d["buckets"], 0), path
        assert (float(resolve.group(1)), int(resolve.group(2)), int(resolve.group(3))) == (d["gain"], d["dest"], 0), path


def invalid_records(rt):
    lib = rt.host.load_library()

    def begin(**kw):
        p = rt.host.CRobustParams()
        lib.rtgl_robust_defaults(C.byref(p), None)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def resolve(**kw):
        p = rt.host.CRobustResolveParams()
        lib.rtgl_robust_defaults(None, C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return ([begin(buckets=k) for k in (0, 1, 2, 3, 5, 7, 9, 12, 15, 17, 32, 0xFFFFFFFF)] + [begin(flags=1), begin(flags=0x80000000), begin(reserved=(0, 0, 0, 0, 0, 1)),
                                                                                            begin(reserved=(1, 0, 0, 0, 0, 0))],
            [resolve(gain=nan), resolve(gain=inf), resolve(gain=-inf), resolve(gain=-1.0), resolve(gain=-1e-30), resolve(dest=2), resolve(dest=0xFFFFFFFF),
             resolve(flags=1), resolve(reserved=(0, 0, 0, 0, 1)), resolve(reserved=(1, 0, 0, 0, 0))])


def test_calls_reject_a_null_context_and_null_arguments(rt):
    lib = rt.host.load_library()
    p, r = rt.host.CRobustParams(), rt.host.CRobustResolveParams()
    lib.rtgl_robust_defaults(C.byref(p), C.byref(r))
    begins, resolves = invalid_records(rt)
    assert lib.rtgl_robust_begin(None, None) == ERR_INVALID and lib.rtgl_robust_begin(None, C.byref(p)) == ERR_INVALID
    for bad in begins:
        assert lib.rtgl_robust_begin(None, C.byref(bad)) == ERR_INVALID
    assert lib.rtgl_robust_resolve(None, None) == ERR_INVALID and lib.rtgl_robust_resolve(None, C.byref(r)) == ERR_INVALID
    for bad in resolves:
        assert lib.rtgl_robust_resolve(None, C.byref(bad)) == ERR_INVALID
    n, k, px = C.c_uint32(), C.c_uint32(), (C.c_float * 4)()
    assert lib.rtgl_robust_accumulate(None) == ERR_INVALID and lib.rtgl_robust_end(None) == ERR_INVALID
    assert lib.rtgl_robust_frames(None, C.byref(n), C.byref(k)) == ERR_INVALID and lib.rtgl_robust_frames(None, None, None) == ERR_INVALID
    assert lib.rtgl_read_robust_f32(None, px) == ERR_INVALID and lib.rtgl_read_robust_f32(None, None) == ERR_INVALID
    assert lib.rtgl_read_robust_bucket_f32(None, 0, px) == ERR_INVALID and lib.rtgl_read_robust_bucket_f32(None, 99, None) == ERR_INVALID


def test_the_mirror_refuses_what_the_library_refuses(rt):
    """the records the device tests send to a live context (tests/test_gpu_robust.py) are the ones the mirror's validation refuses"""
    import robust_mirror
    begins, resolves = invalid_records(rt)
    for bad in begins:
        assert not robust_mirror.valid_params(bad.buckets, bad.flags, tuple(bad.reserved))
    for bad in resolves:
        assert not robust_mirror.valid_resolve_params(bad.gain, bad.dest, bad.flags, tuple(bad.reserved))


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_robust_params p;
    rtgl_robust_resolve_params r;
    float px[4];
    uint32_t frames, buckets;
    int rc = rtgl_robust_defaults(&p, &r);
    p.buckets = 16u; p.flags = 0u; p.reserved[5] = 0u;
    r.gain = 0.5f; r.dest = RTGL_ROBUST_DEST_IMAGE; r.flags = 0u; r.reserved[4] = 0u;
    rc |= rtgl_robust_begin((rtgl_context *)0, &p);
    rc |= rtgl_robust_accumulate((rtgl_context *)0);
    rc |= rtgl_robust_resolve((rtgl_context *)0, &r);
    rc |= rtgl_robust_frames((rtgl_context *)0, &frames, &buckets);
    rc |= rtgl_read_robust_f32((rtgl_context *)0, px);
    rc |= rtgl_read_robust_bucket_f32((rtgl_context *)0, 3u, px);
    rc |= rtgl_robust_end((rtgl_context *)0);
    return rc + (int)(sizeof p != 32) + (int)(sizeof r != 32) + (int)(RTGL_ROBUST_DEST_BUFFER != 0);
}
"""

FACADE_ROBUST = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    bool ok = r.robust_begin();
    ok = r.robust_frame() && ok;
    ok = r.robust_accumulate() && ok;
    ok = r.robust_resolve() && ok;
    rtgl_robust_resolve_params rp;
    rtgl_robust_defaults(nullptr, &rp);
    rp.dest = RTGL_ROBUST_DEST_IMAGE;
    ok = r.robust_resolve(&rp) && ok;
    const long n = r.robust_frames();
    std::vector<float> out = r.read_robust(), bucket = r.read_robust_bucket(1);
    ok = r.robust_end() && ok;
    const long frames = r.render_robust(32);
    const long more = r.render_robust(64, 16, 0.5f, true);
    return ok && n >= 0 && frames >= 0 && more >= 0 && out.size() == bucket.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "robust.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_robust.cpp"
    src.write_text(FACADE_ROBUST)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


def test_robust_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "robust_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "robust_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    with open(os.path.join(CSRC, "rt_robust_plan.hpp")) as f:
        header = f.read()
    assert set(re.findall(r"#include\s+(\S+)", header)) - {"<cmath>"} == {"<cstddef>", "<cstdint>"}
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for name in ("invalid", "next_bucket", "next_count", "plane_pixels", "bucket_bytes", "output_bytes", "default_params", "default_resolve_params"):
        assert f"rt_robust_plan::{name}(" in code, name
    with open(os.path.join(CSRC, "rt_robust.hpp")) as f:
        kernels = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "#pragma clang fp contract(off)" in kernels and "__shared__" not in kernels and "atomic" not in kernels


@pytest.fixture(scope="module")
def resource_report():
    return report()


# VGPRs and waves per SIMD as the build gives them: (K, dest) -> (VGPRs, occupancy)
RESOLVE_PINS = {(4, 0): (30, 8), (4, 1): (34, 8), (8, 0): (52, 8), (8, 1): (58, 8), (16, 0): (92, 5), (16, 1): (101, 4)}
FOLD_PIN = (27, 8)


def test_robust_kernels_spill_nothing_and_hold_no_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        if "robust" not in name:
            continue
        m = re.match(r"_ZN2rt\d+robust_accumulate_kernelE", name)
        if m:
            found["fold"] = r
            continue
        m = re.match(r"_ZN2rt\d+robust_resolve_kernelILi(\d+)ELi(\d+)EEE", name)
        assert m, name                                       # exactly these: nothing else carries the name
        found[(int(m.group(1)), int(m.group(2)))] = r
    assert sorted(found, key=str) == sorted(list(RESOLVE_PINS) + ["fold"], key=str), sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, f"{key}: {r}"
        assert (r["VGPRs"], r["Occupancy"]) == (FOLD_PIN if key == "fold" else RESOLVE_PINS[key]), f"{key}: {r}"
    assert found["fold"]["Occupancy"] >= 8                   # the fold streams: the registers must not limit the waves per SIMD (8 is the most the report states)
