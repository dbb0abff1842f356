"""rtgl_robust_denoise (include/rtgl_amd.h, "robust denoise") at the ABI level, without a GPU: the header, the Python binding and the
library agree on the entry points and on the layout; header, binding, facade, library and mirror state the same defaults; the calls reject
a NULL context and invalid records before touching a device; a C99 program compiles against the header and the facade's methods with the
host compilers; the host half (rt_bucket_guide_plan.hpp) passes its stand-alone program under the address and undefined-behaviour
sanitizers; and the six kernels spill nothing, use no scratch and hold 9504 bytes of LDS (compiler resource report)."""
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
ENTRY_POINTS = ["rtgl_robust_denoise_defaults", "rtgl_robust_denoise"]
DEFAULTS_TEXT = r"passes (\d+), sigma_lum ([\d.]+), sigma_normal ([\d.]+),\s+(?:\*\s+|//\s+)?sigma_position ([\d.]+), gain ([\d.]+),\s+(?:\*\s+|//\s+)?demodulate (on|off)"
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
    for decl in (r"\bint\s+rtgl_robust_denoise_defaults\s*\(\s*rtgl_robust_denoise_params\s*\*\s*\w+\s*\)\s*;",
                 r"\bint\s+rtgl_robust_denoise\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*const\s+rtgl_robust_denoise_params\s*\*\s*\w+\s*\)\s*;"):
        assert re.search(decl, text), decl
    H_ = rt.host
    assert set(ENTRY_POINTS) <= set(H_.ABI_SYMBOLS)
    assert text.index("-- robust denoise") > text.index("-- robust error estimate")      # a section behind the robust error estimate
    fields = struct_fields(text, "rtgl_robust_denoise_params")
    assert fields == [("uint32_t", "passes", 1), ("float", "sigma_lum", 1), ("float", "sigma_normal", 1), ("float", "sigma_position", 1), ("float", "gain", 1),
                      ("uint32_t", "flags", 1), ("uint32_t", "reserved", 2)]
    ctype = H_.CRobustDenoiseParams
    assert 4 * sum(k for _, _, k in fields) == 32 == C.sizeof(ctype)
    assert [(n, CTYPE[t] * k if k > 1 else CTYPE[t]) for t, n, k in fields] == list(ctype._fields_)
    offsets, at = [], 0
    for _, _, k in fields:
        offsets.append(at)
        at += 4 * k
    assert [getattr(ctype, n).offset for _, n, _ in fields] == offsets
    # the header states the identity the mirror test holds, and the limit of the guides
    assert "the v of rtgl_robust_error_estimate step 7" in text and "LATEST frame's jittered hit" in text


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_library_and_mirror_state_the_same_defaults(rt):
    import robust_denoise_mirror
    lib = rt.host.load_library()
    p = rt.host.CRobustDenoiseParams(passes=77, sigma_lum=-1, sigma_normal=9, sigma_position=9, gain=-3, flags=6, reserved=(1, 2))
    assert lib.rtgl_robust_denoise_defaults(C.byref(p)) == 0
    assert lib.rtgl_robust_denoise_defaults(None) == ERR_INVALID
    d = rt.host.ROBUST_DENOISE_DEFAULTS
    assert list(p.reserved) == [0, 0] and p.passes == d["passes"] and p.flags == (rt.host.DENOISE_DEMODULATE if d["demodulate"] else 0)
    for name in ("sigma_lum", "sigma_normal", "sigma_position", "gain"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, gain=1.0, demodulate=True)
    assert robust_denoise_mirror.DEFAULTS == d
    assert robust_denoise_mirror.valid_params(d["passes"], d["sigma_lum"], d["sigma_normal"], d["sigma_position"], d["gain"])
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m, path
        g = m.groups()
        assert (int(g[0]), float(g[1]), float(g[2]), float(g[3]), float(g[4]), g[5] == "on") == tuple(d.values()), path


def invalid_blocks(rt):
    lib = rt.host.load_library()

    def block(**kw):
        p = rt.host.CRobustDenoiseParams()
        lib.rtgl_robust_denoise_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    return [block(passes=9), block(passes=0xFFFFFFFF), block(sigma_lum=nan), block(sigma_lum=inf), block(sigma_lum=0.0), block(sigma_lum=-4.0),
            block(sigma_normal=nan), block(sigma_normal=inf), block(sigma_normal=-inf), block(sigma_position=nan), block(sigma_position=inf),
            block(gain=nan), block(gain=inf), block(gain=-inf), block(gain=-1.0), block(gain=-1e-30), block(flags=2), block(flags=3), block(flags=0x80000000),
            block(reserved=(0, 1)), block(reserved=(1, 0))]


def test_calls_reject_a_null_context(rt):
    lib = rt.host.load_library()
    p = rt.host.CRobustDenoiseParams()
    lib.rtgl_robust_denoise_defaults(C.byref(p))
    assert lib.rtgl_robust_denoise(None, None) == ERR_INVALID and lib.rtgl_robust_denoise(None, C.byref(p)) == ERR_INVALID
    for bad in invalid_blocks(rt):
        assert lib.rtgl_robust_denoise(None, C.byref(bad)) == ERR_INVALID


def test_the_mirror_refuses_what_the_library_refuses(rt):
    """the records the device test sends to a live context are the ones the mirror's validation refuses"""
    import robust_denoise_mirror
    for bad in invalid_blocks(rt):
        assert not robust_denoise_mirror.valid_params(bad.passes, bad.sigma_lum, bad.sigma_normal, bad.sigma_position, bad.gain, bad.flags, tuple(bad.reserved))


C_SNIPPET = r"""
#include "rtgl_amd.h"
int main(void)
{
    rtgl_robust_denoise_params p;
    int rc = rtgl_robust_denoise_defaults(&p);
    p.passes = 3u; p.sigma_lum = 2.0f; p.sigma_normal = 0.0f; p.sigma_position = -1.0f; p.gain = 0.5f; p.flags = RTGL_DENOISE_DEMODULATE; p.reserved[1] = 0u;
    rc |= rtgl_robust_denoise((rtgl_context *)0, &p);
    rc |= rtgl_robust_denoise((rtgl_context *)0, (const rtgl_robust_denoise_params *)0);
    return rc + (int)(sizeof p != 32);
}
"""

FACADE_ROBUST_DENOISE = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    bool ok = r.render_robust(16) == 16;
    ok = r.robust_denoise() && ok;
    rtgl_robust_denoise_params p;
    rtgl_robust_denoise_defaults(&p);
    p.gain = 0.0f; p.passes = 2u; p.flags = 0u;
    ok = r.robust_denoise(&p) && ok;
    const std::vector<float> picture = r.read_denoised(), variance = r.read_denoise_variance();
    return ok && picture.size() == variance.size() ? 0 : 1;
}
"""


def test_header_and_facade_compile_with_the_host_compilers(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "robust_denoise.c"
    src.write_text(C_SNIPPET)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    src = tmp_path / "facade_robust_denoise_methods.cpp"
    src.write_text(FACADE_ROBUST_DENOISE)
    for path in (str(src), os.path.join(ROOT, "tests", "cpp", "facade_robust_denoise.cpp")):      # the methods alone, and the device test's driver
        out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", inc, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]


def test_bucket_guide_plan_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bucket_guide_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "bucket_guide_plan_check.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0, done.stdout


def test_plan_header_is_host_only_and_the_library_uses_it():
    with open(os.path.join(CSRC, "rt_bucket_guide_plan.hpp")) as f:
        header = f.read()
    assert set(re.findall(r"#include\s+(\S+)", header)) == {"<cmath>", "<cstddef>", "<cstdint>"}
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for name in ("default_params", "invalid", "refused", "planes_refused", "planes_needed", "demodulates", "tiles_x", "tiles_y", "pixels", "record_bytes",
                 "near_bytes", "scratch_buffers"):
        assert f"rt_bucket_guide_plan::{name}(" in code, name
    with open(os.path.join(CSRC, "rt_bucket_guide.hpp")) as f:
        kernels = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "#pragma clang fp contract(off)" in kernels and "atomic" not in kernels and "store_through(" in kernels
    stores = re.findall(r"^\s*(?:a\.\w+\[[^\]]*\]|\*\s*a\.\w+)\s*=", kernels, re.M)
    assert not stores, stores                                        # every global store goes through store_through
    # the passes are the existing ones, launched by the one function that launches them for rtgl_denoise_guided
    def body_of(entry):
        body = code[code.index(f'extern "C" int {entry}('):]
        return body[:body.index("\n}\n")]
    body = body_of("rtgl_robust_denoise")
    assert body.count("launch_guided_passes(") == 1 and body_of("rtgl_denoise_guided").count("launch_guided_passes(") == 1
    assert code.count("launch_guided_passes(") == 3 and code.count("launch_guided<") == 3      # (the definition and the two calls; the three forms of a pass)
    passes = code[code.index("static int launch_guided_passes("):]
    assert passes[:passes.index("\n}\n")].count("launch_guided<") == 3
    assert "launch_guided<" not in body and "guided_prepare_kernel" not in body and "buf_ensure(" in body and "hipMalloc" not in body


@pytest.fixture(scope="module")
def resource_report():
    return report()


# VGPRs and waves per SIMD as the build gives them: (K, demodulating) -> (VGPRs, occupancy)
BUCKET_GUIDE_PINS = {(4, 1): (44, 8), (4, 0): (44, 8), (8, 1): (60, 8), (8, 0): (68, 7), (16, 1): (114, 4), (16, 0): (118, 4)}
LDS_BYTES = 6 * 66 * 6 * 4


def test_bucket_guide_kernels_spill_nothing_and_hold_the_designed_lds(resource_report):
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt\d+bucket_guide_kernelILi(\d+)ELb([01])EEEvNS_\d+BucketGuideArgsE$", name)
        if m:
            found[(int(m.group(1)), int(m.group(2)))] = r
        else:
            assert "bucket_guide" not in name, name                # exactly these: nothing else carries the name
    assert sorted(found) == sorted(BUCKET_GUIDE_PINS), sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        assert r["LDS Size"] == LDS_BYTES == 9504, f"{key}: {r}"   # normal.xyz and position.xyz of the 66 x 6 pixels about the tile
        assert (r["VGPRs"], r["Occupancy"]) == BUCKET_GUIDE_PINS[key], f"{key}: {r}"
