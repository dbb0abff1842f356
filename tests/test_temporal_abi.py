"""Temporal accumulation (rtgl_temporal_accumulate, include/rtgl_amd.h) at the ABI level, without a GPU: the header, the Python binding and
the library agree on the entry points and on the parameter block; header, binding, facade and mirror state the same defaults; the calls
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
ENTRY_POINTS = ["rtgl_temporal_defaults", "rtgl_temporal_accumulate", "rtgl_temporal_reset", "rtgl_read_temporal_f32", "rtgl_device_temporal"]
DEFAULTS_TEXT = r"max_history (\d+), sigma_normal 0\.3, sigma_position 0\.05"
ERR_INVALID = -1


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_parameter_block(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_temporal_defaults\s*\(\s*rtgl_temporal_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_temporal_accumulate\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*const\s+rtgl_temporal_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_temporal_reset\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+rtgl_read_temporal_f32\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bvoid\s*\*\s*rtgl_device_temporal\s*\(\s*rtgl_context\s*\*\s*\w+\s*\)\s*;", text)
    assert '"denoise_source"' in text
    assert set(ENTRY_POINTS) <= set(rt.host.ABI_SYMBOLS)
    # the block: the header's fields in the binding's order, 32 bytes
    body = re.search(r"typedef\s+struct\s+rtgl_temporal_params\s*\{(.*?)\}\s*rtgl_temporal_params\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("float", "max_history", 1), ("float", "sigma_normal", 1), ("float", "sigma_position", 1), ("uint32_t", "flags", 1),
                      ("uint32_t", "reserved", 4)]
    assert 4 * sum(k for _, _, k in fields) == 32
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in fields] == list(rt.host.CTemporalParams._fields_)
    assert C.sizeof(rt.host.CTemporalParams) == 32
    assert [getattr(rt.host.CTemporalParams, n).offset for _, n, _ in fields] == [0, 4, 8, 12, 16]


def test_library_exports_the_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_binding_facade_and_mirror_state_the_same_defaults(rt):
    import temporal_mirror
    lib = rt.host.load_library()
    p = rt.host.CTemporalParams(max_history=-7, sigma_normal=-1, sigma_position=9, flags=7, reserved=(1, 2, 3, 4))
    assert lib.rtgl_temporal_defaults(C.byref(p)) == 0
    assert lib.rtgl_temporal_defaults(None) == ERR_INVALID
    d = rt.host.TEMPORAL_DEFAULTS
    assert (p.flags, list(p.reserved)) == (0, [0, 0, 0, 0])
    for name in ("max_history", "sigma_normal", "sigma_position"):
        assert np.float32(getattr(p, name)) == np.float32(d[name]), name
    assert d == dict(max_history=32.0, sigma_normal=0.3, sigma_position=0.05)
    assert temporal_mirror.DEFAULTS == d
    for path in (HEADER, FACADE):
        with open(path) as f:
            m = re.search(DEFAULTS_TEXT, f.read())
        assert m and float(m.group(1)) == d["max_history"], path


def test_calls_reject_a_null_context(rt):
    """a NULL context is refused before a single field of the record is read: the rules themselves are checked by tests/test_post_plans.py"""
    lib = rt.host.load_library()
    buf = np.zeros(64, np.float32)
    p = rt.host.CTemporalParams()
    lib.rtgl_temporal_defaults(C.byref(p))
    assert lib.rtgl_temporal_accumulate(None, None) == ERR_INVALID
    assert lib.rtgl_temporal_accumulate(None, C.byref(p)) == ERR_INVALID
    assert lib.rtgl_temporal_reset(None) == ERR_INVALID
    assert lib.rtgl_read_temporal_f32(None, buf.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    assert lib.rtgl_device_temporal(None) is None


FACADE_TEMPORAL = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    r.set_frame_budget(2);
    r.run();
    bool ok = r.temporal_accumulate();
    rtgl_temporal_params p;
    rtgl_temporal_defaults(&p);
    p.max_history = 8.0f; p.sigma_normal = 0.0f;
    ok = r.temporal_accumulate(&p) && ok;
    const std::vector<float> hist = r.read_temporal();
    ok = r.temporal_reset() && ok;
    return ok && hist.size() == (size_t)64 * 48 * 4 ? 0 : 1;
}
"""


def test_facade_methods_compile_with_the_host_compiler(tmp_path):
    src = tmp_path / "facade_temporal.cpp"
    src.write_text(FACADE_TEMPORAL)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


def test_temporal_kernel_instances_spill_nothing(resource_report):
    """temporal_kernel<history, static shortcut, normal test, position test, moments mode>, the mode-0 instances (option "temporal_moments"
    off; modes 1 and 2: tests/test_temporal_moments_abi.py): the instance without history and all eight with it"""
    found = {}
    for name, r in resource_report.items():
        m = re.match(r"_ZN2rt15temporal_kernelILb([01])ELb([01])ELb([01])ELb([01])ELi0EEEv", name)
        if m:
            found[tuple(int(g) for g in m.groups())] = r
    assert sorted(found) == [(0, 0, 0, 0)] + [(1, s, n, p) for s in (0, 1) for n in (0, 1) for p in (0, 1)], sorted(resource_report)
    for key, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{key}: {r}"
        assert r["LDS Size"] == 0, f"{key}: {r}"
        # nothing but memory latency to hide: a gather kernel wants every wave slot the SIMD has
        assert r["Occupancy"] >= 8, f"{key}: {r}"
