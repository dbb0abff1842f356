"""First-hit planes (option "aov": albedo, normal, position, hit ids) at the ABI level, without a GPU: the header, the Python binding and
the library agree on the new entry points, both reject a NULL context before touching a device, the C++ facade's accessors compile with
the host compiler, and the kernel instances that write the planes spill nothing (compiler resource report; hipcc cross-compiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from resource_report import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtgl_amd.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_aov_entry_points_and_constants(rt):
    text = header_text()
    assert re.search(r"\bint\s+rtgl_read_aov\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bvoid\s*\*\s*rtgl_device_aov\s*\(\s*rtgl_context\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bRTGL_AOV_([A-Z]+)\s*=\s*(\d+)", text)}
    assert consts == {"ALBEDO": rt.host.AOV_ALBEDO, "NORMAL": rt.host.AOV_NORMAL, "POSITION": rt.host.AOV_POSITION, "IDS": rt.host.AOV_IDS,
                      "ALL": rt.host.AOV_ALL}
    assert (consts["ALBEDO"], consts["NORMAL"], consts["POSITION"], consts["IDS"]) == (1, 2, 4, 8)
    assert {"rtgl_read_aov", "rtgl_device_aov"} <= set(rt.host.ABI_SYMBOLS)


def test_library_exports_the_aov_entry_points(rt):
    rt.host.build_library()
    lib = rt.host.load_library()
    assert hasattr(lib, "rtgl_read_aov") and hasattr(lib, "rtgl_device_aov")


def test_aov_calls_reject_a_null_context(rt):
    lib = rt.host.load_library()
    buf = np.zeros(64, np.float32)
    for plane in (rt.host.AOV_ALBEDO, rt.host.AOV_IDS, 3, 0):
        assert lib.rtgl_read_aov(None, plane, buf.ctypes.data_as(C.c_void_p)) == -1       # RTGL_ERR_INVALID
        assert lib.rtgl_device_aov(None, plane) is None


FACADE_AOV = r"""
#include "rtgl/renderer.h"
int main()
{
    Renderer r(64, 48);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION | RTGL_AOV_IDS);
    r.set_frame_budget(1);
    r.run();
    const std::vector<float> albedo = r.read_aov(RTGL_AOV_ALBEDO);
    const std::vector<int32_t> ids = r.read_aov<int32_t>(RTGL_AOV_IDS);
    const bool ok = r.save_aov_pfm(RTGL_AOV_NORMAL, "normal.pfm") && r.save_pfm("beauty.pfm");
    r.set_aov(0);
    return ok && albedo.size() == ids.size() ? 0 : 1;
}
"""


def test_facade_aov_accessors_compile_with_the_host_compiler(tmp_path):
    src = tmp_path / "facade_aov.cpp"
    src.write_text(FACADE_AOV)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def resource_report():
    return report()


# the instances that write the planes: the last template argument (kAov) is true
AOV_INSTANCE = {
    "pathtrace_mega_kernel": r"_Z21pathtrace_mega_kernelILb[01]ELb1EEv",
    "bounce_kernel": r"_ZN2rt13bounce_kernelILi[124]ELi[01]ELb[01]ELb1EEEv",
    "shade_kernel": r"_ZN2rt12shade_kernelILb[01]ELb[01]ELb1EEEv",
}


@pytest.mark.parametrize("kernel,count", [("pathtrace_mega_kernel", 2), ("bounce_kernel", 12), ("shade_kernel", 4)])
def test_aov_kernel_instances_spill_nothing(kernel, count, resource_report):
    found = {name: r for name, r in resource_report.items() if re.match(AOV_INSTANCE[kernel], name)}
    assert len(found) == count, f"{kernel}: {sorted(found)}"
    for name, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{name}: {r}"
