"""Resource usage of the lean camera bounce's shade launch (rt_wavefront.hpp: shade_camera_kernel), from the compiler's own
report (no GPU needed: hipcc cross-compiles).  The camera form of shade computes a camera ray where shade_kernel loads one; that must
cost it neither a spill nor a wave per SIMD against the instance of shade_kernel it stands in for, in the same build."""
import re

import pytest

from resource_report import report


@pytest.fixture(scope="module")
def resource_report():
    return report()


def kernels(rep, pattern):
    return {fn: r for fn, r in rep.items() if re.match(pattern, fn)}


def test_camera_kernels_spill_nothing(resource_report):
    found = kernels(resource_report, r"_ZN2rt\d+shade_camera_kernelILb[01]ELb[01]EEEv")
    assert len(found) == 4, sorted(found)
    for fn, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{fn}: {r}"


def test_camera_shade_keeps_the_waves_of_the_kernel_it_replaces(resource_report):
    """<counters off, binning on>: the instance a C2 frame runs"""
    cam = kernels(resource_report, r"_ZN2rt\d+shade_camera_kernelILb0ELb1EEEv")
    ref = kernels(resource_report, r"_ZN2rt\d+shade_kernelILb0ELb1ELb0EEEv")
    assert len(cam) == 1 and len(ref) == 1, (sorted(cam), sorted(ref))
    (c,), (r,) = cam.values(), ref.values()
    print("shade_camera_kernel<false, true>", c, "shade_kernel<false, true, false>", r)
    assert c["Occupancy"] >= r["Occupancy"], f"camera form {c}, shade_kernel {r}"
