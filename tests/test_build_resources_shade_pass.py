"""Resource usage of the one-pass shade launch (rt_wavefront.hpp: shade_kernel), from the compiler's own report (no GPU needed: hipcc
cross-compiles).  The point of the one-pass form is what the grid-stride loop cost the same body: 99 VGPRs, 32 spilled scalar registers
and 4 waves per SIMD.  Without the loop every instance must spill nothing, use no scratch, reach at least 7 waves per SIMD and stay within
the 16,404 B of LDS of the binning instances (four waves' staging records + five counters), so that nine blocks fit a CU.  The camera
form keeps its 8 waves.  The stride form (shade_stride_kernel) is printed, not pinned: it is the parent's kernel, kept for short queues."""
import re

import pytest

from resource_report import report


@pytest.fixture(scope="module")
def resource_report():
    return report()


def kernels(rep, pattern):
    return {fn: r for fn, r in rep.items() if re.match(pattern, fn)}


def test_one_pass_instances_spill_nothing_and_reach_seven_waves(resource_report):
    found = kernels(resource_report, r"_ZN2rt\d+shade_kernelILb[01]ELb[01]ELb[01]EEEv")
    assert len(found) == 8, sorted(found)
    for fn, r in sorted(found.items()):
        print(fn, r)
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{fn}: {r}"
        assert r["Occupancy"] >= 7, f"{fn}: {r}"
        assert r["LDS Size"] <= 16404, f"{fn}: {r}"


def test_camera_instances_keep_eight_waves(resource_report):
    found = kernels(resource_report, r"_ZN2rt\d+shade_camera_kernelILb[01]ELb[01]EEEv")
    assert len(found) == 4, sorted(found)
    for fn, r in sorted(found.items()):
        print(fn, r)
        assert r["Occupancy"] >= 8, f"{fn}: {r}"


def test_stride_instances_are_reported(resource_report):
    """figures only: the loop form is what the parent ran"""
    found = kernels(resource_report, r"_ZN2rt\d+shade_stride_kernelILb[01]ELb[01]ELb[01]EEEv")
    assert len(found) == 8, sorted(found)
    for fn, r in sorted(found.items()):
        print(fn, {k: r.get(k) for k in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")})
