"""Resource usage of ray binning's move (rt_wavefront.hpp, sort_place_kernel; rt_scan.hpp, packet_cull_kernel's gather), from the
compiler's own report (no GPU needed: hipcc cross-compiles).  The gather loads and stores every ray of a binned queue inside packet
culling; it must cost that kernel neither a spill nor its five waves per SIMD."""
import re

import pytest

from resource_report import report


@pytest.fixture(scope="module")
def resource_report():
    return report()


def kernel(rep, name):
    found = [r for fn, r in rep.items() if re.match(r"_ZN2rt\d+" + name + r"E", fn)]
    assert len(found) == 1, f"{name}: {len(found)} entries in the report"
    return found[0]


@pytest.mark.parametrize("name", ["packet_cull_kernel", "sort_place_kernel", "sort_scatter_kernel"])
def test_move_kernels_spill_nothing(name, resource_report):
    r = kernel(resource_report, name)
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, f"{name}: {r}"


def test_packet_cull_keeps_five_waves_per_simd(resource_report):
    r = kernel(resource_report, "packet_cull_kernel")
    assert r["VGPRs"] <= 96 and r["Occupancy"] >= 5, r
