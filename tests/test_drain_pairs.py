"""The pair expansion of the scan's tail drain (raytracer.glsl_amd/csrc/rt_drain_pairs.hpp), without a GPU.
  * tests/cpp/drain_pairs_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: a model of drain_region's turn over one wave -- window, ballots, list, the four reads per lane -- for regions of 0 .. 1,300
    records with full, single-bit, random and straddling masks: every set bit tested exactly once and in order, no index beyond the
    wave's queue, ceil(pairs / 256) turns, and the model is sharp (a record that forgets its carry is caught).
  * rt_drain_pairs.hpp is host-only, rt_scan.hpp calls it and keeps no copy of its arithmetic.
  * the queue the model allocates is the kernel's (SoloCfg::kQueue), and the record form stays behind its macro, with a Makefile target."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
GXX = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined"]


def stripped(path):
    with open(path) as f:
        return "".join(re.sub(r"//.*", "", line) for line in f)


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("drain_pairs") / "drain_pairs_check")
    subprocess.check_call(GXX + [os.path.join(ROOT, "tests", "cpp", "drain_pairs_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    return p.returncode, p.stdout


def test_drain_pairs_program_under_sanitizers(check_run):
    code, text = check_run
    assert code == 0, text
    assert "runtime error" not in text and "Sanitizer" not in text, text
    m = re.search(r"^ok: (\d+) regions, (\d+) turns, mutant caught on (\d+) of (\d+) shapes, 0 failures$", text, re.M)
    assert m, text
    regions, turns, caught, shapes = (int(x) for x in m.groups())
    assert regions >= 5 * 1301 and turns > regions and caught == shapes > 0, text


def test_header_is_host_only_and_the_kernel_keeps_no_copy():
    with open(os.path.join(CSRC, "rt_drain_pairs.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<algorithm>", "<cstdint>"]
    assert "getenv" not in header
    code = stripped(os.path.join(CSRC, "rt_scan.hpp"))
    assert '#include "rt_drain_pairs.hpp"' in code
    begin = code.index("#ifdef RT_DRAIN_RECORDS")
    middle = code.index("#else", begin)
    end = code.index("#endif", middle)
    pairs = code[middle:end]
    for call in ("load_record(", "record_in_region(", "window_behind(", "bits_from_ballots(", "first_pair(", "pair_fits(", "list_entry(", "fill_behind(",
                 "turn_full(", "lane_has_pair(", "lane_entry("):
        assert "dp::" + call in pairs, call
    # no list arithmetic written out beside the header's: no literal turn length, no fill + ..., no index built from the lane
    assert not re.search(r"\b256u?\b|\b64u\b", pairs)
    assert not re.search(r"fill\s*\+|\+\s*fill", pairs)
    assert not re.search(r"list\[(?!dp::)", pairs)
    # the list is the wave's own queue and its scratch entry; the kernel checks that it fits
    assert re.search(r"static_assert\(rt_drain_pairs::kTurnPairs < Cfg::kQueue", code)
    assert re.search(r"drain_region\(sc, mf, qin, best, reinterpret_cast<const unsigned long long \*>\(cand\), n_rec, \(uint32_t\)lane, queue, Cfg::kQueue - 1u\)", code)
    # one drain per library: the record form only under its macro, which nothing but the Makefile's `records` target defines
    assert code.count("void drain_region(") == 2 and code.index("void drain_region(") > begin and code.rindex("void drain_region(") < end
    assert len(re.findall(r"RT_DRAIN_RECORDS", code)) == 1


def test_the_models_queue_is_the_kernels():
    code = stripped(os.path.join(CSRC, "rt_scan.hpp"))
    step = re.search(r"kStepMax = (\d+)u \* (\d+)u;", code)
    drain = re.search(r"kDrain = (\d+)u;", code)
    assert step and drain and re.search(r"kQueue = kStepMax \+ kDrain \+ 1u;", code)
    k_queue = int(step.group(1)) * int(step.group(2)) + int(drain.group(1)) + 1
    with open(os.path.join(ROOT, "tests", "cpp", "drain_pairs_check.cpp")) as f:
        model = f.read()
    m = re.search(r"constexpr uint32_t kQueue = (\d+)u \* (\d+)u \+ (\d+)u \+ 1u;", model)
    assert m and int(m.group(1)) * int(m.group(2)) + int(m.group(3)) + 1 == k_queue == 321


def test_records_target_builds_the_off_arm_only():
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^records: \$\(SRCS\)\n\t\$\(HIPCC\) \$\(FLAGS\) -DRT_DRAIN_RECORDS -shared -o \$\(HERE\)\.\./librtgl_amd_records\.so", mk, re.M)
    assert mk.count("RT_DRAIN_RECORDS") == 2                     # the comment and the target
    assert "RT_DRAIN_RECORDS" not in mk[mk.index("$(OUT): $(SRCS)"):mk.index("asm:")]
    for name in ("rtgl_amd.hip", "rt_scan_launch.hpp"):
        assert "RT_DRAIN" not in stripped(os.path.join(CSRC, name))
