"""The plan of ray binning (raytracer.glsl_amd/csrc/rt_bin_plan.hpp), without a GPU.
  * tests/cpp/bin_plan_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: every (RTGL_AMD_SORT_OB, RTGL_AMD_SORT_DB) pair of 0..7 x 0..8, the refused ones included; for every accepted plan the bits
    per axis, the shifts, the grids, the counters, and the keys of an adversarial and a random ray set.
  * the check is sharp: built against a copy of the header with the accepted range widened back to what the variables used to take, with
    the cap of 10 bits per axis removed, the cell word left unshifted, the direction bits shifted by T instead of T + 1, or
    RTGL_AMD_BIN_SPLIT=0 ignored, the program fails (the last two cannot show on the device: any key renders the same image).
  * rtgl_amd.hip and rt_wavefront.hpp call the header and keep no copy."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "cpp", "bin_plan_check.cpp")


def build_and_run(tmp_path, include_dir, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", include_dir, CHECK, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_bin_plan_program_under_sanitizers(tmp_path):
    done = build_and_run(tmp_path, CSRC, "bin_plan_check")
    assert done.returncode == 0, done.stdout
    assert "runtime error" not in done.stdout and "Sanitizer" not in done.stdout, done.stdout      # UBSan reports and goes on
    assert "ok: 19 accepted pairs, 0 failures" in done.stdout, done.stdout


MUTANTS = {
    # the ranges of the parent: ob 1..5 and db 2..6, whatever they add up to
    "parent_ranges": ("return bits >= 12 && 2 * db <= 16 && T >= 0 && T <= (int)kOrderSlots;", "return bits > 0 || T > 0 || true;"),
    "no_axis_cap": ("if (bits[best] >= kAxisCap) for (int a = 0; a < 3; ++a) if (bits[a] < bits[best]) best = a;", ""),
    "cell_unshifted": ("| (cell << (T - n));", "| cell;"),
    "direction_shift": ("return (dir << (T + 1u)) |", "return (dir << T) |"),
    "bin_split_ignored": ("if (!bin_split) for", "if (false && !bin_split) for"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_bin_plan_check_fails_on_a_mutated_header(name, tmp_path):
    old, new = MUTANTS[name]
    with open(os.path.join(CSRC, "rt_bin_plan.hpp")) as f:
        header = f.read()
    assert header.count(old) == 1, f"the text of mutant {name} is not in the header (once)"
    with open(tmp_path / "rt_bin_plan.hpp", "w") as f:
        f.write(header.replace(old, new))
    done = build_and_run(tmp_path, str(tmp_path), "bin_plan_check_" + name)
    assert done.returncode != 0 and "FAIL" in done.stdout, f"mutant {name} passed the check:\n{done.stdout}"


def test_header_is_host_only_and_the_library_keeps_no_copy():
    with open(os.path.join(CSRC, "rt_bin_plan.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<cmath>", "<cstddef>", "<cstdint>", "<cstring>"]
    code = {}
    for name in ("rtgl_amd.hip", "rt_wavefront.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            code[name] = "".join(re.sub(r"//.*", "", line) for line in f)
    both = code["rtgl_amd.hip"] + code["rt_wavefront.hpp"]
    for call in ("rt_bin_plan::plan(", "rt_bin_plan::cells(", "rt_bin_plan::hist_words(", "rt_bin_plan::sums_grid("):
        assert call in code["rtgl_amd.hip"], call
    assert "rt_bin_plan::ray_bin_key(" in code["rt_wavefront.hpp"]
    assert not re.search(r"\b(spread2|ray_bin_key)\s*\([^)]*\)\s*\{", both)                      # no second definition
    assert not re.search(r"8u?\s*\+\s*3u?\s*\*", both) and not re.search(r"1u?\s*-\s*2u?\s*\*", both)      # sort_bits and sort_T written out
    assert not re.search(r"bins\s*/\s*kSortSeg", both)                                         # the grids and the counter words
    assert not re.search(r"\bsort_(lo|inv_cell|in_lo|in_hi|cen|inv_unit|in_bits|out_bits|in_order|out_order|db|T)\b", both)      # the fields live in rt_bin_plan::Cells
    assert re.search(r"kSortSeg\s*=\s*rt_bin_plan::kSortSeg", code["rt_wavefront.hpp"])
    # the two variables are read in one place, through the header's rule
    assert len(re.findall(r'getenv\("RTGL_AMD_SORT_(?:OB|DB)"\)', code["rtgl_amd.hip"])) == 2
