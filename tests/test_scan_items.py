"""The item schedule of the kernel-4 scan (raytracer.glsl_amd/csrc/rt_scan_items.hpp), without a GPU.
  * tests/cpp/scan_items_check.cpp, built by the host compiler with the address and undefined-behaviour sanitizers and run as a child
    process: the partition of a chunk's granules into turns and tail, the ranks of a chunk's blocks, and a model of the wave loop of
    scan_solo_kernel under seeded and adversarial interleavings -- every item once, a record or rays read ahead only used in the numbering
    they were read in.
  * the model is sharp: built with -DSCAN_ITEMS_PARENT_RULE (records and ray_k survive the switch from turns to tail, as they did) it
    finds the reused record at RTGL_AMD_HYBRID_DIV=2 and at no other divisor -- and stale rays, with one wave per SIMD on culled bounces,
    at 2, 3 and 4: ray_k names the last turn whose row was not empty, which may be any earlier turn of the wave.
  * rt_scan.hpp calls the header and keeps no copy.
  * the shapes of tests/test_gpu_tuning_knobs.py (tests/tuning_knob_cases.py) still make waves take two turns and then claim, by the
    launch policy of rt_scan_launch.hpp."""
import os
import re
import subprocess

import pytest

import tuning_knob_cases as tk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
GXX = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined"]


@pytest.fixture(scope="module")
def check_runs(tmp_path_factory):
    """the check program under the kernel's rule and under the parent's: built, then run side by side"""
    tmp = tmp_path_factory.mktemp("scan_items")
    src = os.path.join(ROOT, "tests", "cpp", "scan_items_check.cpp")
    exes = {"new": (str(tmp / "scan_items_check"), []), "parent": (str(tmp / "scan_items_check_parent"), ["-DSCAN_ITEMS_PARENT_RULE"])}
    for exe, flags in exes.values():
        subprocess.check_call(GXX + flags + [src, "-o", exe])
    procs = {k: subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k, (exe, _) in exes.items()}
    out = {}
    for k, p in procs.items():
        text, _ = p.communicate(timeout=240)
        out[k] = (p.returncode, text)
    return out


def test_scan_items_program_under_sanitizers(check_runs):
    code, text = check_runs["new"]
    assert code == 0, text
    assert "runtime error" not in text and "Sanitizer" not in text, text
    assert re.search(r"^ok: \d+ interleavings, 0 failures$", text, re.M), text


def test_the_model_finds_the_parents_defect(check_runs):
    code, text = check_runs["parent"]
    assert code == 0 and "runtime error" not in text and "Sanitizer" not in text, text
    print(text)
    found = {(int(d), kind): what for d, kind, what in re.findall(r"^parent-rule hybrid_div (\d+) (record|rays): (VIOLATION|clean)", text, re.M)}
    assert sorted(found) == sorted((d, k) for d in tk.HYBRID_DIVS for k in ("record", "rays")), text
    # the record read ahead: the last turn has no successor, its index can only be claimed where k_last < n_tail -- hybrid_div 2
    assert found[(2, "record")] == "VIOLATION", text
    assert all(found[(d, "record")] == "clean" for d in tk.HYBRID_DIVS if d != 2), text
    # the rays in flight (one wave per SIMD): ray_k moves on only to a successor whose row is not empty
    assert [d for d in tk.HYBRID_DIVS if found[(d, "rays")] == "VIOLATION"] == [2, 3, 4], text
    witness = re.search(r"hybrid_div 2 record: VIOLATION in \d+ shapes; first: reused record: .*hybrid_div 2 .* holds granule (\d+), item_of gives (\d+)", text)
    assert witness and witness.group(1) != witness.group(2), text


def test_header_is_host_only_and_the_kernel_keeps_no_copy():
    with open(os.path.join(CSRC, "rt_scan_items.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<algorithm>", "<cstdint>"]
    with open(os.path.join(CSRC, "rt_scan.hpp")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    for call in ("first_chunk(", "blocks_on(", "rank_on(", "hdiv_of(", "n_tail(", "hybrid_granule(", "claim_batch_hybrid(", "claim_batch_dynamic("):
        assert "rt_scan_items::" + call in code, call
    assert not re.search(r"\bhturn\b|\bkXcds\b|\bby_xcd\b", code)                        # the turn mapping and the block layout, written out
    assert not re.search(r"hdiv\s*\*\s*k|n_gran\s*/\s*hdiv", code)                       # the tail mapping and n_tail
    assert not re.search(r"rem\s*/\s*\(", code)                                          # the claim batch
    # both places where a wave enters the tail: the start (nothing read ahead yet: the record is declared behind it) and advance()
    assert len(re.findall(r"tail\s*=\s*true", code)) == 2
    assert re.search(r"tail = true; step = 1u; rec_k = kNone; ray_k = kNone; claim\(0u, k, hi\)", code)
    start = code.index("tail = true")
    assert code.index("uint32_t rec_k = kNone") > start and code.index("uint32_t ray_k = kNone") > start
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        host = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "rt_scan_items::hybrid_div_accepted(" in host and "rt_scan_items::kHybridDivDefault" in host


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "rt_scan_launch.hpp"
int main(int argc, char **argv)
{
    if (argc != 9) return 2;      // CUs, quads, mf_chunk_quads, scan_waves, scan_dynamic, cull, rays, items per wave
    const rt_scan_launch::Setup s = {(uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
    const uint32_t n = (uint32_t)atoi(argv[7]);
    const rt_scan_launch::Launch L = rt_scan_launch::launch(s, (uint64_t)atoi(argv[8]), n, n, 0u, false);
    printf("%u %u %u %u %d %d %u\n", L.blocks, L.chunks, L.waves, L.est_gran, L.dist, L.cull, L.chunk_quads);
    return 0;
}
"""


@pytest.fixture(scope="module")
def launch_driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launch_driver")
    src, exe = tmp / "launch_driver.cpp", str(tmp / "launch_driver")
    src.write_text(DRIVER)
    subprocess.check_call(GXX + ["-I", CSRC, str(src), "-o", exe])
    return lambda *args: [int(x) for x in subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]


def test_items_per_wave_values_cut_the_mesh_differently(launch_driver):
    """the case of test_gpu_tuning_knobs.py::test_items_per_wave_changes_the_chunking_and_nothing_else is not vacuous"""
    w, h = tk.ITEMS_SIZE
    got = {v: launch_driver(tk.N_CUS, tk.ITEMS_QUADS, 32, 0, 1, 1, tk.rays(w, h), v)[6] for v in tk.ITEMS_PER_WAVE}
    assert got == tk.ITEMS_CHUNK_QUADS and len(set(got.values())) >= 3, got


def test_gpu_shapes_still_take_turns_and_claim(launch_driver):
    """the camera bounce of every hybrid case of tests/test_gpu_tuning_knobs.py: (blocks per chunk, step, turns of the busiest wave, n_tail)"""
    table = {}
    for family, quads, sizes in (("chunks", tk.CHUNKS_QUADS, tk.CHUNKS_SIZES), ("blocks", tk.BLOCKS_QUADS, tk.BLOCKS_SIZES)):
        for (w, h), n_gran in sizes.items():
            for waves in tk.SCAN_WAVES:
                out = launch_driver(tk.N_CUS, quads, 1, waves, 4, 1, tk.rays(w, h), 3)
                blocks, chunks, per_block, est_gran, dist, cull = out[:6]
                assert (chunks, per_block, est_gran, dist, cull) == (quads, 4 * waves, n_gran, 3, 1), out      # one quad per chunk, hybrid, culled
                assert blocks % chunks == 0
                step = blocks // chunks * per_block
                for d in tk.HYBRID_DIVS:
                    table[(family, (w, h), waves, d)] = (blocks // chunks, step) + tk.hybrid_figures(n_gran, step, d)
    for key in sorted(table):
        print(key, table[key])
    assert all(table[("chunks", s, w, d)][:2] == (1, 4 * w) for s in tk.CHUNKS_SIZES for w in tk.SCAN_WAVES for d in tk.HYBRID_DIVS)
    assert all(table[("blocks", s, w, d)][:2] == (21, 84 * w) for s in tk.BLOCKS_SIZES for w in tk.SCAN_WAVES for d in tk.HYBRID_DIVS)
    # every divisor that has turns and a tail at all (2, 3, 4, 7), with four and with eight waves per block: in each family some size lets a
    # wave take two turns or more and leaves a tail to claim
    for family, sizes in (("chunks", tk.CHUNKS_SIZES), ("blocks", tk.BLOCKS_SIZES)):
        for waves in tk.SCAN_WAVES:
            for d in (2, 3, 4, 7):
                assert any(table[(family, s, waves, d)][2] >= 2 and table[(family, s, waves, d)][3] >= 1 for s in sizes), (family, waves, d)
    # the figures the device module's docstring quotes
    assert table[("chunks", (48, 32), 1, 2)] == (1, 4, 2, 6) and table[("chunks", (80, 64), 2, 2)] == (1, 8, 3, 20)
    assert table[("blocks", (256, 176), 2, 2)] == (21, 168, 2, 176) and table[("blocks", (256, 176), 1, 7)] == (21, 84, 4, 50)
