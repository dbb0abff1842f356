"""The host rules of the six older post-process calls (rtgl_denoise, rtgl_denoise_guided, rtgl_temporal_accumulate, rtgl_temporal_clip,
rtgl_tonemap, rtgl_error_estimate; raytracer.glsl_amd/csrc/rt_{denoise,temporal,tonemap,error}_plan.hpp), without a GPU.
  * tests/golden/post_replies.json holds what the six calls answered before the rules moved into those headers: every parameter probe in
    every state (tests/golden/make_post_replies.py took it on the device).  tests/cpp/{denoise,temporal,tonemap,error}_plan_check.cpp,
    built by the host compiler with the address and undefined-behaviour sanitizers and run as child processes, answer the same probes
    from the headers, each state given as plain values: status and whole message must be the recorded ones.
    tests/test_gpu_post_replies.py asks the built library the same.
  * the programs' own checks: defaults, the geometry of the denoisers' passes, the snapshot's life against the mirror's Estimator, the
    factors of the estimate bit for bit; a mutated copy of each header makes its program fail.
  * the headers are host-only, rtgl_amd.hip calls what they name, and the six bodies keep no rule's text of their own."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ERR_INVALID, ERR_STATE = -1, -4
# program -> (the calls it answers, the values of a state it is given, in the order of its `state` line)
PROGRAMS = {"denoise": (["rtgl_denoise", "rtgl_denoise_guided"],
                        ["tiled", "px", "aov", "aov_restart", "aov_n", "denoise_source", "denoise_variance", "tm_moments", "has_temporal"]),
            "temporal": (["rtgl_temporal_accumulate", "rtgl_temporal_clip"], ["tiled", "px", "aov", "aov_restart", "aov_n", "temporal_moments", "has_temporal"]),
            "tonemap": (["rtgl_tonemap"], ["tiled", "px", "has_denoised", "has_temporal"]),
            "error": (["rtgl_error_estimate"], ["tiled", "rendered", "fn", "fm", "first", "snap", "width", "height"])}
# header -> (the functions rtgl_amd.hip must call, one mutation that its program must notice)
HEADERS = {"denoise": (["default_params", "default_guided_params", "invalid", "planes_needed", "input_refused", "guided_variance_refused", "pass", "lds_bytes",
                        "prepare_grid_x", "prepare_grid_y", "identity_blocks", "pixels", "record_bytes", "near_bytes", "scratch_buffers", "guided_scratch_buffers"],
                       ("if (!(p.sigma_lum > 0.0f))", "if (!(p.sigma_lum >= 0.0f))")),
           "temporal": (["default_params", "default_clip_params", "invalid", "planes_needed", "planes_refused", "pixels_refused", "clip_refused", "history_usable",
                         "turn", "grid_x", "grid_y", "pixels", "record_bytes"],
                        ("has_temporal ? from ^ 1 : from", "has_temporal ? from : from ^ 1")),
           "tonemap": (["default_params", "invalid", "automatic", "source_refused", "pixels_refused", "blocks", "display_bytes"],
                       ("if (p.adapt > 1.0f)", "if (p.adapt >= 1.0f)")),
           "error": (["default_params", "invalid", "drop", "rendered_frame", "refused", "plan", "taken", "footprint_side", "footprint", "tiles_along",
                      "record_bytes", "snapshot_bytes"],
                     ("fn > (int64_t)s.fm", "fn >= (int64_t)s.fm"))}


def load_record():
    """(the record with every message index replaced by its text, the recorder's module)"""
    spec = importlib.util.spec_from_file_location("make_post_replies", os.path.join(GOLDEN, "make_post_replies.py"))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    with open(os.path.join(GOLDEN, "post_replies.json")) as f:
        return recorder.with_texts(json.load(f)), recorder


@pytest.fixture(scope="module")
def record():
    return load_record()[0]


@pytest.fixture(scope="module")
def recorder():
    return load_record()[1]


def build(name, source_dir, out_dir):
    exe = os.path.join(str(out_dir), name + "_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", os.path.join(source_dir, name + "_plan_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("post_plans")
    return {name: build(name, os.path.join(ROOT, "tests", "cpp"), out) for name in PROGRAMS}


def library_source():
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_plan_program_under_sanitizers(name, programs):
    done = subprocess.run([programs[name]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout == name + "_plan_check: ok\n", done.stdout


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_replies_of_every_state_as_recorded(name, programs, record, recorder):
    calls, keys = PROGRAMS[name]
    tiled_text = {call: recorder.entry_literals(library_source(), call) for call in calls}
    lines, expected = [], []
    for state, s in record["states"].items():
        lines.append("state " + " ".join(str(int(s["values"][k])) for k in keys))
        for call in calls:
            for (label, words), (rc, left) in zip(record["probes"][call], s["replies"][call]):
                lines.append(call + " " + ("null" if words is None else " ".join(map(str, words))))
                expected.append((state, call, label, rc, left))
    done = subprocess.run([programs[name], "replay"], input="".join(line + "\n" for line in lines), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr, done.stderr
    answers = done.stdout.split("\n")[:-1]
    assert len(answers) == len(expected)
    for answer, (state, call, label, rc, left) in zip(answers, expected):
        where = (state, call, label)
        if answer == "tiled":      # the one refusal whose text rtgl_amd.hip keeps
            assert [left] == tiled_text[call] and rc == ERR_STATE, where
        elif rc == 0:
            assert answer == ("0" if left is None else "0 %d %d %d" % tuple(left)), where
        else:
            assert answer == "%d\t%s" % (rc, left) and rc in (ERR_INVALID, ERR_STATE), where


def test_record_is_the_one_the_issue_describes(record, recorder):
    assert record["calls"] == [c for c, _, _ in recorder.CALLS] and len(record["calls"]) == 6
    states = record["states"]
    assert len(states) >= 19 and all(s["values"]["width"] == s["values"]["height"] == 32 for s in states.values())
    assert sum(s["values"]["tiled"] for s in states.values()) == 1 and not states["fresh"]["values"]["rendered"]
    assert {s["values"]["tm_moments"] for s in states.values()} == {0, 1, 2} and {s["values"]["denoise_variance"] for s in states.values()} == {0, 1}
    assert any(s["values"]["aov_restart"] and s["values"]["rendered"] and s["values"]["aov"] for s in states.values())      # planes enabled after the frames
    assert any(s["values"]["has_denoised"] for s in states.values()) and any(s["values"]["snap"] for s in states.values())
    for call, rows in record["probes"].items():
        labels = [label for label, _ in rows]
        assert labels[:2] == ["NULL", "defaults"] and rows[0][1] is None and all(len(r) == len(rows) for r in (s["replies"][call] for s in states.values())), call
        assert any("nan" in x for x in labels) and any("-inf" in x for x in labels) and any("1e-45" in x for x in labels) and any("=-0.0" in x for x in labels), call
        assert any("4294967295" in x for x in labels), call
    for call, need in (("rtgl_denoise", ["passes=8", "passes=9"]), ("rtgl_tonemap", ["adapt=1.0", "adapt=1.0000001192092896", "low_permille=999 high_permille=0", "low_permille=500 high_permille=499"]),
                       ("rtgl_error_estimate", ["quantile_permille=0", "quantile_permille=1", "quantile_permille=1000", "quantile_permille=1001"])):
        assert set(need) <= {label for label, _ in record["probes"][call]}, call
    # every rule's text of the six bodies, as they were, is in the record, but for the two kinds no device run reaches
    messages = {left for s in states.values() for rows in s["replies"].values() for rc, left in rows if rc}
    assert not messages & set(recorder.UNREACHABLE) and len(recorder.UNREACHABLE) == 6
    assert len(messages) >= 50


@pytest.mark.parametrize("name", sorted(HEADERS))
def test_plan_check_fails_on_a_mutated_header(name, tmp_path):
    old, new = HEADERS[name][1]
    shutil.copytree(os.path.join(ROOT, "tests", "cpp"), tmp_path / "tests" / "cpp")
    os.makedirs(tmp_path / "raytracer.glsl_amd" / "csrc")
    for header in os.listdir(CSRC):
        if header.endswith("_plan.hpp"):
            shutil.copy(os.path.join(CSRC, header), tmp_path / "raytracer.glsl_amd" / "csrc" / header)
    path = tmp_path / "raytracer.glsl_amd" / "csrc" / ("rt_%s_plan.hpp" % name)
    text = path.read_text()
    assert text.count(old) == 1, f"the text of the mutation of rt_{name}_plan.hpp is not in the header (once)"
    path.write_text(text.replace(old, new))
    exe = build(name, str(tmp_path / "tests" / "cpp"), tmp_path)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert done.returncode != 0 and "checks failed" in done.stdout, f"the mutated rt_{name}_plan.hpp passed its check:\n{done.stdout}"


def test_headers_are_host_only_and_the_library_uses_them():
    code = "".join(re.sub(r"//.*", "", line) + "\n" for line in library_source().split("\n"))
    for name, (functions, _) in HEADERS.items():
        with open(os.path.join(CSRC, "rt_%s_plan.hpp" % name)) as f:
            header = f.read()
        assert set(re.findall(r"#include\s+(\S+)", header)) == {"<cmath>", "<cstddef>", "<cstdint>"}, name
        plain = "".join(re.sub(r"//.*", "", line) for line in header.splitlines(True))
        assert "rtgl_context" not in plain and "hip" not in plain.lower() and "__" not in plain, name      # plain values in, plain values out
        for function in functions:
            assert f"rt_{name}_plan::{function}(" in code, (name, function)
        assert f"sizeof(rt_{name}_plan::" in code, name                     # tied to the public header by a static_assert
    assert "rt_tonemap_plan::Sets tone" in code and ".after_auto_call()" in code and "rt_error_plan::Snapshot err" in code
    assert "err_epoch" not in code and len(re.findall(r"rt_error_plan::drop\(ctx->err\)", code)) == 8
    for kept in ("rt_bucket_guide_plan::planes_refused(", "temporal_camera(", "read_plane(", "device_plane("):
        assert kept in code, kept


def test_the_six_bodies_keep_no_rule_of_their_own(recorder):
    source = library_source()
    for call, _, _ in recorder.CALLS:
        body = re.search(r'extern "C" int %s\(.*?\n}\n' % call, source, re.S).group(0)
        literals = recorder.entry_literals(source, call)
        assert len(literals) == 1 and literals[0].startswith(call + ": a tiled or multi-device context holds strips"), call
        rest = [m for m in re.findall(r"fail\(ctx, [^;]*;", body) if '"%s: a tiled' % call not in m]
        assert rest and all(re.fullmatch(r'fail\(ctx, [\w.]+, std::string\("%s: "\) \+ (?:no\.)?why\);' % call, m) for m in rest), (call, rest)
        assert "isfinite" not in body and "reserved" not in body
    assert source.count("\n") < 3143      # the library's source got shorter by the move
