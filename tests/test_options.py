"""The option table (raytracer.glsl_amd/csrc/rt_options.hpp) against the replies of the library before the table existed, without a GPU.
  * tests/golden/option_replies.json holds what rtgl_set_option, rtgl_get_option and the environment's spellings answered then
    (tests/golden/make_option_replies.py took it on the device).  tests/cpp/options_check.cpp, built by the host compiler with the
    address and undefined-behaviour sanitizers and run as a child process, answers the same probes from the header: acceptance, message
    and the value read back must be the recorded ones.  tests/test_gpu_options.py asks the built library the same.
  * the table itself: no key or environment name twice, no row for a derived key, RTGL_AMD_SORT_MOVE.
  * the header is host-only; rtgl_amd.hip keeps no chain over the keys and no getenv of a name the table has; include/rtgl_amd.h names
    every key."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K_SET, K_GET = 1, 2


def load_record():
    """(the record with every message index replaced by its text, the recorder's module)"""
    spec = importlib.util.spec_from_file_location("make_option_replies", os.path.join(GOLDEN, "make_option_replies.py"))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    with open(os.path.join(GOLDEN, "option_replies.json")) as f:
        return recorder.with_texts(json.load(f)), recorder


@pytest.fixture(scope="module")
def record():
    return load_record()[0]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("options") / "options_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "cpp", "options_check.cpp"), "-o", exe])

    def ask(lines):
        done = subprocess.run([exe], input="".join(line + "\n" for line in lines), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert done.returncode == 0 and not done.stderr, done.stderr
        answers = done.stdout.split("\n")[:-1]
        return answers
    return ask


@pytest.fixture(scope="module")
def rows(ask):
    """[(key or None, environment name or None, flags)]"""
    answers = ask(["rows"])
    assert answers[-1] == "ok"
    return [(k if k != "-" else None, e if e != "-" else None, int(f)) for k, e, f in (a.split(" ")[1:] for a in answers[:-1])]


def test_record_is_the_one_the_issue_describes(record):
    probes = record["probes"]
    assert probes == sorted(probes) and set(range(-2, 71)) <= set(probes)
    assert {127, 128, 129, 192, 255, 256, 4032, 4095, 4096, 4097, 4160, 131072, 2 ** 31 - 1, -2 ** 31} <= set(probes)
    assert all(len(replies) == len(probes) for replies in record["set"].values())
    assert all(list(e["replies"]) == ["0", "1", "2", "3", "4", "5", "16", "17", "-1", "", "abc", "2x", " 1"] for e in record["env"].values())


def test_set_and_read_back_as_recorded(ask, record):
    lines = []
    for key in record["set"]:
        lines.append("reset")
        for value in record["probes"]:
            lines += [f"set {key} {value}", f"get {key}"]
    answers = iter(ask(lines))
    for key, replies in record["set"].items():
        assert next(answers) == "ok"
        for value, (rc, message, get_rc, got) in zip(record["probes"], replies):
            stored, read = next(answers), next(answers)
            assert stored == ("ok" if rc == 0 else "refused " + message), (key, value)
            assert rc in (0, -1) and (message is None) == (rc == 0), (key, value)
            if read == "unknown":      # the table does not answer this read: the library refused it, or answers it as a derived key
                assert key in record["derived"] or (get_rc, got) == (-1, "unknown option " + key), (key, value)
            else:
                assert get_rc == 0 and read == f"value {got}", (key, value)


def test_defaults_and_unknown_keys_as_recorded(ask, record):
    table = [key for key in record["fresh"] if key not in record["derived"]]
    answers = ask(["reset"] + [f"get {key}" for key in table] + ["set no_such_option 1", "get no_such_option"])
    assert answers[1:-2] == [f"value {record['fresh'][key][1]}" for key in table] and all(record["fresh"][key][0] == 0 for key in table)
    assert answers[-2:] == ["unknown", "unknown"]
    assert record["unknown"] == {"set": [-1, "unknown option no_such_option"], "get": [-1, "unknown option no_such_option"]}


def test_environment_as_recorded(ask, record):
    cases = [(name, text, e["replies"][text]) for name, e in record["env"].items() for text in e["replies"]]
    answers = ask([f"env {name} {text}" for name, text, _ in cases])
    for (name, text, (rc, value)), answer in zip(cases, answers):
        default = record["fresh"][record["env"][name]["option"]][1]
        assert rc == 0 and answer.split(" ")[:2] == ["value", str(value)], (name, text, answer)
        assert answer.endswith(" set") or value == default, (name, text, answer)      # a value that was not kept is the default


def test_sort_move_is_an_environment_spelling_only(ask, rows, record):
    assert (None, "RTGL_AMD_SORT_MOVE", 0) in rows
    # it takes 0 and 1 (as atoi reads the text: "" and "abc" are 0) and otherwise leaves the default, 1
    taken = {"0": "value 0 set", "1": "value 1 set", " 1": "value 1 set", "": "value 0 set", "abc": "value 0 set"}
    texts = list(record["env"]["RTGL_AMD_NARROW_FUSED"]["replies"]) + ["-2", "64", "2147483647"]
    answers = ask([f"env RTGL_AMD_SORT_MOVE {text}" for text in texts])
    assert answers == [taken.get(text, "value 1 kept") for text in texts]


def test_table_has_each_name_once_and_no_derived_key(rows, record):
    keys, names = [k for k, _, _ in rows if k], [e for _, e, _ in rows if e]
    assert len(keys) == len(set(keys)) and len(names) == len(set(names))
    assert not set(keys) & set(record["derived"]) - {"mf_group_quads"} and len(record["derived"]) == 7
    # "mf_group_quads": the option is a row that can be set; the read is derived (the value in use), so the row cannot be read
    assert [f for k, _, f in rows if k == "mf_group_quads"] == [K_SET]
    assert [f & (K_SET | K_GET) for k, _, f in rows if k == "debug_skip_exact"] == [K_SET]
    assert {k for k, _, f in rows if f & K_SET} == set(record["set"])
    assert {k for k, _, f in rows if f & K_GET} | set(record["derived"]) == set(record["fresh"])
    assert set(names) == set(record["env"]) | {"RTGL_AMD_SORT_MOVE"}
    assert {k: e for k, e, _ in rows if k and e} == {e["option"]: name for name, e in record["env"].items()}


def stripped(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/", "", "".join(re.sub(r"//.*", "", line) for line in f), flags=re.S)


# getenv("...") calls that rtgl_amd.hip keeps: the tuning variables and switches read where they are used
READ_IN_PLACE = {"RTGL_AMD_PRIVATE_STREAMS": 2, "RTGL_AMD_ALLOW_CONCURRENT_PIPELINES": 1, "RTGL_AMD_MULTI_THREADS": 1, "RTGL_AMD_KD_LAMBDA": 1,
                 "RTGL_AMD_CULL_NODE": 1, "RTGL_AMD_ROW_GAMMA": 2, "RTGL_AMD_SORT_OB": 1, "RTGL_AMD_SORT_DB": 1, "RTGL_AMD_BIN_SPLIT": 1,
                 "RTGL_AMD_BIN_UNIT": 1, "RTGL_AMD_HYBRID_DIV": 1, "RTGL_AMD_NO_CAMERA_KEEP": 1, "RTGL_AMD_ITEMS_PER_WAVE": 2,
                 "RTGL_AMD_SCHED_FILL": 1, "RTGL_AMD_HIST_FILL": 1}


def test_header_is_host_only_and_the_library_keeps_no_second_copy(rows):
    with open(os.path.join(CSRC, "rt_options.hpp")) as f:
        header = f.read()
    includes = re.findall(r"#include\s+(\S+)", header)
    assert includes and all(re.fullmatch(r"<c[a-z]+>", i) for i in includes), includes
    assert "getenv(" not in header
    code = stripped(os.path.join(CSRC, "rtgl_amd.hip"))
    assert "strcmp(key," not in code
    assert len(re.findall(r"rt_options::read_environment\(", code)) == 1
    found = re.findall(r'getenv\("(RTGL_AMD_[A-Z_]+)"\)', code)
    assert not set(found) & {e for _, e, _ in rows if e}
    assert set(found) == set(READ_IN_PLACE) and all(found.count(n) <= READ_IN_PLACE[n] for n in READ_IN_PLACE), found


def test_public_header_names_every_key(rows, record):
    with open(os.path.join(ROOT, "include", "rtgl_amd.h")) as f:
        text = f.read()
    comments = [re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, text, re.S).group(1) for name in ("rtgl_set_option", "rtgl_get_option")]
    missing = [k for k in [k for k, _, _ in rows if k] + record["derived"] if '"%s"' % k not in comments[0] + comments[1]]
    assert not missing, missing
    assert all('"%s"' % k in comments[1] for k in record["derived"])
