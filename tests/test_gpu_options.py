"""rtgl_set_option, rtgl_get_option and the environment's spellings of the options, on the device, against the replies recorded before
the options moved into one table (tests/golden/option_replies.json; tests/test_options.py replays the same record on the CPU).

The probes are the recorder's own (tests/golden/make_option_replies.py, record()): 8 x 8 contexts that never see a scene or a frame, so
every probe is an argument check or an accepted store.  Return codes, messages and the values read back must all be the recorded ones."""
import pytest

from test_options import load_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replies(rt, gpu_lib):
    want, recorder = load_record()
    return recorder.with_texts(recorder.record(rt.host)), want


def test_set_option_replies_as_recorded(replies):
    got, want = replies
    assert got["probes"] == want["probes"] and list(got["set"]) == list(want["set"])
    for key in want["set"]:
        for value, g, w in zip(want["probes"], got["set"][key], want["set"][key]):
            assert g == w, (key, value)      # [rc, message, rc of the read afterwards, its value or message]


def test_get_option_replies_as_recorded(replies):
    got, want = replies
    for section in ("fresh", "unknown", "null_key", "null_value"):
        assert got[section] == want[section], section


def test_environment_spellings_as_recorded(replies):
    got, want = replies
    for name in want["env"]:
        assert got["env"][name] == want["env"][name], name
    assert list(got["env"]) == list(want["env"])
