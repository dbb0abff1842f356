"""The six older post-process calls on the device, against the replies recorded before their host rules moved into the plan headers
(tests/golden/post_replies.json; tests/test_post_plans.py replays the same record on the CPU).

The probes and the states are the recorder's own (tests/golden/make_post_replies.py, record()): 32 x 32 contexts, the small scene, a few
frames.  Return codes, messages, what the host then knows of each state, and the summary's valid, frames_now and frames_snapshot after
every successful rtgl_error_estimate must all be the recorded ones."""
import pytest

from test_post_plans import load_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replies(rt, gpu_lib):
    want, recorder = load_record()
    return recorder.with_texts(recorder.record(rt.host)), want


def test_probes_and_states_are_the_recorded_ones(replies):
    got, want = replies
    assert got["calls"] == want["calls"] and got["probes"] == want["probes"]
    assert list(got["states"]) == list(want["states"])
    for state in want["states"]:
        assert got["states"][state]["values"] == want["states"][state]["values"], state


@pytest.mark.parametrize("call", ["rtgl_error_estimate", "rtgl_tonemap", "rtgl_temporal_clip", "rtgl_denoise", "rtgl_denoise_guided", "rtgl_temporal_accumulate"])
def test_replies_as_recorded(call, replies):
    got, want = replies
    for state, s in want["states"].items():
        for (label, _), g, w in zip(want["probes"][call], got["states"][state]["replies"][call], s["replies"][call]):
            assert g == w, (state, label)      # [rc, message, or what a success left]
