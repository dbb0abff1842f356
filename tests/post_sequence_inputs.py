"""Seeded call sequences over ONE context that cross the post-process features (include/rtgl_amd.h: both denoisers, the temporal calls, the
display transform, the error estimate, the adaptive and the robust session with its estimate and its denoiser) for
tests/post_sequence_model.py, the CPU test of this file and tests/test_gpu_post_sequences.py.  A helper, not a test; plain numpy and
Python, no device.

`sequence(seed)` returns a fixed scene (the mesh, spheres and cube map of the post-process tests, 4 bounces), one of three sizes and a
list of 24 to 40 steps.  A step is (kind, args); `frame_params` turns the args of a frame into its uniforms.  A sequence is a row of UNITS:
each unit is a short scripted stretch that sets up one or more of the named HAZARDS (a pair of calls of which the first writes host state
the second reads), with its parameters taken in turn from the alphabet's lists, starting at a place that depends on the seed.  The
fifteen rows hold every unit twice -- nine rows for the calls up to rtgl_robust_error_estimate, six for rtgl_robust_denoise, whose session
has to be filled first -- so fifteen consecutive seeds meet every hazard at least twice and every alphabet entry at least once whatever
the first seed is (tests/test_post_sequence_inputs.py counts them).  Steps the contract refuses are wanted: a unit of the first nine rows
does not look at what the units before it left behind, and several ask for a refusal outright.

HAZARDS and ALPHABET are data: (name, predicate over a step list) and (name, predicate over a step)."""
from collections import namedtuple

import numpy as np

import raytracer_glsl_amd
import temporal_inputs as ti

sc = raytracer_glsl_amd.scenes
f32 = np.float32

Step = namedtuple("Step", "kind args")
Sequence = namedtuple("Sequence", "seed W H scene base steps units")

SIZES = [(48, 40), (70, 53), (33, 17)]     # (W, H): whole tiles; a multiple of neither 8 nor 16; narrower than a 64-column block, one ragged tile row
DEFAULT_SEQUENCES = 15
MIN_STEPS, MAX_STEPS = 24, 40
BOUNCES = 4
A, N, P, IDS, ALL = 1, 2, 4, 8, 15
AOV_MASKS = (0, P, N | P, A | N | P, ALL)
PASSES = (0, 1, 2, 5)
BUCKETS = (4, 8, 16)
MASKS = ("checker", "left", "none", "all")
CAMERAS = [ti.cam(), ti.cam((0.6, 0.2, -35.0)), ti.cam(yaw=0.03, pitch=0.01), ti.cam((1.0, 0.0, -33.0), yaw=-0.02)]
DENOISERS = ("denoise", "denoise_guided")
FILTERS = DENOISERS + ("robust_denoise",)                              # the writers of the denoised buffer
NEED_PLANES = DENOISERS + ("temporal_accumulate", "temporal_clip")
RESTARTS = ("clear_image", "set_aov", "adaptive_begin")                # the calls that restart the first-hit planes
TONE = ("tonemap", "tonemap_reset")
FEATURES = dict(denoise=("denoise",), denoise_guided=("denoise_guided",), temporal=("temporal_accumulate",), temporal_clip=("temporal_clip",),
                tonemap=("tonemap",), error=("error_estimate",), adaptive=("adaptive_begin", "adaptive_frame", "adaptive_update", "adaptive_set_mask"),
                robust=("robust_begin", "robust_accumulate", "robust_resolve", "robust_end"), robust_error=("robust_error_estimate",),
                robust_denoise=("robust_denoise",))


def default_seeds(n=DEFAULT_SEQUENCES, start=0):
    return list(range(int(start), int(start) + int(n)))


def scene():
    return sc.scene_mesh(10, 5, env_size=16)


def base_params():
    return sc.params_c2().replace(max_bounce=BOUNCES)


def frame_params(base, args):
    """the uniforms of a "render" or "adaptive_frame" step"""
    return base.replace(frames=args["frames"], reset_flag=args["reset_flag"], random=args["random"], samples=args.get("samples", 1), **CAMERAS[args["camera"]])


def written_image(h, w, k):
    """what a "write_image" step writes: positive, smooth, different per channel, alpha 1"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rgb = [0.5 + 0.4 * np.sin(0.21 * x + 0.9 * c + k) * np.cos(0.13 * y - 0.5 * c) for c in range(3)]
    return np.stack(rgb + [np.ones((h, w))], -1).astype(f32)


def mask_tiles(name, h, w):
    """the explicit mask of an "adaptive_set_mask" step, (ty, tx) uint8"""
    ty, tx = (h + 15) // 16, (w + 15) // 16
    if name == "checker":
        return (np.add.outer(np.arange(ty), np.arange(tx)) % 2).astype(np.uint8)
    if name == "left":
        return np.repeat((np.arange(tx) < (tx + 1) // 2)[None, :], ty, 0).astype(np.uint8)
    return np.full((ty, tx), 1 if name == "all" else 0, np.uint8)


def resolved(seq, step):
    """the step with the arrays its args only name: the pixels of "write_image", the tiles of "adaptive_set_mask" """
    if step.kind == "write_image":
        return Step(step.kind, dict(step.args, pixels=written_image(seq.H, seq.W, step.args["image"])))
    if step.kind == "adaptive_set_mask":
        return Step(step.kind, dict(step.args, tiles=mask_tiles(step.args["mask"], seq.H, seq.W)))
    return step


# ------------------------------------------------------------------------------------------------ the generator

class _Gen:
    def __init__(self, seed):
        self.seed, self.rng = seed, np.random.default_rng([seed, 29, 20263])
        self.frames, self.camera, self.turn = 0, 0, {}

    def pick(self, name, values):
        """the lists of the alphabet in turn, from a place that depends on the seed: consecutive seeds see every value"""
        k = self.turn.get(name, 0)
        self.turn[name] = k + 1
        return values[(self.seed + k) % len(values)]

    def word(self):
        return int(self.rng.integers(0, 2 ** 31))

    def render(self, reset=0, move=None, session=False, restart=False, sync=None):
        """one ordinary frame.  session: a session frame (frames 0, reset_flag 1, the count stands still).  restart: the count starts
        again at 1; otherwise it goes on, across a reset frame too: a larger `frames` after the event is what makes a stale snapshot of
        rtgl_error_estimate look usable.  sync: whether the test waits for the frame; None takes the list's turn."""
        if self.pick("move", (False, True, False)) if move is None else move:
            self.camera = (self.camera + 1) % len(CAMERAS)
        if restart:
            self.frames = 0
        if not session:
            self.frames += 1
        return Step("render", dict(frames=0 if session else self.frames, reset_flag=1 if session else reset, camera=self.camera, random=self.word(),
                                   sync=self.pick("sync", (True, False)) if sync is None else sync))

    def adaptive_frame(self):
        return Step("adaptive_frame", dict(frames=77, reset_flag=self.pick("af_reset", (0, 1)), camera=self.camera, random=self.word(), sync=self.pick("sync", (True, False))))

    def denoise(self, passes=None, planes=True, **over):
        args = dict(passes=self.pick("dn_passes", PASSES) if passes is None else passes, demodulate=self.pick("dn_demod", (True, False)) and planes,
                    sigma_color=self.pick("dn_sc", (16.0, 0.0)), sigma_normal=self.pick("dn_sn", (0.3, 0.0)) if planes else 0.0,
                    sigma_position=self.pick("dn_sp", (0.05, 0.0)) if planes else 0.0)
        args.update(over)
        return Step("denoise", args)

    def guided(self, passes=None, planes=True, **over):
        args = dict(passes=self.pick("dg_passes", PASSES) if passes is None else passes, firefly_ratio=self.pick("dg_ff", (1.0, 0.0)),
                    demodulate=self.pick("dg_demod", (True, False)) and planes, sigma_lum=4.0, sigma_normal=0.3 if planes else 0.0, sigma_position=0.05 if planes else 0.0)
        args.update(over)
        return Step("denoise_guided", args)

    def tonemap(self, source=None, auto=None, **over):
        args = dict(source=self.pick("tm_source", (0, 1, 2)) if source is None else source, op=self.pick("tm_op", (1, 0, 2)),
                    auto=self.pick("tm_auto", (True, False)) if auto is None else auto, adapt=self.pick("tm_adapt", (1.0, 0.5, 0.25)), exposure=self.pick("tm_exp", (1.0, 0.5)))
        args.update(over)
        return Step("tonemap", args)

    def error(self, **over):
        args = dict(keep_snapshot=self.pick("ee_keep", (False, True)), first_frames=1)
        args.update(over)
        return Step("error_estimate", args)

    def adaptive_begin(self, **over):
        args = dict(threshold=self.pick("ab_thr", (0.05, 0.5)), min_samples=self.pick("ab_min", (1, 2)), max_samples=self.pick("ab_max", (4, 1024)))
        args.update(over)
        return Step("adaptive_begin", args)

    def temporal(self, **over):
        args = dict(max_history=self.pick("ta_mh", (32.0, 4.0)), sigma_normal=0.3, sigma_position=self.pick("ta_sp", (0.05, 0.0)))
        args.update(over)
        return Step("temporal_accumulate", args)

    def clip(self, **over):
        args = dict(sigma_scale=self.pick("tc_ss", (2.0, 0.5)), clip_history=3.0, sigma_normal=0.3, sigma_position=0.05)
        args.update(over)
        return Step("temporal_clip", args)

    def resolve(self, dest, gain=None):
        return Step("robust_resolve", dict(dest=dest, gain=self.pick("rr_gain", (1.0, 0.0)) if gain is None else gain))

    def robust_error(self, **over):
        args = dict(threshold=0.05, floor=0.01, gain=self.pick("re_gain", (1.0, 0.0)))
        args.update(over)
        return Step("robust_error_estimate", args)

    def robust_denoise(self, passes=None, planes=True, **over):
        args = dict(passes=self.pick("rd_passes", PASSES) if passes is None else passes, sigma_lum=4.0, sigma_normal=self.pick("rd_sn", (0.3, 0.0)) if planes else 0.0,
                    sigma_position=self.pick("rd_sp", (0.05, 0.0, 0.05)) if planes else 0.0, gain=self.pick("rd_gain", (1.0, 0.0)),
                    demodulate=self.pick("rd_demod", (True, False)) and planes)
        args.update(over)
        return Step("robust_denoise", args)

    def robust_denoise_needs(self, passes=None):
        """rtgl_robust_denoise with parameters that need a plane: the albedo, the normal, the position or all three, in turn"""
        a, n, p = self.pick("rd_need", ((True, 0.0, 0.0), (False, 0.3, 0.0), (False, 0.0, 0.05), (True, 0.3, 0.05)))
        return self.robust_denoise(passes, demodulate=a, sigma_normal=n, sigma_position=p)

    def fill(self, K, frames=4, probe=None):
        """a robust session (begun by the caller) brought to N = K with buckets that differ: `frames` session frames, each folded K / frames
        times (rtgl_robust_accumulate folds the image "AS IT STANDS").  probe: a step put in front of the last fold, at N = K - 1"""
        out = []
        for _ in range(frames):
            out += [self.render(session=True)] + [S("robust_accumulate")] * (K // frames)
        return out if probe is None else out[:-1] + [probe, out[-1]]

    def needs_planes(self):
        """one of the four calls that RTGL_ERR_STATE after the planes restarted, with parameters that need a plane"""
        kind = self.pick("pp", NEED_PLANES[:3])
        if kind == "denoise":
            return self.denoise(demodulate=True, sigma_normal=0.3, sigma_position=0.05)
        if kind == "denoise_guided":
            return self.guided(demodulate=True)
        return self.temporal()


def S(kind, **args):
    return Step(kind, args)


ENDERS = ("render", "clear_image", "write_image", "bind_image", "robust_resolve_image")
PLANES = A | N | P


def unit_source(g):
    """first in its sequence: the calls that need an earlier one, before it; "denoise_source" = 1 before and after the first temporal call"""
    return [g.tonemap(2), g.error(), g.clip(), S("set_aov", mask=PLANES), g.render(session=True), S("set_option", key="denoise_source", value=1), g.denoise(), g.temporal(),
            g.guided(), S("set_option", key="denoise_source", value=0)]


def unit_ender_clear(g):
    """rtgl_clear_image ends the session AND restarts the planes: a call that needs them is refused until a frame"""
    call = g.needs_planes()
    return [S("set_aov", mask=PLANES), g.render(session=True), g.adaptive_begin(), S("clear_image"), call, g.render(session=True), call, S("adaptive_update")]


def unit_ender_render(g):
    """rtgl_adaptive_begin restarts the planes; an ordinary frame ends the session"""
    call = g.needs_planes()
    return [S("set_aov", mask=PLANES), g.render(session=True), g.adaptive_begin(), call, g.render(session=True), call, S("adaptive_update")]


def unit_ender(which):
    def unit(g):
        pre = [S("robust_begin", buckets=g.pick("rb_K", BUCKETS)), g.render(session=True), S("robust_accumulate")] if which == "robust_resolve" else []
        end = g.resolve(1) if which == "robust_resolve" else S("write_image", image=g.word() % 7) if which == "write_image" else S(which)
        return [S("set_aov", mask=0)] + pre + [g.adaptive_begin(), g.adaptive_frame(), end, S("adaptive_update")]
    return unit


def unit_aov_adaptive(g):
    """"aov" set: the planes restart; a masked frame with "aov" still on is refused"""
    call = g.needs_planes()
    return [S("set_aov", mask=g.pick("restart_aov", (PLANES, ALL))), call, g.render(session=True), call, g.adaptive_begin(), g.adaptive_frame(), S("set_aov", mask=0),
            g.adaptive_frame(), S("adaptive_set_mask", mask=g.pick("mask", MASKS)), g.adaptive_frame(), S("adaptive_update")]


def unit_robust_open(g):
    """a robust session left open across an adaptive session and across ordinary frames"""
    return [S("set_aov", mask=0), S("robust_begin", buckets=g.pick("rb_K", BUCKETS)), g.render(session=True), S("robust_accumulate"), g.adaptive_begin(), g.adaptive_frame(),
            g.render(restart=True), g.render(), S("robust_accumulate"), g.resolve(0)]


def unit_denoisers(g):
    """both denoisers in either order with scratch needs that differ, the display transform of each one's result"""
    return [S("set_aov", mask=ALL), g.render(), g.denoise(1), g.tonemap(1), g.guided(5), g.tonemap(1), g.guided(0), g.denoise(2), g.denoise(5), g.guided(0)]


def unit_temporal(g):
    """the history across a change of the normal plane; the display transform of the clipped history"""
    return [S("set_aov", mask=PLANES), g.render(session=True, move=True), g.temporal(), g.clip(), g.tonemap(2), S("set_aov", mask=P), g.render(session=True, move=True),
            g.temporal(sigma_normal=0.0), S("set_aov", mask=N | P), g.render(session=True), g.temporal()]


def unit_invalid(g):
    """one bad argument per feature"""
    return [g.denoise(9), g.guided(9), g.temporal(max_history=0.5), g.clip(sigma_scale=0.0), g.tonemap(0, True, adapt=2.0), g.error(first_frames=-1),
            g.adaptive_begin(min_samples=0), S("robust_begin", buckets=5), g.resolve(2), g.robust_error(threshold=0.0), g.robust_denoise(sigma_lum=0.0),
            S("set_option", key="denoise_source", value=2)]


def unit_tone(g):
    """the exposure's memory and the two histogram sets: auto, manual, auto, reset, auto"""
    return [g.render(), g.tonemap(0, True, adapt=0.5), g.tonemap(0, False), g.render(), g.tonemap(0, True, adapt=0.5), S("tonemap_reset"), g.tonemap(0, True, adapt=0.25),
            S("temporal_reset")]


def unit_robust_image(g):
    """a full session, its error estimate, the resolve into the image between two estimates of the image, the display transform of it"""
    out = [S("robust_begin", buckets=4)]
    for _ in range(4):
        out += [g.render(session=True), S("robust_accumulate")]
    return out + [g.robust_error(), g.render(restart=True), g.error(keep_snapshot=False), g.resolve(1), g.tonemap(0), g.render(), g.error()]


def unit_moments(g):
    """the history across a change of "temporal_moments"; the guided denoiser on the temporal variance"""
    mode = g.pick("tm_mode", (1, 2))
    return [S("set_aov", mask=PLANES), S("set_option", key="temporal_moments", value=mode), g.render(session=True), g.temporal(),
            S("set_option", key="denoise_source", value=1), S("set_option", key="denoise_variance", value=1), g.guided(demodulate=(mode == 2)),
            S("set_option", key="temporal_moments", value=3 - mode), g.temporal(), S("set_option", key="temporal_moments", value=0),
            S("set_option", key="denoise_variance", value=0), S("set_option", key="denoise_source", value=0)]


def unit_robust_twice(g):
    k1 = g.pick("rb_K", BUCKETS)
    k2 = BUCKETS[(BUCKETS.index(k1) + 1) % len(BUCKETS)]
    return [S("robust_begin", buckets=k1), g.render(session=True), S("robust_accumulate"), S("robust_begin", buckets=k2), g.resolve(0), g.render(session=True),
            S("robust_accumulate"), g.robust_error(), g.resolve(0), S("robust_end"), S("robust_accumulate")]


def unit_epochs_a(g):
    """two estimates with no event between, across rtgl_clear_image, across a reset frame; `frames` grows throughout"""
    first = dict(keep_snapshot=False)
    return [S("clear_image"), g.render(), g.error(**first), g.render(), g.error(), S("clear_image"), g.render(), g.error(), g.render(reset=1), g.render(), g.error()]


def unit_epochs_b(g):
    """across rtgl_error_reset, rtgl_write_image_f32, rtgl_bind_device_image"""
    return [g.render(), g.error(keep_snapshot=False), S("error_reset"), g.render(), g.error(), S("write_image", image=g.word() % 7), g.render(), g.error(), S("bind_image"),
            g.render(), g.error()]


def unit_epochs_c(g):
    """across rtgl_adaptive_begin, across a masked frame"""
    return [S("set_aov", mask=0), g.render(), g.error(keep_snapshot=False), g.adaptive_begin(), g.render(), g.error(), g.adaptive_begin(), g.error(), g.adaptive_frame(),
            g.render(), g.error()]


def unit_sweep(g):
    """the pass counts the other units leave to the turn of the lists; a filter that needs no plane; a frame refused for its parameters
    (samples = 0), which leaves an adaptive session open"""
    refused = g.render()
    refused.args["samples"] = 0
    return [S("set_aov", mask=PLANES), g.render(), g.denoise(0), g.guided(1), g.guided(2), g.denoise(5, planes=False), g.tonemap(1), g.adaptive_begin(), refused,
            S("adaptive_update")]


# The units of rtgl_robust_denoise.  All but "rd_open" count on what the "rd_open" at the head of their row leaves: the planes on and
# holding a frame, a session at N >= K whose buckets differ.  Each but "rd_second", which ends the session, leaves that state behind in turn.

def unit_rd_open(K, probe):
    """first in its row, "aov" still 0: a session filled to N = K from four frames, which a batching context holds back until the fold
    behind them; then the planes on and a frame in them.  probe: rtgl_robust_denoise needing no plane at N = K - 1 (refused: an empty
    bucket and nothing else), and the same call right after the last fold"""
    def unit(g):
        call = g.robust_denoise(planes=False) if probe else None
        return [S("robust_begin", buckets=K)] + g.fill(K, probe=call) + ([call] if probe else []) + [S("set_aov", mask=PLANES), g.render(session=True)]
    return unit


def unit_rd_source(g):
    """before any temporal call in its row.  "denoise_source" = 1 with no history: a denoiser is refused, rtgl_robust_denoise filters the
    buckets and is not; after the first temporal call again, and rtgl_denoise_guided behind it takes the history: the latest writer wins"""
    refused = g.denoise() if g.pick("rd_refused", DENOISERS) == "denoise" else g.guided()
    return [S("set_option", key="denoise_source", value=1), refused, g.robust_denoise(1), g.temporal(), g.robust_denoise(5), g.guided(0),
            S("set_option", key="denoise_source", value=0)]


def unit_rd_pairs(robust_first):
    """rtgl_robust_denoise and rtgl_denoise_guided in either order, the pass counts 5 then 0 and 0 or 1 then 5 both ways: the scratch and
    near buffers are met allocated smaller and larger than needed.  The display transform of the robust call's result; rtgl_denoise
    behind it, which leaves the variance buffer the robust call's"""
    def unit(g):
        if robust_first:
            return [g.robust_denoise(1), g.guided(5), g.robust_denoise(0), g.tonemap(1), g.denoise(), g.guided(1), g.robust_denoise(5), g.guided(0)]
        return [g.guided(0), g.robust_denoise(5), g.guided(0), g.robust_denoise(1), g.guided(5), g.robust_denoise(0), g.tonemap(1), g.denoise()]
    return unit


def unit_rd_restarts(g):
    """rtgl_clear_image and rtgl_adaptive_begin restart the planes under a full session: RTGL_ERR_STATE for the planes alone, and the
    same call after one frame is accepted"""
    a, b = g.robust_denoise_needs(), g.robust_denoise_needs()
    return [S("clear_image"), a, g.render(session=True), a, g.adaptive_begin(), b, g.render(session=True), b]


def unit_rd_aov0(g):
    """"aov" = 0 and calls that need no plane: accepted right after the restart; right behind a frame nobody waited for (a batching
    context holds it back); with an adaptive session open, which goes on.  Then "aov" on again: the third restart"""
    call = g.robust_denoise_needs()
    return [S("set_aov", mask=0), g.robust_denoise(planes=False), g.render(session=True, sync=False), g.robust_denoise(planes=False), g.adaptive_begin(), g.adaptive_frame(),
            g.robust_denoise(planes=False), g.adaptive_frame(), S("adaptive_update"), S("set_aov", mask=g.pick("restart_aov", (PLANES, ALL))), call,
            g.render(session=True), call]


def unit_rd_estimates(g):
    """between two estimates of the session, and between two of the image with the snapshot of the first still in use"""
    return [g.robust_error(), g.robust_denoise(), g.robust_error(), g.render(restart=True), g.error(keep_snapshot=False), g.render(), g.robust_denoise(),
            g.error(keep_snapshot=True)]


def unit_rd_resolve(g):
    """the resolve into the image leaves the planes and their count as they are: accepted right behind it, and behind the next frame"""
    call = g.robust_denoise_needs()
    return [g.resolve(1), call, g.render(session=True), call]


def unit_rd_second(g):
    """a second rtgl_robust_begin with a smaller K under a session that held more frames than that: refused at N = 0 and at N = K - 1,
    accepted at N = K; refused after rtgl_robust_end, the denoised and the variance buffer stay readable"""
    call = g.robust_denoise()
    return [S("robust_begin", buckets=4), call] + g.fill(4, probe=call) + [call, S("robust_end"), call]


UNITS = dict(source=unit_source, sweep=unit_sweep, ender_clear=unit_ender_clear, ender_render=unit_ender_render, ender_write=unit_ender("write_image"), ender_bind=unit_ender("bind_image"),
             ender_resolve=unit_ender("robust_resolve"), aov_adaptive=unit_aov_adaptive, robust_open=unit_robust_open, denoisers=unit_denoisers, temporal=unit_temporal,
             invalid=unit_invalid, tone=unit_tone, robust_image=unit_robust_image, moments=unit_moments, robust_twice=unit_robust_twice, epochs_a=unit_epochs_a,
             epochs_b=unit_epochs_b, epochs_c=unit_epochs_c,
             rd_open8=unit_rd_open(8, False), rd_open8_probe=unit_rd_open(8, True), rd_open16=unit_rd_open(16, False),
             rd_source=unit_rd_source, rd_pairs_a=unit_rd_pairs(False), rd_pairs_b=unit_rd_pairs(True), rd_restarts=unit_rd_restarts, rd_aov0=unit_rd_aov0,
             rd_estimates=unit_rd_estimates, rd_resolve=unit_rd_resolve, rd_second=unit_rd_second)
# fifteen rows, packed by hand to 24..40 steps: every unit twice ("invalid" and "sweep" once), "source" first where it occurs.  Seed s takes row
# s % 15.  The last six are rtgl_robust_denoise's: an "rd_open" first (a fill is K + 4 steps, so K = 16 takes more than half a row), then
# its units, each twice and at two sizes; K = 4 is "rd_second"'s
ROWS = [("source", "robust_image", "ender_write", "ender_clear"), ("robust_image", "denoisers", "ender_bind", "ender_resolve"),
        ("moments", "aov_adaptive", "temporal", "ender_write"), ("moments", "epochs_a", "epochs_b", "ender_bind"), ("epochs_c", "invalid", "robust_open", "ender_render"),
        ("aov_adaptive", "epochs_a", "robust_twice", "ender_render"), ("source", "temporal", "epochs_b", "tone"), ("epochs_c", "robust_open", "denoisers", "ender_clear"),
        ("robust_twice", "ender_resolve", "tone", "sweep"),
        ("rd_open8", "rd_source", "rd_aov0", "rd_resolve"), ("rd_open16", "rd_pairs_a", "rd_restarts"), ("rd_open8", "rd_source", "rd_estimates", "rd_pairs_b"),
        ("rd_open8_probe", "rd_estimates", "rd_second"), ("rd_open16", "rd_aov0", "rd_resolve"), ("rd_open8_probe", "rd_restarts", "rd_second")]


def size_of(seed):
    """five rows per size, and the two rows of a unit at different sizes where the packing allows"""
    row = seed % len(ROWS)
    return SIZES[(row + row // 3) % len(SIZES)]


def sequence(seed):
    seed = int(seed)
    g = _Gen(seed)
    W, H = size_of(seed)
    names = ROWS[seed % len(ROWS)]
    steps = []
    for n in names:
        steps += UNITS[n](g)
    assert MIN_STEPS <= len(steps) <= MAX_STEPS, (seed, names, len(steps))
    return Sequence(seed, W, H, scene(), base_params(), steps, names)


# ------------------------------------------------------------------------------------------------ the alphabet, as data

def _is(kind, **want):
    return lambda s: s.kind == kind and all(s.args.get(k) == v for k, v in want.items())


ALPHABET = ([(f"render reset_flag={r}", _is("render", reset_flag=r)) for r in (0, 1)] + [(f"render sync={v}", _is("render", sync=v)) for v in (True, False)]
            + [("render frames restarting", lambda s: s.kind == "render" and s.args["frames"] == 1 and s.args["reset_flag"] == 0),
               ("render frames counting", lambda s: s.kind == "render" and s.args["frames"] > 2),
               ("render camera moved", lambda s: s.kind == "render" and s.args["camera"] != 0),
               ("render refused for samples = 0", lambda s: s.kind == "render" and s.args.get("samples", 1) == 0)]
            + [(k, _is(k)) for k in ("write_image", "clear_image", "bind_image", "temporal_accumulate", "temporal_reset", "temporal_clip", "tonemap_reset", "error_reset",
                                     "adaptive_begin", "adaptive_frame", "adaptive_update", "adaptive_set_mask", "robust_accumulate", "robust_error_estimate", "robust_end")]
            + [(f"set_aov {m}", _is("set_aov", mask=m)) for m in AOV_MASKS]
            + [(f"set_option {k}={v}", _is("set_option", key=k, value=v)) for k, vs in (("denoise_source", (0, 1)), ("temporal_moments", (0, 1, 2)), ("denoise_variance", (0, 1))) for v in vs]
            + [(f"denoise passes={p}", _is("denoise", passes=p)) for p in PASSES] + [(f"denoise demodulate={v}", _is("denoise", demodulate=v)) for v in (True, False)]
            + [(f"denoise {k} {'on' if v else 'off'}", (lambda k, v: lambda s: s.kind == "denoise" and (s.args[k] > 0) == v)(k, v))
               for k in ("sigma_color", "sigma_normal", "sigma_position") for v in (True, False)]
            + [(f"denoise_guided passes={p}", _is("denoise_guided", passes=p)) for p in PASSES]
            + [(f"denoise_guided clamp {'on' if v else 'off'}", (lambda v: lambda s: s.kind == "denoise_guided" and (s.args["firefly_ratio"] > 0) == v)(v)) for v in (True, False)]
            + [(f"tonemap source={v}", _is("tonemap", source=v)) for v in (0, 1, 2)] + [(f"tonemap op={v}", _is("tonemap", op=v)) for v in (0, 1, 2)]
            + [(f"tonemap auto={v}", _is("tonemap", auto=v)) for v in (True, False)] + [("tonemap adapt below 1", lambda s: s.kind == "tonemap" and s.args["auto"] and s.args["adapt"] < 1)]
            + [(f"error_estimate keep_snapshot={v}", _is("error_estimate", keep_snapshot=v)) for v in (True, False)] + [("error_estimate first_frames=1", _is("error_estimate", first_frames=1))]
            + [(f"robust_begin K={k}", _is("robust_begin", buckets=k)) for k in BUCKETS]
            + [(f"robust_resolve dest={d} gain={v}", _is("robust_resolve", dest=d, gain=v)) for d in (0, 1) for v in (0.0, 1.0)]
            + [(f"robust_denoise passes={p}", _is("robust_denoise", passes=p)) for p in PASSES]
            + [(f"robust_denoise demodulate={v}", _is("robust_denoise", demodulate=v)) for v in (True, False)]
            + [(f"robust_denoise gain={v}", _is("robust_denoise", gain=v)) for v in (0.0, 1.0)]
            + [(f"robust_denoise {k} {'on' if v else 'off'}", (lambda k, v: lambda s: s.kind == "robust_denoise" and (s.args[k] > 0) == v)(k, v))
               for k in ("sigma_normal", "sigma_position") for v in (True, False)])


# ------------------------------------------------------------------------------------------------ the hazards, as data

def _denoiser_pairs(steps):
    d = [s for s in steps if s.kind in DENOISERS]
    return [(a, b) for a, b in zip(d, d[1:]) if a.kind != b.kind]


def _pair(first_passes, second_passes, first_kind=None):
    return lambda steps: any(a.args["passes"] == first_passes and b.args["passes"] == second_passes and first_kind in (None, a.kind) for a, b in _denoiser_pairs(steps))


def _tonemap_after(source, family, last):
    def pred(steps):
        seen = None
        for s in steps:
            if s.kind in family:
                seen = s.kind
            elif s.kind == "tonemap" and s.args["source"] == source and seen == last:
                return True
        return False
    return pred


def _source_one(after_temporal):
    def pred(steps):
        source, temporal = 0, False
        for s in steps:
            if s.kind == "set_option" and s.args["key"] == "denoise_source" and s.args["value"] in (0, 1):
                source = s.args["value"]
            temporal |= s.kind == "temporal_accumulate"
            if s.kind in DENOISERS and source == 1 and temporal == after_temporal:
                return True
        return False
    return pred


EPOCH_EVENTS = ("reset_frame", "write_image", "clear_image", "bind_image", "error_reset", "adaptive_begin", "adaptive_frame", "robust_resolve_image")


def epoch_event(s):
    """the name of the event of rtgl_error_estimate's epoch this step is, or None"""
    if s.kind == "render":
        return "reset_frame" if s.args["reset_flag"] else None
    if s.kind == "robust_resolve":
        return "robust_resolve_image" if s.args["dest"] == 1 else None
    return s.kind if s.kind in EPOCH_EVENTS else None


def _error_separated_by(event):
    def pred(steps):
        between = None
        for s in steps:
            if s.kind == "error_estimate" and s.args["first_frames"] == 1:
                if between is not None and (event in between if event else not between):
                    return True
                between = set()
            elif between is not None and epoch_event(s):
                between.add(epoch_event(s))
        return False
    return pred


def _restart(kind):
    def pred(steps):
        for i in range(len(steps) - 3):
            a, b, c, d = steps[i:i + 4]
            if a.kind == kind and b.kind in NEED_PLANES and c.kind == "render" and d.kind in NEED_PLANES:
                return True
        return False
    return pred


def _adaptive_frame_with_aov(steps):
    aov = 0
    for s in steps:
        if s.kind == "set_aov":
            aov = s.args["mask"]
        if s.kind == "adaptive_frame" and aov:
            return True
    return False


def ender_of(s):
    if s.kind == "render":
        return "render" if s.args.get("samples", 1) else None
    if s.kind == "robust_resolve":
        return "robust_resolve_image" if s.args["dest"] == 1 else None
    return s.kind if s.kind in ENDERS else None


def _ended_by(ender):
    def pred(steps):
        is_open, by = False, None
        for s in steps:
            if s.kind == "adaptive_begin" and s.args.get("min_samples", 1) >= 1:
                is_open, by = True, None
            elif ender_of(s) and is_open:
                is_open, by = False, ender_of(s)
            elif s.kind == "adaptive_update" and not is_open and by == ender:
                return True
        return False
    return pred


def _robust_open_across(what):
    def pred(steps):
        is_open, frames, session = False, 0, False
        for s in steps:
            if s.kind == "robust_begin" and s.args["buckets"] in BUCKETS:
                is_open, frames, session = True, 0, False
            elif s.kind == "robust_end":
                is_open = False
            elif is_open and s.kind == "render" and not s.args["reset_flag"]:
                frames += 1
            elif is_open and s.kind == "adaptive_frame":
                session = True
            elif is_open and s.kind == "robust_accumulate":
                if (session if what == "adaptive" else frames >= 2):
                    return True
        return False
    return pred


def _resolve_image_then(steps):
    for i, s in enumerate(steps):
        if s.kind == "robust_resolve" and s.args["dest"] == 1:
            after = [t.kind for t in steps[i + 1:i + 4]]
            if "error_estimate" in after and "tonemap" in after:
                return True
    return False


def _begin_twice(steps):
    k = None
    for s in steps:
        if s.kind == "robust_begin" and s.args["buckets"] in BUCKETS:
            if k is not None and k != s.args["buckets"]:
                return True
            k = s.args["buckets"]
        elif s.kind == "robust_end":
            k = None
    return False


def _tone_memory(steps):
    t = [("reset" if s.kind == "tonemap_reset" else "auto" if s.args["auto"] else "manual") for s in steps if s.kind in TONE]
    for i in range(len(t)):
        autos, seen = 0, set()
        for x in t[i:]:
            if x == "auto":
                autos += 1
                if autos == 3:
                    break
            elif autos:
                seen.add(x)
        if t[i] == "auto" and autos == 3 and seen == {"manual", "reset"}:
            return True
    return False


def _temporal_across(what):
    def pred(steps):
        aov = moments = 0
        called, changed = False, False
        for s in steps:
            if s.kind == "temporal_accumulate":
                if called and changed:
                    return True
                called, changed = True, False
            elif what == "normal" and s.kind == "set_aov":
                changed |= called and bool(s.args["mask"] & N) != bool(aov & N)
                aov = s.args["mask"]
            elif what == "moments" and s.kind == "set_option" and s.args["key"] == "temporal_moments" and s.args["value"] in (0, 1, 2):
                changed |= called and s.args["value"] != moments
                moments = s.args["value"]
        return False
    return pred


# rtgl_robust_denoise.  What a predicate has to know of the context it reads off the steps before the call, by the header's rules and on
# the assumption that every step with good arguments was accepted where only its arguments decide (the CPU test checks the statuses
# themselves against the model)

RdCall = namedtuple("RdCall", "i step prev full N K session need aov restarted source temporal adaptive ran prior")


def _rd_calls(steps):
    """every robust_denoise step with good arguments.  full: a session is open at N >= K.  need: the planes its parameters need.
    restarted: no frame since the planes restarted.  source: "denoise_source".  temporal: a temporal_accumulate came before.  adaptive: an
    adaptive session is open.  session: a counter of robust_begin and robust_end.  ran: a call was accepted earlier.  prior: (N, K) of
    the session a robust_begin right before the call replaced, or None"""
    out = []
    n = k = None
    session = aov = source = 0
    restarted, temporal, adaptive, ran, prior = True, False, False, False, None
    for i, s in enumerate(steps):
        a, before = s.args, prior
        prior = None
        if s.kind == "robust_begin" and a["buckets"] in BUCKETS:
            prior = (n, k) if k is not None else None
            n, k, session = 0, a["buckets"], session + 1
        elif s.kind == "robust_end" and k is not None:
            n, k, session = None, None, session + 1
        elif s.kind == "robust_accumulate" and k is not None:
            n += 1
        elif s.kind == "set_aov" and 0 <= a["mask"] <= 15:
            aov, restarted = a["mask"], True
        elif s.kind == "clear_image":
            restarted, adaptive = True, False
        elif s.kind == "adaptive_begin" and a["min_samples"] >= 1:
            restarted, adaptive = True, True
        elif ender_of(s):
            adaptive = False
            if s.kind == "render" and aov:
                restarted = False
        elif s.kind == "set_option" and a["key"] == "denoise_source" and a["value"] in (0, 1):
            source = a["value"]
        elif s.kind == "temporal_accumulate":
            temporal = True
        elif s.kind == "robust_denoise" and a["sigma_lum"] > 0 and a["passes"] <= 8:
            need = (A if a["demodulate"] else 0) | (N if a["sigma_normal"] > 0 else 0) | (P if a["sigma_position"] > 0 else 0)
            full = k is not None and n >= k
            out.append(RdCall(i, s, steps[i - 1] if i else None, full, n, k, session, need, aov, restarted, source, temporal, adaptive, ran, before))
            ran |= full and not need & ~aov and not (need and restarted)
    return out


def _rd_accepted(c):
    return c.full and not c.need & ~c.aov and not (c.need and c.restarted)


def _filter_pairs(steps):
    d = [s for s in steps if s.kind in FILTERS]
    return list(zip(d, d[1:]))


def _rd_pair(first, first_passes, second, second_passes):
    return lambda steps: any(a.kind == first and b.kind == second and a.args["passes"] in first_passes and b.args["passes"] in second_passes for a, b in _filter_pairs(steps))


def _rd_source_one(after_temporal):
    """accepted with "denoise_source" = 1: before any temporal call, where the two denoisers are refused; after one, with a denoise_guided
    behind it that takes the history"""
    def pred(steps):
        for c in _rd_calls(steps):
            if _rd_accepted(c) and c.source == 1 and c.temporal == after_temporal:
                later = [s for s in steps[c.i + 1:] if s.kind in FILTERS or (s.kind == "set_option" and s.args["key"] == "denoise_source")]
                if not after_temporal or (later and later[0].kind == "denoise_guided"):
                    return True
        return False
    return pred


def _rd_restart(kind):
    """refused for the planes and nothing else right after `kind`, and the same call accepted after one frame"""
    def pred(steps):
        calls = {c.i: c for c in _rd_calls(steps)}
        for i, c in calls.items():
            d = calls.get(i + 2)
            if (c.prev is not None and c.prev.kind == kind and c.full and c.need and not c.need & ~c.aov and c.restarted and d is not None and steps[i + 1].kind == "render"
                    and d.step is c.step and _rd_accepted(d)):
                return True
        return False
    return pred


def _rd_any(test):
    return lambda steps: any(test(c) for c in _rd_calls(steps))


def _rd_between(kind):
    """accepted between two calls of `kind` of which the second still stands on what the first left: robust_error_estimate in one
    session; error_estimate with no event of its epoch between, and a counting frame, so that the second uses the snapshot"""
    def pred(steps):
        open_, seen, frame = False, False, False
        calls = {c.i: c for c in _rd_calls(steps)}
        for i, s in enumerate(steps):
            if s.kind == kind:
                if open_ and seen and (frame or kind == "robust_error_estimate"):
                    return True
                open_, seen, frame = True, False, False
            elif s.kind in ("robust_begin", "robust_end") if kind == "robust_error_estimate" else epoch_event(s):
                open_ = False
            elif s.kind == "render":
                frame = True
            elif i in calls and _rd_accepted(calls[i]):
                seen = True
        return False
    return pred


def _rd_adaptive(steps):
    """accepted with an adaptive session open, then a masked frame and an update: the session goes on"""
    return any(_rd_accepted(c) and c.adaptive and c.aov == 0 and [s.kind for s in steps[c.i + 1:c.i + 3]] == ["adaptive_frame", "adaptive_update"] for c in _rd_calls(steps))


def _rd_short_then_full(steps):
    calls = _rd_calls(steps)
    return any(c.K is not None and 0 < c.N < c.K and any(d.session == c.session and _rd_accepted(d) for d in calls if d.i > c.i) for c in calls)


def _rd_second_begin(steps):
    """right after a second robust_begin with a K the old session's N would have satisfied, and again at N >= K"""
    calls = _rd_calls(steps)
    return any(c.prior is not None and c.prior[1] != c.K and c.prior[0] >= c.K and c.prev.kind == "robust_begin"
               and any(d.session == c.session and _rd_accepted(d) for d in calls if d.i > c.i) for c in calls)


def _rd_after_resolve(steps):
    """robust_resolve into the image, a frame, then a call that needs planes"""
    calls = {c.i: c for c in _rd_calls(steps)}
    for i, s in enumerate(steps):
        if s.kind == "robust_resolve" and s.args["dest"] == 1 and s.args["gain"] >= 0:
            after = steps[i + 1:i + 4]
            k = next((j for j, t in enumerate(after) if t.kind == "render"), None)
            c = calls.get(i + 2 + k) if k is not None else None
            if c is not None and c.need and _rd_accepted(c) and all(t.kind == "robust_denoise" for t in after[:k]):
                return True
    return False


RD_HAZARDS = ([("denoise_guided 5 passes then robust_denoise 0", _rd_pair("denoise_guided", (5,), "robust_denoise", (0,))),
               ("denoise_guided 0 or 1 passes then robust_denoise 5", _rd_pair("denoise_guided", (0, 1), "robust_denoise", (5,))),
               ("robust_denoise 5 passes then denoise_guided 0", _rd_pair("robust_denoise", (5,), "denoise_guided", (0,))),
               ("robust_denoise 0 or 1 passes then denoise_guided 5", _rd_pair("robust_denoise", (0, 1), "denoise_guided", (5,))),
               ("denoise after robust_denoise", _rd_pair("robust_denoise", PASSES, "denoise", tuple(range(9)))),
               ("robust_denoise with denoise_source 1 before any temporal call", _rd_source_one(False)),
               ("robust_denoise with denoise_source 1 after a temporal call, denoise_guided behind it", _rd_source_one(True))]
              + [(f"robust_denoise needing planes right after {k}, and after a frame", _rd_restart(k)) for k in RESTARTS]
              + [("robust_denoise needing no plane right after a restart with aov 0",
                  _rd_any(lambda c: _rd_accepted(c) and not c.need and c.aov == 0 and c.restarted and c.prev.kind in RESTARTS)),
                 ("robust_denoise between two robust_error_estimate calls", _rd_between("robust_error_estimate")),
                 ("robust_denoise between two error_estimate calls that share a snapshot", _rd_between("error_estimate")),
                 ("robust_denoise with an adaptive session open, which goes on", _rd_adaptive),
                 ("robust_denoise at 0 < N < K, and at N >= K", _rd_short_then_full),
                 ("robust_denoise after robust_end", _rd_any(lambda c: c.K is None and c.ran and c.prev.kind == "robust_end")),
                 ("robust_denoise right after a second robust_begin with a smaller K, and at N >= K", _rd_second_begin),
                 ("robust_denoise needing no plane behind a frame nobody waited for, aov 0",
                  _rd_any(lambda c: _rd_accepted(c) and not c.need and c.aov == 0 and c.prev.kind == "render" and not c.prev.args["sync"])),
                 ("robust_resolve into the image, a frame, then robust_denoise needing planes", _rd_after_resolve)])

HAZARDS = ([("denoisers 1 then 5 passes", _pair(1, 5)), ("guided 0 then plain 2 passes", _pair(0, 2, "denoise_guided")), ("denoisers 5 then 0 passes", _pair(5, 0)),
            ("plain then guided", lambda steps: any(a.kind == "denoise" for a, _ in _denoiser_pairs(steps))),
            ("guided then plain", lambda steps: any(a.kind == "denoise_guided" for a, _ in _denoiser_pairs(steps))),
            ("tonemap source 1 after denoise", _tonemap_after(1, FILTERS, "denoise")), ("tonemap source 1 after denoise_guided", _tonemap_after(1, FILTERS, "denoise_guided")),
            ("tonemap source 1 after robust_denoise", _tonemap_after(1, FILTERS, "robust_denoise")),
            ("tonemap source 2 after temporal_clip", _tonemap_after(2, ("temporal_accumulate", "temporal_clip"), "temporal_clip")),
            ("denoise_source 1 before any temporal call", _source_one(False)), ("denoise_source 1 after a temporal call", _source_one(True))]
           + [(f"error_estimate across {e}", _error_separated_by(e)) for e in EPOCH_EVENTS] + [("error_estimate across no event", _error_separated_by(None))]
           + [(f"a call that needs planes right after {k}, and after a frame", _restart(k)) for k in ("clear_image", "set_aov", "adaptive_begin")]
           + [("adaptive_frame with aov on", _adaptive_frame_with_aov)] + [(f"adaptive_update after the session was ended by {e}", _ended_by(e)) for e in ENDERS]
           + [("a robust session open across an adaptive session", _robust_open_across("adaptive")), ("a robust session open across ordinary frames", _robust_open_across("frames")),
              ("robust_resolve into the image, then error_estimate and tonemap", _resolve_image_then), ("robust_begin twice with different K", _begin_twice),
              ("three auto tonemaps with a manual call and a reset between", _tone_memory),
              ("temporal_accumulate across a change of the normal plane", _temporal_across("normal")),
              ("temporal_accumulate across a change of temporal_moments", _temporal_across("moments"))]
           + RD_HAZARDS)
