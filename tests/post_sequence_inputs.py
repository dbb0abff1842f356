"""Seeded call sequences over ONE context that cross the post-process features (include/rtgl_amd.h: both denoisers, the temporal calls, the
display transform, the error estimate, the adaptive, the robust and the robust adaptive session, the robust one with its estimate and
its denoiser) for
tests/post_sequence_model.py, the CPU test of this file and tests/test_gpu_post_sequences.py.  A helper, not a test; plain numpy and
Python, no device.

`sequence(seed)` returns a fixed scene (the mesh, spheres and cube map of the post-process tests, 4 bounces), one of three sizes and a
list of 24 to 40 steps.  A step is (kind, args); `frame_params` turns the args of a frame into its uniforms.  A sequence is a row of UNITS:
each unit is a short scripted stretch that sets up one or more of the named HAZARDS (a pair of calls of which the first writes host state
the second reads), with its parameters taken in turn from the alphabet's lists, starting at a place that depends on the seed.  The
twenty-four rows hold every unit twice -- nine rows for the calls up to rtgl_robust_error_estimate, six for rtgl_robust_denoise, whose
session has to be filled first, nine for the robust adaptive session, likewise -- so twenty-four consecutive seeds meet every hazard at
least twice and every alphabet entry at least once whatever the first seed is (tests/test_post_sequence_inputs.py counts them).  Steps
the contract refuses are wanted: a unit of the first nine rows does not look at what the units before it left behind, and several ask
for a refusal outright.

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
DEFAULT_SEQUENCES = 24
MIN_STEPS, MAX_STEPS = 24, 40
BOUNCES = 4
A, N, P, IDS, ALL = 1, 2, 4, 8, 15
AOV_MASKS = (0, P, N | P, A | N | P, ALL)
PASSES = (0, 1, 2, 5)
BUCKETS = (4, 8, 16)
MASKS = ("checker", "left", "none", "all")
RA_MASKS = ("checker", "odd", "left", "none", "all")                  # of the robust adaptive rows: "odd" is the checker's other half
CAMERAS = [ti.cam(), ti.cam((0.6, 0.2, -35.0)), ti.cam(yaw=0.03, pitch=0.01), ti.cam((1.0, 0.0, -33.0), yaw=-0.02)]
DENOISERS = ("denoise", "denoise_guided")
FILTERS = DENOISERS + ("robust_denoise",)                              # the writers of the denoised buffer
NEED_PLANES = DENOISERS + ("temporal_accumulate", "temporal_clip")
RESTARTS = ("clear_image", "set_aov", "adaptive_begin")                # the calls that restart the first-hit planes
TONE = ("tonemap", "tonemap_reset")
FEATURES = dict(denoise=("denoise",), denoise_guided=("denoise_guided",), temporal=("temporal_accumulate",), temporal_clip=("temporal_clip",),
                tonemap=("tonemap",), error=("error_estimate",), adaptive=("adaptive_begin", "adaptive_frame", "adaptive_update", "adaptive_set_mask"),
                robust=("robust_begin", "robust_accumulate", "robust_resolve", "robust_end"), robust_error=("robust_error_estimate",),
                robust_denoise=("robust_denoise",),
                robust_adaptive=("robust_adaptive_begin", "robust_adaptive_frame", "robust_adaptive_accumulate", "robust_adaptive_update", "robust_adaptive_set_mask",
                                 "robust_adaptive_resolve", "robust_adaptive_end"))
MASKED_FRAMES = ("adaptive_frame", "robust_adaptive_frame")


def default_seeds(n=DEFAULT_SEQUENCES, start=0):
    return list(range(int(start), int(start) + int(n)))


def scene():
    return sc.scene_mesh(10, 5, env_size=16)


def base_params():
    return sc.params_c2().replace(max_bounce=BOUNCES)


def frame_params(base, args):
    """the uniforms of a "render", "adaptive_frame" or "robust_adaptive_frame" step"""
    return base.replace(frames=args["frames"], reset_flag=args["reset_flag"], random=args["random"], samples=args.get("samples", 1), **CAMERAS[args["camera"]])


def written_image(h, w, k):
    """what a "write_image" step writes: positive, smooth, different per channel, alpha 1"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rgb = [0.5 + 0.4 * np.sin(0.21 * x + 0.9 * c + k) * np.cos(0.13 * y - 0.5 * c) for c in range(3)]
    return np.stack(rgb + [np.ones((h, w))], -1).astype(f32)


def mask_tiles(name, h, w):
    """the explicit mask of an "adaptive_set_mask" or "robust_adaptive_set_mask" step, (ty, tx) uint8"""
    ty, tx = (h + 15) // 16, (w + 15) // 16
    if name in ("checker", "odd"):
        return ((np.add.outer(np.arange(ty), np.arange(tx)) + (name == "odd")) % 2).astype(np.uint8)
    if name == "left":
        return np.repeat((np.arange(tx) < (tx + 1) // 2)[None, :], ty, 0).astype(np.uint8)
    return np.full((ty, tx), 1 if name == "all" else 0, np.uint8)


def resolved(seq, step):
    """the step with the arrays its args only name: the pixels of "write_image", the tiles of "adaptive_set_mask" and of
    "robust_adaptive_set_mask" """
    if step.kind == "write_image":
        return Step(step.kind, dict(step.args, pixels=written_image(seq.H, seq.W, step.args["image"])))
    if step.kind in ("adaptive_set_mask", "robust_adaptive_set_mask"):
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

    def ra_begin(self, K, **over):
        """min_samples = K and max_samples = K + 2: a tile with fewer than K samples stays active whatever it holds, one with K + 2 stops;
    between them the threshold decides, one of the two so small that no tile meets it"""
        args = dict(buckets=K, threshold=self.pick("rab_thr", (0.05, 0.002)), floor=0.01, gain=self.pick("rab_gain", (1.0, 0.0)), min_samples=K, max_samples=K + 2)
        args.update(over)
        return Step("robust_adaptive_begin", args)

    def ra_frame(self, **over):
        args = dict(frames=77, reset_flag=self.pick("raf_reset", (0, 1)), camera=self.camera, random=self.word(), sync=self.pick("sync", (True, False)))
        args.update(over)
        return Step("robust_adaptive_frame", args)

    def ra_resolve(self, dest, gain=None):
        return Step("robust_adaptive_resolve", dict(dest=dest, gain=self.pick("rar_gain", (1.0, 0.0)) if gain is None else gain))

    def ra_fill(self, K):
        """a robust adaptive session (begun by the caller, every tile active, "aov" 0) brought to n = K in every tile with buckets that
        differ: two masked frames, then two session frames each folded K / 2 - 1 times by rtgl_robust_adaptive_accumulate; nobody waits for
        the first of the two, so a batching context holds it back until the fold behind it"""
        return ([self.ra_frame(), self.ra_frame(), self.render(session=True, sync=False)] + [S("robust_adaptive_accumulate")] * (K // 2 - 1)
                + [self.render(session=True)] + [S("robust_adaptive_accumulate")] * (K // 2 - 1))

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


ENDERS = ("render", "clear_image", "write_image", "bind_image", "robust_resolve_image", "robust_adaptive_resolve_image")
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


# The units of the robust adaptive session.  All but "ra_open" count on what the "ra_open" at the head of their row leaves: "aov" 0, a
# session open with n >= K in every tile.  Each leaves "aov" 0 and no plain robust session behind; "ra_resolves" leaves a session of K = 4
# with counts that differ, "ra_end" none.

def ra_mask(name):
    return S("robust_adaptive_set_mask", mask=name)


def unit_ra_open(K, probe=True):
    """first in its row: a frame in the image, which the begin leaves alone; the fill; an update at n = K with buckets that differ.
    probe: a fold before the begin, refused"""
    def unit(g):
        return ([S("set_aov", mask=0), g.render()] + ([S("robust_adaptive_accumulate")] if probe else []) + [g.ra_begin(K)] + g.ra_fill(K) + [S("robust_adaptive_update")])
    return unit


def unit_ra_across_a(g):
    """the session open across an ordinary frame, rtgl_clear_image, rtgl_write_image_f32 and rtgl_bind_device_image, each with a call
    behind it that a session ended by mistake would refuse; the fold of a written image"""
    return [g.render(), S("robust_adaptive_update"), S("clear_image"), ra_mask("all"), g.ra_frame(), S("write_image", image=g.word() % 7), S("robust_adaptive_accumulate"),
            g.ra_resolve(0), S("bind_image"), S("robust_adaptive_update")]


def unit_ra_across_b(g):
    """across rtgl_adaptive_begin, rtgl_robust_resolve into the image and rtgl_robust_end; the fold of the image a masked frame of the
    adaptive session merged into, and of the one the plain session resolved into"""
    return [S("robust_begin", buckets=g.pick("rb_K", BUCKETS)), g.render(session=True), S("robust_accumulate"), g.adaptive_begin(), ra_mask("all"), g.ra_frame(),
            g.adaptive_frame(), S("robust_adaptive_accumulate"), g.resolve(1), S("robust_adaptive_accumulate"), S("robust_adaptive_update"), S("robust_end"), g.ra_resolve(0)]


def unit_ra_both(g):
    """an adaptive and a robust adaptive session side by side with masks and block counts that differ: a masked frame of each kind right
    behind a larger one of the other, a mask of each set between two frames of the other, an update of each.  The adaptive session's
    max_samples = 2 stops its checker tiles at the update whatever they hold"""
    return [g.adaptive_begin(min_samples=1, max_samples=2), ra_mask("odd"), g.adaptive_frame(), g.ra_frame(), S("adaptive_set_mask", mask="checker"), g.ra_frame(),
            ra_mask("all"), g.ra_frame(), g.adaptive_frame(), S("adaptive_update"), S("robust_adaptive_update")]


def unit_ra_image(g):
    """a masked frame between two estimates of the image that share a snapshot; the resolve into the image between two, the display
    transform and a denoiser of it, and the fold of it; rtgl_robust_denoise, which this session does not serve"""
    filt = g.denoise(planes=False) if g.pick("ra_filter", DENOISERS) == "denoise" else g.guided(planes=False)
    return [g.robust_denoise(planes=False), g.render(restart=True), g.error(keep_snapshot=False), g.render(), ra_mask("all"), g.ra_frame(), g.error(), g.render(), g.ra_resolve(1), g.error(), g.tonemap(0), filt,
            S("robust_adaptive_accumulate")]


def unit_ra_ender(g):
    """the resolve into the image ends an adaptive session"""
    return [g.adaptive_begin(), g.adaptive_frame(), g.ra_resolve(1), S("adaptive_update")]


def unit_ra_resolves(g):
    """the output readable and a mask set, then a second begin with K = 4 under a session of another K: the output is refused, every tile
    active; resolves into the buffer at N = 0 everywhere, under "checker" with N = 0 and 2, under "left" with N = 0, 2, 4 and 6 in one
    picture; an empty list and the resolve behind it; an update that stops the tiles at 6, keeps those below 4 and asks the records of the others"""
    return ([g.ra_resolve(0), ra_mask("odd"), g.ra_begin(4), g.ra_resolve(0), ra_mask("checker"), g.ra_frame(), g.ra_frame(), g.ra_resolve(0), ra_mask("left")]
            + [S("robust_adaptive_accumulate")] * 4 + [g.ra_resolve(0), ra_mask("none"), g.ra_frame(), g.ra_resolve(0), S("robust_adaptive_update")])


def unit_ra_plain(K):
    """rtgl_robust_denoise and rtgl_robust_error_estimate serve the plain session only: refused with the robust adaptive session alone,
    accepted on the planes of a plain session of another K beside it"""
    def unit(g):
        call, est = g.robust_denoise(planes=False), g.robust_error()
        return [call, est, S("robust_begin", buckets=K)] + g.fill(K, frames=2) + [call, est, S("robust_end")]
    return unit


def unit_ra_end(g):
    """rtgl_robust_adaptive_end with a plain session open, which goes on; then every call of the session, refused: for the state, and a
    resolve with dest = 2 for its argument"""
    return [S("robust_begin", buckets=4), g.render(session=True), S("robust_accumulate"), S("robust_adaptive_end"), g.ra_frame(), S("robust_adaptive_accumulate"),
            S("robust_adaptive_update"), ra_mask("all"), g.ra_resolve(0), g.ra_resolve(2), S("robust_adaptive_end"), g.resolve(0), S("robust_end")]


def unit_ra_aov(g):
    """a masked frame with "aov" on is refused for the state, with samples = 2 as well (the state comes first); with "aov" 0 again it is
    accepted although no frame has been rendered since the restart"""
    return [S("set_aov", mask=g.pick("restart_aov", (PLANES, ALL))), g.ra_frame(), g.ra_frame(samples=2), S("set_aov", mask=0), ra_mask("all"), g.ra_frame()]


def unit_ra_invalid(g):
    """bad arguments with the session open, which goes on: min_samples < K, a masked frame of either kind with samples = 2"""
    K = g.pick("rb_K", BUCKETS)
    return [g.ra_begin(K, min_samples=K - 1, max_samples=K), g.ra_frame(samples=2), S("robust_adaptive_update"), g.adaptive_begin(),
            Step("adaptive_frame", dict(g.adaptive_frame().args, samples=2)), S("adaptive_update")]


UNITS = dict(source=unit_source, sweep=unit_sweep, ender_clear=unit_ender_clear, ender_render=unit_ender_render, ender_write=unit_ender("write_image"), ender_bind=unit_ender("bind_image"),
             ender_resolve=unit_ender("robust_resolve"), aov_adaptive=unit_aov_adaptive, robust_open=unit_robust_open, denoisers=unit_denoisers, temporal=unit_temporal,
             invalid=unit_invalid, tone=unit_tone, robust_image=unit_robust_image, moments=unit_moments, robust_twice=unit_robust_twice, epochs_a=unit_epochs_a,
             epochs_b=unit_epochs_b, epochs_c=unit_epochs_c,
             rd_open8=unit_rd_open(8, False), rd_open8_probe=unit_rd_open(8, True), rd_open16=unit_rd_open(16, False),
             rd_source=unit_rd_source, rd_pairs_a=unit_rd_pairs(False), rd_pairs_b=unit_rd_pairs(True), rd_restarts=unit_rd_restarts, rd_aov0=unit_rd_aov0,
             rd_estimates=unit_rd_estimates, rd_resolve=unit_rd_resolve, rd_second=unit_rd_second,
             ra_open4=unit_ra_open(4), ra_open8=unit_ra_open(8), ra_open16=unit_ra_open(16, False), ra_across_a=unit_ra_across_a, ra_across_b=unit_ra_across_b, ra_both=unit_ra_both,
             ra_image=unit_ra_image, ra_ender=unit_ra_ender, ra_resolves=unit_ra_resolves, ra_plain4=unit_ra_plain(4), ra_end=unit_ra_end, ra_aov=unit_ra_aov,
             ra_invalid=unit_ra_invalid)
# twenty-four rows, packed by hand to 24..40 steps: every unit twice ("invalid" and "sweep" once), "source" first where it occurs.  Seed s takes row
# s % 24.  Rows 9 to 14 are rtgl_robust_denoise's: an "rd_open" first (a fill is K + 4 steps, so K = 16 takes more than half a row), then
# its units, each twice and at two sizes; K = 4 is "rd_second"'s
ROWS = [("source", "robust_image", "ender_write", "ender_clear"), ("robust_image", "denoisers", "ender_bind", "ender_resolve"),
        ("moments", "aov_adaptive", "temporal", "ender_write"), ("moments", "epochs_a", "epochs_b", "ender_bind"), ("epochs_c", "invalid", "robust_open", "ender_render"),
        ("aov_adaptive", "epochs_a", "robust_twice", "ender_render"), ("source", "temporal", "epochs_b", "tone"), ("epochs_c", "robust_open", "denoisers", "ender_clear"),
        ("robust_twice", "ender_resolve", "tone", "sweep"),
        ("rd_open8", "rd_source", "rd_aov0", "rd_resolve"), ("rd_open16", "rd_pairs_a", "rd_restarts"), ("rd_open8", "rd_source", "rd_estimates", "rd_pairs_b"),
        ("rd_open8_probe", "rd_estimates", "rd_second"), ("rd_open16", "rd_aov0", "rd_resolve"), ("rd_open8_probe", "rd_restarts", "rd_second"),
        # the robust adaptive session's: an "ra_open" first (K + 6 or K + 7 steps, so K = 16 takes more than half a row), then its units, each twice and at two
        # sizes; "ra_resolves" and "ra_plain4" under K = 8 and 16, whose K differs from theirs
        ("ra_open16", "ra_resolves"), ("ra_open4", "ra_across_a", "ra_across_b", "ra_invalid"), ("ra_open8", "ra_aov", "ra_resolves"),
        ("ra_open8", "ra_across_b", "ra_both"), ("ra_open8", "ra_across_a", "ra_image"), ("ra_open16", "ra_plain4", "ra_aov"),
        ("ra_open8", "ra_plain4", "ra_end"), ("ra_open4", "ra_both", "ra_image", "ra_ender"), ("ra_open4", "ra_aov", "ra_invalid", "ra_ender", "ra_end")]


def size_of(seed):
    """eight rows per size, and the two rows of a unit at different sizes where the packing allows"""
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
               for k in ("sigma_normal", "sigma_position") for v in (True, False)]
            + [(k, _is(k)) for k in ("robust_adaptive_accumulate", "robust_adaptive_update", "robust_adaptive_end")]
            + [(f"robust_adaptive_begin K={k}", _is("robust_adaptive_begin", buckets=k, min_samples=k)) for k in BUCKETS]
            + [("robust_adaptive_begin min_samples < K", lambda s: s.kind == "robust_adaptive_begin" and s.args["min_samples"] < s.args["buckets"])]
            + [(f"robust_adaptive_begin gain={v}", _is("robust_adaptive_begin", gain=v)) for v in (0.0, 1.0)]
            + [(f"robust_adaptive_begin threshold={v}", _is("robust_adaptive_begin", threshold=v)) for v in (0.05, 0.002)]
            + [(f"robust_adaptive_frame sync={v}", _is("robust_adaptive_frame", sync=v)) for v in (True, False)]
            + [(f"{k} samples=2", _is(k, samples=2)) for k in MASKED_FRAMES]
            + [(f"robust_adaptive_set_mask {m}", _is("robust_adaptive_set_mask", mask=m)) for m in RA_MASKS]
            + [(f"robust_adaptive_resolve dest={d} gain={v}", _is("robust_adaptive_resolve", dest=d, gain=v)) for d in (0, 1) for v in (0.0, 1.0)]
            + [("robust_adaptive_resolve dest=2", _is("robust_adaptive_resolve", dest=2))])


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


EPOCH_EVENTS = ("reset_frame", "write_image", "clear_image", "bind_image", "error_reset", "adaptive_begin", "adaptive_frame", "robust_resolve_image",
                "robust_adaptive_resolve_image")


def epoch_event(s):
    """the name of the event of rtgl_error_estimate's epoch this step is, or None"""
    if s.kind == "render":
        return "reset_frame" if s.args["reset_flag"] else None
    if s.kind in ("robust_resolve", "robust_adaptive_resolve"):
        return s.kind + "_image" if s.args["dest"] == 1 else None
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
    if s.kind in ("robust_resolve", "robust_adaptive_resolve"):
        return s.kind + "_image" if s.args["dest"] == 1 else None
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


# The robust adaptive session.  _ra_trace works out from the steps alone, by the header's rules, what every predicate below has to know of
# the context BEFORE each step, and the status of the steps whose acceptance the hazards speak of (RA_JUDGED; the CPU test holds these to
# the model).  The counts are kept per CLASS of tiles, (in "checker", in "left"): every named mask is a union of classes, so the counts
# are exact until an update sets the mask by its rule; from then on a class is known active below min_samples, known inactive from
# max_samples on, and unknown (None) between, and a fold under an unknown mask makes its count unknown.

CLASSES = ((0, 0), (0, 1), (1, 0), (1, 1))
RA_KINDS = FEATURES["robust_adaptive"]
RA_JUDGED = RA_KINDS + ("adaptive_frame", "robust_error_estimate", "robust_resolve")
RaStep = namedtuple("RaStep", "i step status aov restarted ad ad_mask ra K lo hi n mask buffer sid prior rb rb_K rb_N writer unsynced")


def _mask_classes(name):
    return {c: {"checker": c[0] == 1, "odd": c[0] == 0, "left": c[1] == 1, "none": False, "all": True}[name] for c in CLASSES}


def _known_size(mask):
    """the number of classes the mask holds, or None where a class is unknown"""
    return None if None in mask.values() else sum(mask.values())


def _ra_trace(steps):
    """[RaStep]: the state before every step and the status the header gives it (None for a kind that is not among RA_JUDGED).
    ad, ra, rb: an adaptive, a robust adaptive, a plain robust session is open.  n, mask: per class.  buffer: a resolve with dest BUFFER
    since the begin.  sid: a counter of begins and ends.  prior: (K, buffer) of the session a begin right before the step replaced.
    writer: the kind of the latest accepted writer of the image; unsynced: it was a frame nobody waited for."""
    out = []
    full = {c: True for c in CLASSES}
    aov, restarted, ad, ad_mask = 0, True, False, dict(full)
    ra, K, lo, hi, n, mask, buffer, sid, prior = False, None, None, None, {c: 0 for c in CLASSES}, dict(full), False, 0, None
    rb, rb_K, rb_N, writer, unsynced = False, None, 0, None, False
    for i, s in enumerate(steps):
        a, k, status, before = s.args, s.kind, None, prior
        prior = None
        if k == "robust_adaptive_begin":
            good = (a["buckets"] in BUCKETS and a["threshold"] > 0 and a["floor"] > 0 and a["gain"] >= 0 and a["buckets"] <= a["min_samples"] <= a["max_samples"] <= 1 << 24)
            status = 0 if good else -1
        elif k == "robust_adaptive_resolve":
            status = -1 if a["dest"] not in (0, 1) or not a["gain"] >= 0 else 0 if ra else -4
        elif k in MASKED_FRAMES:
            open_ = ra if k == "robust_adaptive_frame" else ad
            status = -4 if not open_ or aov else -1 if a.get("samples", 1) != 1 else 0
        elif k in RA_KINDS:
            status = 0 if ra else -4
        elif k == "robust_error_estimate":
            status = -1 if not (a["threshold"] > 0 and a["floor"] > 0 and a["gain"] >= 0) else 0 if rb and rb_N >= rb_K else -4
        elif k == "robust_resolve":
            status = -1 if a["dest"] not in (0, 1) or not a["gain"] >= 0 else 0 if rb and rb_N > 0 else -4
        out.append(RaStep(i, s, status, aov, restarted, ad, dict(ad_mask), ra, K, lo, hi, dict(n), dict(mask), buffer, sid, before, rb, rb_K, rb_N, writer, unsynced))
        if k in RA_JUDGED and status != 0:
            continue
        if k == "robust_adaptive_begin":
            prior = (K, buffer) if ra else None
            ra, K, lo, hi, n, mask, buffer, sid = True, a["buckets"], a["min_samples"], a["max_samples"], {c: 0 for c in CLASSES}, dict(full), False, sid + 1
        elif k == "robust_adaptive_end":
            ra, K, sid = False, None, sid + 1
        elif k in ("robust_adaptive_frame", "robust_adaptive_accumulate"):
            n = {c: None if mask[c] is None or n[c] is None else n[c] + mask[c] for c in CLASSES}
        elif k == "robust_adaptive_update":
            mask = {c: None if n[c] is None else True if n[c] < lo else False if n[c] >= hi else None for c in CLASSES}
        elif k == "robust_adaptive_set_mask":
            mask = _mask_classes(a["mask"])
        elif k == "robust_adaptive_resolve":
            buffer |= a["dest"] == 0
            if a["dest"] == 1:
                ad, writer, unsynced = False, "robust_adaptive_resolve_image", False
        elif k == "adaptive_frame":
            writer, unsynced = k, False
        elif k == "robust_resolve":
            if a["dest"] == 1:
                ad, writer, unsynced = False, "robust_resolve_image", False
        elif k == "robust_begin" and a["buckets"] in BUCKETS:
            rb, rb_K, rb_N = True, a["buckets"], 0
        elif k == "robust_accumulate" and rb:
            rb_N += 1
        elif k == "robust_end":
            rb = False
        elif k == "set_aov" and 0 <= a["mask"] <= 15:
            aov, restarted = a["mask"], True
        elif k == "adaptive_begin" and a["min_samples"] >= 1:
            ad, ad_mask, restarted, writer, unsynced = True, dict(full), True, k, False
        elif k == "adaptive_set_mask" and ad:
            ad_mask = _mask_classes(a["mask"])
        elif k == "adaptive_update" and ad:
            ad_mask = {c: None for c in CLASSES}
        elif k == "render" and a.get("samples", 1):
            ad, writer, unsynced = False, k, not a["sync"]
            restarted &= not aov
        elif k in ("clear_image", "write_image", "bind_image"):
            ad = False
            restarted |= k == "clear_image"
            if k != "bind_image":
                writer, unsynced = k, False
    return out


def _ra_ok(t):
    return t.status == 0


def _ra_update_full(K):
    """an accepted update with n >= K in some class whose buckets differ: the fill folds more than one source"""
    def pred(steps):
        sources = 0
        for t in _ra_trace(steps):
            if t.step.kind == "robust_adaptive_begin" and _ra_ok(t):
                sources = 0
            elif t.step.kind == "robust_adaptive_frame" and _ra_ok(t) or (t.step.kind == "render" and t.ra):
                sources += 1
            elif t.step.kind == "robust_adaptive_update" and _ra_ok(t) and t.K == K and sources >= 2 and any(v is not None and v >= K for v in t.n.values()):
                return True
        return False
    return pred


def _ra_event(t):
    """the name of the event of an adaptive session or of the plain robust one that this step is for an open robust adaptive session"""
    s = t.step
    if s.kind in ("adaptive_begin", "robust_end"):
        return s.kind
    if s.kind == "robust_resolve":
        return "robust_resolve_image" if _ra_ok(t) and s.args["dest"] == 1 else None
    return ender_of(s) if s.kind != "robust_adaptive_resolve" else None


RA_ACROSS = ("render", "clear_image", "write_image", "bind_image", "adaptive_begin", "robust_resolve_image", "robust_end")
RA_PROOFS = ("robust_adaptive_update", "robust_adaptive_frame", "robust_adaptive_resolve")


def _ra_open_across(event):
    """the session open across the event, and within three steps a call accepted that a session ended by mistake would refuse"""
    def pred(steps):
        tr = _ra_trace(steps)
        return any(t.ra and _ra_event(t) == event and any(u.step.kind in RA_PROOFS and _ra_ok(u) and u.sid == t.sid for u in tr[t.i + 1:t.i + 4]) for t in tr)
    return pred


def _ra_pairs(tr):
    """(first, second): accepted masked frames of different kinds at consecutive steps, both sessions open, their masks' sizes known"""
    for t, u in zip(tr, tr[1:]):
        if {t.step.kind, u.step.kind} == set(MASKED_FRAMES) and _ra_ok(t) and _ra_ok(u) and t.ra and t.ad:
            size = lambda v: _known_size(v.mask if v.step.kind == "robust_adaptive_frame" else v.ad_mask)
            if size(t) is not None and size(u) is not None:
                yield t, u, size(t), size(u)


def _ra_behind_larger(kind):
    """a masked frame of `kind` right behind a larger one of the other kind, the two masks differing; later an update of each session"""
    def pred(steps):
        tr = _ra_trace(steps)
        for t, u, a, b in _ra_pairs(tr):
            later = [v.step.kind for v in tr[u.i + 1:] if _ra_ok(v) or (v.step.kind == "adaptive_update" and v.ad)]
            if u.step.kind == kind and a > b and u.mask != u.ad_mask and "adaptive_update" in later and "robust_adaptive_update" in later:
                return True
        return False
    return pred


def _ra_mask_between(setter, frame):
    """`setter` accepted between two accepted `frame` calls, both sessions open throughout"""
    def pred(steps):
        first = seen = False
        for t in _ra_trace(steps):
            if not (t.ra and t.ad):
                first = seen = False
            elif t.step.kind == frame and _ra_ok(t):
                if first and seen:
                    return True
                first, seen = True, False
            elif t.step.kind == setter and first:
                seen = True
        return False
    return pred


def _ra_accumulate_after(writer, unsynced=False):
    return lambda steps: any(t.step.kind == "robust_adaptive_accumulate" and _ra_ok(t) and t.writer == writer and (t.unsynced and t.aov == 0 and t.i and steps[t.i - 1].kind == "render"
                                                                                                                 if unsynced else True) for t in _ra_trace(steps))


def _ra_between_errors(kind, event):
    """an accepted step of `kind` between two error_estimate calls with (event) or without (None) an event of the epoch between them,
    and a counted frame, so that the second one would use the snapshot if it were there"""
    def pred(steps):
        open_, seen, frame, events = False, False, False, set()
        for t in _ra_trace(steps):
            s = t.step
            if s.kind == "error_estimate" and s.args["first_frames"] == 1:
                if open_ and seen and frame and events == ({event} if event else set()):
                    return True
                open_, seen, frame, events = True, False, False, set()
            elif s.kind == kind and _ra_ok(t) and (event is None or epoch_event(s) == event):
                seen = True
                events |= {event} if event else set()
            elif epoch_event(s):
                events.add(epoch_event(s))
            elif s.kind == "render":
                frame = True
        return False
    return pred


def _ra_resolve_image_then(steps):
    """robust_adaptive_resolve into the image, then tonemap source 0 and a denoiser before anything else writes the image"""
    tr = _ra_trace(steps)
    for t in tr:
        if t.step.kind == "robust_adaptive_resolve" and _ra_ok(t) and t.step.args["dest"] == 1:
            after = [u.step for u in tr[t.i + 1:t.i + 5] if u.writer == "robust_adaptive_resolve_image"]
            if any(s.kind == "tonemap" and s.args["source"] == 0 for s in after) and any(s.kind in DENOISERS for s in after):
                return True
    return False


def _ra_resolve_buffer(want, mask):
    """an accepted resolve into the buffer with the mask last set by name to `mask` ("full": by the begin) and the counts as `want` says"""
    def pred(steps):
        named = None
        for t in _ra_trace(steps):
            if t.step.kind == "robust_adaptive_begin" and _ra_ok(t):
                named = "full"
            elif t.step.kind == "robust_adaptive_set_mask" and _ra_ok(t):
                named = t.step.args["mask"]
            elif t.step.kind == "robust_adaptive_update" and _ra_ok(t):
                named = None
            elif t.step.kind == "robust_adaptive_resolve" and _ra_ok(t) and t.step.args["dest"] == 0 and named == mask and None not in t.n.values() and want(set(t.n.values()), t.K):
                return True
        return False
    return pred


def _ra_plain_only(kind, both):
    """both False: `kind` refused for the state with a robust adaptive session that holds K samples open and no plain one.  both True:
    accepted with a plain session of another K open beside it"""
    def pred(steps):
        tr = _ra_trace(steps)
        rd = {c.i: c for c in _rd_calls(steps)}
        for t in tr:
            if t.step.kind != kind or not t.ra or any(v is None or v < t.K for v in t.n.values()):
                continue
            accepted = _rd_accepted(rd[t.i]) if kind == "robust_denoise" and t.i in rd else t.status == 0
            if (both and t.rb and t.rb_K != t.K and accepted) or (not both and not t.rb and kind == "robust_denoise" and t.i in rd and not accepted) or (
                    not both and not t.rb and t.status == -4):
                return True
        return False
    return pred


def _ra_resolve_ends_adaptive(steps):
    """robust_adaptive_resolve into the image accepted with an adaptive session open; then adaptive_update before any new adaptive_begin,
    refused: no adaptive session is open any more"""
    ended = False
    for t in _ra_trace(steps):
        if t.step.kind == "robust_adaptive_resolve" and _ra_ok(t) and t.step.args["dest"] == 1 and t.ad:
            ended = True
        elif t.ad:
            ended = False
        elif ended and t.step.kind == "adaptive_update":
            return True
    return False


def _ra_second_begin(steps):
    """a begin with another K under a session whose output was readable; then in the new session a frame, an update and a resolve"""
    tr = _ra_trace(steps)
    for t in tr:
        if t.prior is not None and t.prior[1] and t.prior[0] != t.K and not t.buffer and tr[t.i - 1].step.kind == "robust_adaptive_begin":
            later = {u.step.kind for u in tr[t.i:] if u.sid == t.sid and _ra_ok(u)}
            if set(RA_PROOFS) <= later:
                return True
    return False


def _ra_aov(steps):
    """a masked frame refused for "aov"; after set_aov 0 accepted with no frame since the planes restarted"""
    tr = _ra_trace(steps)
    refused = [t.i for t in tr if t.step.kind == "robust_adaptive_frame" and t.ra and t.aov and t.status == -4]
    return any(t.step.kind == "robust_adaptive_frame" and _ra_ok(t) and t.restarted and any(i < t.i for i in refused) for t in tr)


def _ra_after_end(kind):
    def pred(steps):
        ended = False
        for t in _ra_trace(steps):
            if t.step.kind == "robust_adaptive_end" and _ra_ok(t):
                ended = True
            elif t.step.kind == "robust_adaptive_begin" and _ra_ok(t):
                ended = False
            if ended and t.step.kind == kind and t.status == -4 and not t.aov:
                return True
        return False
    return pred


def _ra_two_samples(kind):
    """refused for samples = 2 in an open session with "aov" 0, and the session goes on: its update is accepted"""
    def pred(steps):
        tr = _ra_trace(steps)
        update = "robust_adaptive_update" if kind == "robust_adaptive_frame" else "adaptive_update"
        open_ = lambda v: v.ra if kind == "robust_adaptive_frame" else v.ad
        return any(t.step.kind == kind and t.status == -1 and tr[t.i + 1].step.kind == update and open_(tr[t.i + 1]) for t in tr[:-1])
    return pred


RA_HAZARDS = ([(f"robust_adaptive_update at n >= K = {k} with buckets that differ", _ra_update_full(k)) for k in BUCKETS]
              + [(f"a robust adaptive session open across {e}, then a call that proves it", _ra_open_across(e)) for e in RA_ACROSS]
              + [(f"{k} right behind a larger masked frame of the other kind, then an update of each", _ra_behind_larger(k)) for k in MASKED_FRAMES]
              + [("adaptive_set_mask between two robust_adaptive_frame calls", _ra_mask_between("adaptive_set_mask", "robust_adaptive_frame")),
                 ("robust_adaptive_set_mask between two adaptive_frame calls", _ra_mask_between("robust_adaptive_set_mask", "adaptive_frame"))]
              + [(f"robust_adaptive_accumulate after {w}", _ra_accumulate_after(w)) for w in ("render", "write_image", "adaptive_frame", "robust_resolve_image", "robust_adaptive_resolve_image")]
              + [("robust_adaptive_accumulate right behind a frame nobody waited for, aov 0", _ra_accumulate_after("render", True)),
                 ("robust_adaptive_resolve into the image between two error_estimate calls", _ra_between_errors("robust_adaptive_resolve", "robust_adaptive_resolve_image")),
                 ("robust_adaptive_frame between two error_estimate calls that share a snapshot", _ra_between_errors("robust_adaptive_frame", None)),
                 ("robust_adaptive_resolve into the image, then tonemap source 0 and a denoiser", _ra_resolve_image_then),
                 ("robust_adaptive_resolve into the image with an adaptive session open, then adaptive_update refused", _ra_resolve_ends_adaptive),
                 ("robust_adaptive_resolve into the buffer at N = 0 everywhere", _ra_resolve_buffer(lambda n, K: n == {0}, "full")),
                 ("robust_adaptive_resolve into the buffer under checker, N = 0 and 0 < N < K", _ra_resolve_buffer(lambda n, K: 0 in n and any(0 < v < K for v in n), "checker")),
                 ("robust_adaptive_resolve into the buffer under left, N = 0, 0 < N < K and N >= K in one picture",
                  _ra_resolve_buffer(lambda n, K: 0 in n and any(0 < v < K for v in n) and any(v >= K for v in n), "left")),
                 ("robust_adaptive_resolve into the buffer under none", _ra_resolve_buffer(lambda n, K: True, "none"))]
              + [(f"{k} with only a robust adaptive session open", _ra_plain_only(k, False)) for k in ("robust_denoise", "robust_error_estimate")]
              + [(f"{k} with a plain and a robust adaptive session of different K open", _ra_plain_only(k, True)) for k in ("robust_denoise", "robust_error_estimate")]
              + [("a second robust_adaptive_begin with another K: the output refused, then frame, update and resolve", _ra_second_begin),
                 ("robust_adaptive_frame with aov on, and accepted after set_aov 0 while the planes count as restarted", _ra_aov)]
              + [(f"{k} after robust_adaptive_end", _ra_after_end(k)) for k in RA_KINDS if k != "robust_adaptive_begin"]
              + [("robust_adaptive_begin with min_samples < K", lambda steps: any(t.step.kind == "robust_adaptive_begin" and t.status == -1 and t.step.args["min_samples"] < t.step.args["buckets"]
                                                                                 for t in _ra_trace(steps)))]
              + [(f"{k} with samples = 2 in an open session, which goes on", _ra_two_samples(k)) for k in MASKED_FRAMES])

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
           + RD_HAZARDS + RA_HAZARDS)
