"""Options "temporal_moments" and "denoise_variance" on the device (include/rtgl_amd.h, "temporal luminance moments").

The reference is the numpy restatement, tests/temporal_moments_mirror.py, pinned by tests/test_temporal_moments_mirror.py.  The comparison
rule is that of tests/test_gpu_temporal.py: where the mirror's component is not a NaN the kernel's has the same bits, no tolerance; where it
is a NaN, any NaN will do.  The mirror's NaN share is held to temporal_moments_inputs.nan_budget, so the rule cannot hide a failure.
Injected sequences, the guided call over their histories, rendered sequences, the host path, the frame path left alone, and the point of
it: the history filtered with its own variance is closer to the converged image than the history."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as gc
import raytracer_glsl_amd
import temporal_mirror as tm
import temporal_moments_inputs as mi
import temporal_moments_mirror as mm
from test_gpu_denoise import (ALBEDO, ALL, ERR_INVALID, ERR_STATE, GUIDES, IDS, MIRROR_CASES, NORMAL, POSITION, _DeviceArray, bits, c2, differing, golden_path,
                              named_case, same)
from test_gpu_denoise_guided import check as check_guided
from test_gpu_denoise_inputs import inject, prepared
from test_gpu_temporal import look, own_frames, raw_temporal
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def check(got, want, budget, label):
    """got, want: one array (a history, a moments buffer): the rule above"""
    nan = np.isnan(want)
    share = float(nan.mean())
    assert share <= budget, f"{label}: {share:.4%} of the mirror's components are NaN, budget {budget:.0%}"
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} components differ ({int((bad & nan).sum())} of them not NaN where the mirror is), "
                           f"first at (row, column, channel) {list(zip(*np.nonzero(bad)))[:8]}")


def step(rt, ctx, item, ps):
    """one call on injected arrays: (history, moments or None)"""
    image, normal, position, camera, albedo = item
    inject(ctx, image, albedo, normal, position)
    ctx.set_params(look(rt, camera))
    ctx.temporal_accumulate(**ps)
    return ctx.read_temporal(), (ctx.read_temporal_moments() if ctx.get_option("temporal_moments") else None)


def run_sequence(rt, ctx, seq, ps, mode, label, budget=0.0, plain=None):
    """the sequence from a reset on with the option at `mode`, every call's history and moments against the mirror (and the history against
    `plain`, the histories of the same calls with the option off); returns the mirror's results"""
    want = mm.run(seq, mode, **ps)
    ctx.set_option("temporal_moments", mode)
    ctx.temporal_reset()
    for k, item in enumerate(seq):
        h, m = step(rt, ctx, item, ps)
        check(h, want[k][0], budget, f"{label} {ps} mode {mode} call {k}: history")
        check(m, want[k][1], budget, f"{label} {ps} mode {mode} call {k}: moments")
        if plain is not None:
            nan = np.isnan(plain[k])
            assert not np.where(nan, ~np.isnan(h), bits(h) != bits(plain[k])).any(), f"{label} {ps} mode {mode} call {k}: the option changed the history"
    return want


def run_plain(rt, ctx, seq, ps):
    ctx.set_option("temporal_moments", 0)
    ctx.temporal_reset()
    return [step(rt, ctx, item, ps)[0] for item in seq]


# ---------------------------------------------------------------------------------------------- 1. injected sequences

@pytest.mark.parametrize("size", mi.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", sorted(mi.FAMILIES))
def test_injected_sequences_are_bit_identical_to_the_mirror(family, size, rt):
    """every family x every parameter set x modes 1 and 2, at the sizes about the 64 x 4 block tile (1 x 1 up to 200 x 131: the smallest
    shapes at which edge lanes, partial tiles and the taps at -1 can go wrong); moments and history after every call; the history with the
    option on is the history with it off"""
    W, H = size
    ctx = prepared(rt, W, H)
    seq = mi.make(family, H, W)
    for ps in mi.PARAMETER_SETS:
        plain = run_plain(rt, ctx, seq, ps)
        for mode in mi.MODES:
            assert (family, size, ps, mode) in mi.listed_cases()
            run_sequence(rt, ctx, seq, ps, mode, f"{family} {W} x {H}", mi.nan_budget(family), plain)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. the guided call over those histories

COMBINATIONS = [(mode, ratio) for mode in mi.MODES for ratio in (1.0, 0.0)]       # demodulation on with mode 2, off with mode 1; clamp on and off
# one case per family and size, all four combinations in it; above 10,000 pixels (where the mirror's five passes take half a second) one
# case per combination, so that no case takes more than a few seconds
GUIDED_CASES = [(f, size, combos) for f in sorted(mi.FAMILIES) for size in mi.SIZES
                for combos in ([[c] for c in COMBINATIONS] if size[0] * size[1] > 10000 else [COMBINATIONS])]


@pytest.mark.parametrize("family,size,combinations", GUIDED_CASES,
                         ids=[f"{f}-{s[0]}x{s[1]}" + ("" if len(c) > 1 else f"-mode{c[0][0]}-ratio{c[0][1]:g}") for f, s, c in GUIDED_CASES])
def test_guided_call_with_the_temporal_variance_is_bit_identical_to_the_mirror(family, size, combinations, rt):
    """"denoise_variance" = 1 over the history after the last call of every sequence and parameter set: passes 0 / 1 / 5, demodulation on
    with mode 2 and off with mode 1, clamp on and off; the image and all four components of the variance buffer"""
    W, H = size
    ctx = prepared(rt, W, H)
    seq = mi.make(family, H, W)
    image, normal, position, _, albedo = seq[-1]
    ctx.set_option("denoise_source", 1)
    ctx.set_option("denoise_variance", 1)
    for mode in sorted({m for m, _ in combinations}):
        ctx.set_option("temporal_moments", mode)
        for ps in mi.PARAMETER_SETS:
            ctx.temporal_reset()
            for item in seq:
                step(rt, ctx, item, ps)
            h, m = mm.run(seq, mode, **ps)[-1]
            for ratio in [r for m_, r in combinations if m_ == mode]:
                want = mm.denoise_guided_tvar_each(h, m, albedo, normal, position, passes_list=(0, 1, 5), firefly_ratio=ratio, demodulate=mode == 2)
                for passes in (0, 1, 5):
                    ctx.denoise_guided(passes=passes, firefly_ratio=ratio, demodulate=mode == 2)
                    check_guided((ctx.read_denoised(), ctx.read_denoise_variance()), want[passes], mi.nan_budget(family),
                                 f"{family} {W} x {H} {ps} mode {mode} ratio {ratio} passes {passes}")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. rendered sequences

def context_arrays(ctx):
    return ctx.read_image(), ctx.read_aov(NORMAL), ctx.read_aov(POSITION), ctx.read_aov(ALBEDO)


@pytest.mark.parametrize("kernel", [0, 4])
@pytest.mark.parametrize("name", ["camera_moved", "mesh_env_dof", "c1_256"])
def test_rendered_sequences_are_bit_identical_to_the_mirror(name, kernel, rt):
    """six frames, the camera rests, moves, rests; the arrays are read from the context before each call; both modes, and the guided call
    over the last history"""
    case, scene, W, H = named_case(rt, name)
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", kernel)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.set_option("denoise_source", 1)
    ctx.set_option("denoise_variance", 1)
    for mode in mi.MODES:
        ctx.set_option("temporal_moments", mode)
        state = None
        for k, p in enumerate(own_frames(rt, case["frames"][0], (0, 0, 1, 2, 2, 2))):
            ctx.render(p)
            image, normal, position, albedo = context_arrays(ctx)
            ctx.temporal_accumulate()
            state = mm.accumulate(state, image, normal, position, p, albedo, mode, **tm.DEFAULTS)
            check(ctx.read_temporal(), state["H"], 0.0, f"{name}, kernel {kernel}, mode {mode}, frame {k}: history")
            check(ctx.read_temporal_moments(), state["M"], 0.0, f"{name}, kernel {kernel}, mode {mode}, frame {k}: moments")
        assert (state["M"][..., 3] >= 4).any() and (state["M"][..., 3] < 4).any(), "both sides of the select are wanted"
        ctx.denoise_guided(demodulate=mode == 2)
        want = mm.denoise_guided_tvar(state["H"], state["M"], albedo, normal, position, demodulate=mode == 2)
        check_guided((ctx.read_denoised(), ctx.read_denoise_variance()), want, 0.0, f"{name}, kernel {kernel}, mode {mode}: guided")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. host path

def test_errors_and_state(rt):
    sc = rt.scenes
    W, H = 64, 64
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 4)
    buf = np.zeros((H, W, 4), np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    ctx = rt.host.Context(W, H)
    lib = ctx.lib
    ctx.upload_scene(scene)
    # the options: defaults, values
    assert ctx.get_option("temporal_moments") == 0 and ctx.get_option("denoise_variance") == 0
    for bad in (3, -1, 256):
        assert lib.rtgl_set_option(ctx.h, b"temporal_moments", bad) == ERR_INVALID
    for bad in (2, -1):
        assert lib.rtgl_set_option(ctx.h, b"denoise_variance", bad) == ERR_INVALID
    assert ctx.get_option("temporal_moments") == 0 and ctx.get_option("denoise_variance") == 0
    # read-out before the first call
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == ERR_STATE and b"temporal_moments" in lib.rtgl_last_error(ctx.h)
    assert ctx.device_temporal_moments_ptr() == 0
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_read_temporal_moments_f32(None, ptr) == ERR_INVALID and lib.rtgl_device_temporal_moments(None) is None
    # mode 2 needs the albedo plane
    ctx.set_aov(NORMAL | POSITION)
    ctx.render(frames[0])
    ctx.set_option("temporal_moments", 2)
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE and b"albedo" in lib.rtgl_last_error(ctx.h)
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_moments_ptr() == 0
    # a call with the option off stores none; with it on the read-out works; off again: none
    ctx.set_option("temporal_moments", 0)
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_moments_ptr() == 0
    ctx.set_option("temporal_moments", 1)
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == 0 and ctx.device_temporal_moments_ptr() != 0
    assert (buf[..., 3] == 1).all(), "a change of the option drops the history"
    # a call that fails leaves what the latest successful one stored
    assert raw_temporal(ctx, max_history=0.0) == ERR_INVALID
    assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == 0
    # the guided call
    ctx.set_option("denoise_variance", 1)
    assert ctx.get_option("denoise_variance") == 1
    with pytest.raises(rt.host.RtglError):
        ctx.denoise_guided(demodulate=False)                               # (the albedo plane is off: only a call that does not demodulate gets this far)
    assert b"denoise_source" in lib.rtgl_last_error(ctx.h)
    ctx.set_option("denoise_source", 1)
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE, "albedo is off: the default call demodulates"
    with pytest.raises(rt.host.RtglError):
        ctx.denoise_guided(demodulate=False, sigma_lum=0.0)
    ctx.denoise_guided(demodulate=False)                                   # mode 1, no demodulation: fine
    ctx.denoise(demodulate=False)                                          # rtgl_denoise ignores the option
    ctx.set_aov(GUIDES)
    ctx.render(frames[1])
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE and b"temporal_moments" in lib.rtgl_last_error(ctx.h), "mode 1 stored, the call demodulates"
    ctx.set_option("temporal_moments", 2)
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    assert lib.rtgl_denoise_guided(ctx.h, None) == 0
    with pytest.raises(rt.host.RtglError):
        ctx.denoise_guided(demodulate=False)                               # mode 2 stored, the call does not demodulate
    ctx.set_option("temporal_moments", 0)
    assert lib.rtgl_denoise_guided(ctx.h, None) == 0, "the option alone changes nothing: the latest call stored mode 2"
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE and b"stored no moments" in lib.rtgl_last_error(ctx.h)
    ctx.set_option("denoise_variance", 0)
    assert lib.rtgl_denoise_guided(ctx.h, None) == 0
    ctx.close()
    # tiled and multi-device contexts: the options are accepted, the calls stay out of scope
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(W, H, **kw)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.set_option("temporal_moments", 1)
        assert ctx.get_option("temporal_moments") == 1
        ctx.render(frames[0])
        assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        assert lib.rtgl_read_temporal_moments_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_moments_ptr() == 0
        ctx.close()


def test_option_change_means_reset_and_the_pointer_alternates(rt):
    import torch
    W, H = 70, 53
    seq = mi.make("translate", H, W)
    ctx = prepared(rt, W, H)
    # a change in mid-sequence, both ways, against the mirror; the same value again changes nothing
    for a, b in ((1, 2), (2, 1), (1, 1)):
        want = mm.run(seq[:2] + [mm.option(b)] + seq[2:], a)
        ctx.set_option("temporal_moments", a)
        ctx.temporal_reset()
        ptrs = []
        for k, item in enumerate(seq):
            if k == 2:
                before = ctx.read_temporal_moments()
                ctx.set_option("temporal_moments", b)
                assert same(ctx.read_temporal_moments(), before), "setting the option leaves the latest buffer readable"
            h, m = step(rt, ctx, item, dict())
            check(h, want[k][0], 0.0, f"{a} -> {b}, call {k}: history")
            check(m, want[k][1], 0.0, f"{a} -> {b}, call {k}: moments")
            if k == 2:
                assert ((h[..., 3] == 1).all()) == (a != b)
            ptrs.append(ctx.device_temporal_moments_ptr())
            t = torch.as_tensor(_DeviceArray(ptrs[-1], (H, W, 4), "<f4"), device="cuda:0")
            torch.cuda.synchronize()
            assert same(t.cpu().numpy(), m), "the pointer does not name the latest result"
        assert len(set(ptrs)) == 2 and all(p != q for p, q in zip(ptrs, ptrs[1:])), "the two buffers do not take turns"
    # 0 -> 1 and 1 -> 0 drop the history as well
    ctx.set_option("temporal_moments", 0)
    ctx.temporal_reset()
    step(rt, ctx, seq[0], dict())
    assert (step(rt, ctx, seq[1], dict())[0][..., 3] > 1).any()
    ctx.set_option("temporal_moments", 1)
    h, m = step(rt, ctx, seq[2], dict())
    assert (h[..., 3] == 1).all() and (m[..., 3] == 1).all()
    assert (step(rt, ctx, seq[3], dict())[0][..., 3] > 1).any()
    ctx.set_option("temporal_moments", 0)
    assert (step(rt, ctx, seq[3], dict())[0][..., 3] == 1).all()
    ctx.close()


def test_two_live_contexts_take_turns(rt):
    a, b = prepared(rt, 70, 53), prepared(rt, 129, 9)
    sa, sb = mi.make("dolly", 53, 70), mi.make("rotate", 9, 129)
    wa, wb = mm.run(sa, 1), mm.run(sb, 2, max_history=2.5)
    a.set_option("temporal_moments", 1)
    b.set_option("temporal_moments", 2)
    for k in range(4):
        ha, ma = step(rt, a, sa[k], dict())
        hb, mb = step(rt, b, sb[k], dict(max_history=2.5))
        check(ma, wa[k][1], 0.0, f"context 70 x 53, call {k}")
        check(mb, wb[k][1], 0.0, f"context 129 x 9, call {k}")
        check(ha, wa[k][0], 0.0, f"context 70 x 53, call {k}: history")
        assert same(a.read_temporal_moments(), ma)
    a.close()
    b.close()


def test_batching_and_the_headless_renderer(rt):
    sc = rt.scenes
    W, H = 72, 61
    scene = sc.scene_mesh(10, 5, env_size=16)
    base = sc.params_c2()
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.set_aov(GUIDES)
    ctx.set_option("temporal_moments", 2)
    ctx.upload_scene(scene)
    state = None
    for p in own_frames(rt, base, (0, 1, 1)):
        ctx.render(p, sync=False)
        ctx.temporal_accumulate()                        # (submits whatever the batching context holds back first)
        got = ctx.read_temporal_moments()
        image, normal, position, albedo = context_arrays(ctx)
        state = mm.accumulate(state, image, normal, position, p, albedo, 2)
        check(got, state["M"], 0.0, "frame_batch 8")
    ctx.close()
    hr = rt.host.HeadlessRenderer(W, H, aov=GUIDES)
    hr.set_scene(scene)
    hr.params = base
    hr.ctx.set_option("temporal_moments", 1)
    state = None
    for _ in range(3):
        p = hr.render_frame()
        hr.temporal_accumulate(max_history=4.0)
        image, normal, position, albedo = context_arrays(hr.ctx)
        state = mm.accumulate(state, image, normal, position, p, albedo, 1, max_history=4.0)
    check(hr.read_temporal_moments(), state["M"], 0.0, "headless")
    assert hr.device_temporal_moments_ptr()
    hr.ctx.close()


# ---------------------------------------------------------------------------------------------- 5. nothing else changes

@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_options(name, rt):
    """the calls with both options on between the frames of a golden case: the image stays the reference shader's, bit for bit; the RNG
    states and all four planes stay those of a run without them"""
    meta, scene, frames, expected = load_case(golden_path(name), rt)
    W, H = meta["width"], meta["height"]

    def run(calls):
        ctx = rt.host.Context(W, H)
        ctx.set_option("rng_state", 1)
        ctx.set_aov(ALL)
        ctx.upload_scene(scene)
        ctx.write_image(gc.initial_image(meta["init"], W, H))
        for k, p in enumerate(frames):
            ctx.render(p, sync=False)
            if calls:
                ctx.set_option("temporal_moments", 1 + k % 2)
                ctx.temporal_accumulate()
                ctx.temporal_accumulate(max_history=2.0, sigma_normal=0.0)
                ctx.set_option("denoise_source", 1)
                ctx.set_option("denoise_variance", 1)
                ctx.denoise_guided(demodulate=bool(k % 2))
                ctx.read_temporal_moments()
                ctx.set_option("denoise_source", 0)
                ctx.set_option("denoise_variance", 0)
        out = dict(img=ctx.read_image(), seeds=ctx.read_rng_state(), planes={p: ctx.read_aov(p) for p in (ALBEDO, NORMAL, POSITION, IDS)})
        ctx.close()
        return out

    with_calls, without = run(True), run(False)
    assert same(with_calls["img"], expected), differing(with_calls["img"], expected)
    assert same(without["img"], expected)
    fh, fw = H // 8 * 8, W // 8 * 8                      # (outside the dispatch footprint the RNG buffer is never written)
    assert (with_calls["seeds"][:fh, :fw] == without["seeds"][:fh, :fw]).all()
    for p in (ALBEDO, NORMAL, POSITION, IDS):
        assert same(with_calls["planes"][p], without["planes"][p]), f"plane {p}"


def test_options_off_give_the_bits_of_a_context_that_never_heard_of_them(rt):
    """a context on which the options were on and are off again computes what a fresh one computes: history, guided result, variance"""
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    frames = own_frames(rt, case["frames"][0], (0, 1, 1, 1))
    out = []
    for touched in (False, True):
        ctx = rt.host.Context(W, H)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        if touched:
            ctx.set_option("temporal_moments", 2)
            ctx.set_option("denoise_source", 1)
            ctx.set_option("denoise_variance", 1)
            ctx.render(frames[0])
            ctx.temporal_accumulate()
            ctx.denoise_guided()
            for key in ("temporal_moments", "denoise_source", "denoise_variance"):
                ctx.set_option(key, 0)
        for p in frames:
            ctx.render(p)
            ctx.temporal_accumulate()
        ctx.set_option("denoise_source", 1)
        ctx.denoise_guided()
        out.append((ctx.read_temporal(), ctx.read_denoised(), ctx.read_denoise_variance()))
        ctx.close()
    assert all(same(a, b) for a, b in zip(*out))


# ---------------------------------------------------------------------------------------------- 6. it helps

def rmse(a, b, tone=False):
    a, b = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    if tone:
        a, b = a / (1.0 + a), b / (1.0 + b)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def dolly_history_and_target(rt, W, H, scene, base, reference_frames=256):
    """the dolly of tests/test_gpu_temporal.py: 8 moving frames and 4 resting ones with mode 2 moments, the context left holding the history;
    and the target: `reference_frames` accumulated frames of a fresh context at the last pose, times (N + 1) / N"""
    g = rt.scenes.GlibcRand(0)

    def pose(k):
        f = np.array(base.camera_forward, np.float64)
        return tuple(float(np.float32(x)) for x in np.array(base.camera_position, np.float64) + 0.25 * k * f)

    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.set_option("temporal_moments", 2)
    for k in list(range(1, 9)) + [8] * 4:
        ctx.render(base.replace(camera_position=pose(k), reset_flag=1, frames=0, random=g.rand()), sync=False)
        ctx.temporal_accumulate()
    ref = rt.host.Context(W, H)
    ref.upload_scene(scene)
    for n in range(1, reference_frames + 1):
        ref.render(base.replace(camera_position=pose(8), frames=n, random=g.rand()), sync=False)
    target = ref.read_image().astype(np.float64) * ((reference_frames + 1.0) / reference_frames)
    ref.close()
    return ctx, target


def report(ctx, target, label):
    """RMSE of the history and of rtgl_denoise_guided over it with the spatial and with the temporal variance, linear and tone-mapped
    x / (1 + x), for sigma_lum 2 / 4 / 8: printed, and returned as {(sigma_lum, variance option): (linear, tone-mapped)}"""
    history = ctx.read_temporal()
    assert np.isfinite(target).all() and np.isfinite(history).all()
    ctx.set_option("denoise_source", 1)
    out = {"history": (rmse(history, target), rmse(history, target, True))}
    print(f"{label}: mean history length {float(history[..., 3].mean()):.2f}; RMSE of the history {out['history'][0]:.5f} linear, {out['history'][1]:.5f} tone-mapped")
    for sl in (2.0, 4.0, 8.0):
        for tv in (0, 1):
            ctx.set_option("denoise_variance", tv)
            ctx.denoise_guided(sigma_lum=sl)
            dn = ctx.read_denoised()
            out[(sl, tv)] = (rmse(dn, target), rmse(dn, target, True))
        (l0, t0), (l1, t1) = out[(sl, 0)], out[(sl, 1)]
        print(f"{label}: sigma_lum {sl:g}: guided over the history, spatial variance {l0:.5f} linear {t0:.5f} tone-mapped; "
              f"temporal variance {l1:.5f} linear {t1:.5f} tone-mapped (temporal / spatial {l1 / l0:.4f}, {t1 / t0:.4f})")
    return out


def test_c1_256_history_filtered_with_its_own_variance_is_closer_than_the_history(rt):
    """c1_256 at 256 x 256, the dolly of tests/test_gpu_temporal.py (8 moving frames, 4 resting ones), against 256 accumulated frames
    x 257/256.  Asserted: rtgl_denoise_guided (defaults) over the history with "denoise_variance" = 1 is strictly closer, by linear RMSE,
    than the unfiltered history.  Printed, not asserted: the same next to "denoise_variance" = 0, linear and tone-mapped, sigma_lum 2 / 4 / 8."""
    case, scene, W, H = named_case(rt, "c1_256")
    ctx, target = dolly_history_and_target(rt, W, H, scene, case["frames"][0])
    out = report(ctx, target, "c1_256")
    ctx.close()
    assert out[(4.0, 1)][0] < out["history"][0]


def test_c2_640x360_report(rt):
    """the same figures on the C2 scene at 640 x 360: printed for DESIGN.md 5.7, nothing asserted beyond finite results"""
    _, _, scene, frames = c2(rt)
    W, H = 640, 360
    ctx, target = dolly_history_and_target(rt, W, H, scene, next(frames))
    out = report(ctx, target, "C2 640 x 360")
    ctx.close()
    assert all(np.isfinite(v).all() for v in out.values())
