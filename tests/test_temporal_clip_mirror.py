"""tests/temporal_clip_mirror.py, the numpy restatement of rtgl_temporal_clip that tests/test_gpu_temporal_clip.py holds the kernel against,
pinned without a GPU: it equals a second, scalar restatement written from the contract (include/rtgl_amd.h, "temporal clip") in every bit;
it has the properties the definition promises; it does what the call is for (a history that follows a change of lighting); and the scalar
restatement with one plausible defect at a time changes bits that are not NaN on a case the GPU module runs, so a kernel with that defect
cannot pass there."""
import numpy as np
import pytest

import temporal_clip_inputs as ci
import temporal_clip_mirror as cm
import temporal_mirror as tm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def agrees(got, want):
    """the comparison rule of the GPU module: same bits where the mirror has a number, any NaN where it has a NaN"""
    return got.shape == want.shape and not np.where(np.isnan(want), ~np.isnan(got), bits(got) != bits(want)).any()


_sequences, _caches, _runs = {}, {}, {}


def sequence(family, size):
    key = (family, size)
    if key not in _sequences:
        _sequences[key] = ci.make(family, size[1], size[0])
        _caches[key] = {}
    return _sequences[key]


def mirror(family, size, ps, mode=1):
    """[(history before the clip, after, moments before, after)] per frame; ps None: the sequence without clip calls"""
    key = (family, size, None if ps is None else tuple(sorted(ps.items())), mode)
    if key not in _runs:
        seq = sequence(family, size)
        _runs[key] = cm.run(seq, mode, ps, _caches[(family, size)])
    return _runs[key]


# ---------------------------------------------------------------------------------------------- 1. the two restatements agree

# The scalar restatement costs about half a millisecond per pixel and call, so what is reduced is pixels and frames, never sizes,
# parameter sets or modes: EVERY listed size x EVERY parameter set x modes 0, 1 and 2 is compared.  Up to 7 x 5: every pixel of every
# frame, all three modes per parameter set.  Above: two frames (the one two thirds in, where the relit families change, and the last),
# the mode rotating with the parameter set (the mode only decides whether there is a moments record for the length to go to, and every
# mode meets every size), and of each frame the pixels along the image's and the tiles' edges and 60 random ones, which below 400
# pixels is most of the image.

def sampled(size):
    W, H = size
    if W * H <= 35:
        return None
    rng = np.random.default_rng(W)
    cols = [x for x in (0, 1, 3, 60, 63, 64, 66, 127, 128, W - 4, W - 1) if 0 <= x < W]
    rows = [y for y in (0, 2, 3, 4, 7, 8, H - 4, H - 1) if 0 <= y < H]
    picks = {(x, int(rng.integers(H))) for x in cols} | {(int(rng.integers(W)), y) for y in rows} | {(x, y) for x in cols[:6] for y in rows[:4]}
    picks |= {(int(rng.integers(W)), int(rng.integers(H))) for _ in range(60)}
    return sorted(picks)


@pytest.mark.parametrize("family", sorted(ci.FAMILIES))
def test_mirror_equals_the_scalar_restatement(family):
    for size in ci.SIZES:
        pixels = sampled(size)
        seq = sequence(family, size)
        frames = range(len(seq)) if pixels is None else sorted({2 * len(seq) // 3, len(seq) - 1})
        for i, ps in enumerate(ci.PARAMETER_SETS):
            for mode in ci.MODES if pixels is None else [ci.MODES[(i + 1) % 3]]:
                assert (family, size, ps, mode) in ci.listed_cases()
                out = mirror(family, size, ps, mode)
                for k in frames:
                    image, normal, position = seq[k][:3]
                    H0, H1, M0, M1 = out[k]
                    gh, gm = cm.scalar_clip(H0, M0, image, normal, position, pixels=pixels, **dict(cm.DEFAULTS, **ps))
                    label = f"{family} {size} {ps} mode {mode} frame {k}"
                    assert (gm is None) == (M1 is None) == (mode == 0), label
                    pairs = [(gh, H1)] + ([(gm, M1)] if mode else [])
                    if pixels is not None:
                        xs, ys = np.array([p[0] for p in pixels]), np.array([p[1] for p in pixels])
                        pairs = [(g[ys, xs], w[ys, xs]) for g, w in pairs]
                    for g, w in pairs:
                        assert agrees(g, w), label
                        assert (np.isnan(g) == np.isnan(w)).all(), f"{label}: the NaNs are not in the same places"


def test_bad_parameters_raise():
    image, normal, position = sequence("rest", (7, 5))[0][:3]
    for ps in (dict(sigma_scale=0.0), dict(sigma_scale=-1.0), dict(sigma_scale=float("nan")), dict(clip_history=0.5), dict(clip_history=float("inf")),
               dict(sigma_normal=float("inf")), dict(sigma_position=float("nan"))):
        with pytest.raises(ValueError):
            cm.clip(image, None, image, normal, position, **ps)
    with pytest.raises(ValueError):
        cm.clip(image, None, image, None, position)
    assert cm.clip(image, None, image, None, position, sigma_normal=0.0)[1] is None


# ---------------------------------------------------------------------------------------------- 2. the NaN cap

@pytest.mark.parametrize("family", sorted(ci.FAMILIES))
def test_nan_share_of_the_mirror_is_within_the_cap(family):
    """the comparison on the device cannot see into a NaN: at most NAN_CAP of the components of any call's history and of the lengths in
    its moments' .w, and none outside `specials` (m1, m2 and v of `specials` go beyond the cap -- DESIGN.md 5.7 -- and are not this call's:
    the GPU module holds them to what they were before the call, bit for bit)"""
    seen = 0.0
    for size in ci.SIZES:
        for ps in ci.PARAMETER_SETS:
            for k, (H0, H1, M0, M1) in enumerate(mirror(family, size, ps)):
                share = max(float(np.isnan(H1).mean()), float(np.isnan(M1[..., 3]).mean()), float(np.isnan(H0).mean()))
                seen = max(seen, share)
                assert share <= ci.nan_budget(family), f"{family} {size} {ps} call {k}: {share:.4%}"
    print(f"{family}: largest NaN share of a history or of the moments' lengths {seen:.4%}")
    if family == "specials":
        assert seen > 0, "the family is there to put NaN and infinities in front of the kernel"


# ---------------------------------------------------------------------------------------------- 3. properties

@pytest.mark.parametrize("family", sorted(ci.FAMILIES))
def test_properties_on_every_listed_case(family):
    """a second clip is the identity; clip_history = 1e6 leaves every n alone; the moments' .w is the history's alpha after the call and
    m1, m2, v are untouched; every changed component lies in the widened box; the option's mode does not change the history"""
    for size in ci.SIZES:
        seq = sequence(family, size)
        for ps in ci.PARAMETER_SETS:
            full = dict(cm.DEFAULTS, **ps)
            plain = mirror(family, size, ps, 0) if size[0] * size[1] < 10000 else None
            for k, (H0, H1, M0, M1) in enumerate(mirror(family, size, ps)):
                label = f"{family} {size} {ps} frame {k}"
                image, normal, position = seq[k][:3]
                sums = _caches[(family, size)][(k, max(float(f32(full["sigma_normal"])), 0.0), max(float(f32(full["sigma_position"])), 0.0))]
                H2, M2 = cm.clip(H1, M1, image, normal, position, sums=sums, **full)
                assert same(H2, H1) and same(M2, M1), f"{label}: a second clip is not the identity"
                assert same(M1[..., 3], H1[..., 3]) and same(M1[..., :3], M0[..., :3]), label
                if ps.get("clip_history") == 1e6:
                    assert same(H1[..., 3], H0[..., 3]), label
                s0, lo, hi = cm.box(image, normal, position, full["sigma_scale"], full["sigma_normal"], full["sigma_position"], sums)
                changed = bits(H1[..., :3]) != bits(H0[..., :3])
                with np.errstate(all="ignore"):
                    assert ((H1[..., :3] >= lo) & (H1[..., :3] <= hi) & (s0 > 0)[..., None])[changed].all(), f"{label}: a clipped component outside its box"
                assert (H1[..., 3] <= H0[..., 3])[~np.isnan(H0[..., 3])].all(), label
                if plain is not None:
                    assert same(plain[k][1], H1) and plain[k][3] is None, f"{label}: the moments option changed the history"


def test_flat_radiance_is_left_alone():
    for size in ci.SIZES:
        for ps in ci.PARAMETER_SETS:
            for k, (H0, H1, M0, M1) in enumerate(mirror("flat", size, ps)):
                assert same(H1, H0) and same(M1, M0), f"flat {size} {ps} frame {k}"
                assert (H1[..., 3] == min(k + 1, 32)).all()


NOISY = ["rest", "translate", "rotate", "dolly", "all_miss", "skewed", "relight", "relight_moving", "edge", "narrow"]


@pytest.mark.parametrize("family", NOISY)
def test_a_box_of_a_million_sigmas_clips_nothing(family):
    """sigma_scale = 1e6, finite inputs: the history is bit for bit tests/temporal_mirror.py's wherever the window holds two taps that
    differ (a variance > 0 in every channel).  A pixel alone in its window has the box [I, I], by the contract, and its history becomes
    the frame: in the families taken from tests/temporal_inputs.py neighbouring hits are 23.7 / W position tolerances apart, so that is
    every hit below 63 columns; from 63 columns on no pixel is alone.  `narrow` is there for the small sizes: its neighbours are
    1.6 / W tolerances apart, and from 2 x 2 on the whole history, every frame, is tests/temporal_mirror.py's (1 x 1 has no
    neighbour to have)."""
    for size in ci.SIZES:
        seq = sequence(family, size)
        want = tm.run([item[:4] for item in seq])
        alone = 0
        for k, (H0, H1, M0, M1) in enumerate(mirror(family, size, dict(sigma_scale=1e6), 0)):
            s0, lo, hi = cm.box(*seq[k][:3], sigma_scale=1e6)
            wide = (s0 > 0) & ((hi - lo) > 1).all(-1)
            alone += int((~wide).sum())
            assert same(H1[wide], H0[wide]), f"{family} {size} frame {k}"
            if alone == 0:
                assert same(H1, want[k]), f"{family} {size} frame {k}"
        if size[0] >= 63 or (family == "narrow" and size != (1, 1)):
            assert alone == 0, f"{family} {size}: {alone} pixels alone in their windows"


# ---------------------------------------------------------------------------------------------- 4. what it is for

def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b) ** 2)))


def test_relit_history_follows_the_new_lighting():
    """`relight` at 200 x 131, the defaults: RMSE of the history against the noise-free relit radiance after the fourth relit frame; with
    the clip it must be below HALF of that without it.  Derivation: without the clip the old radiance keeps weight 8 / 12 = 0.67 of a
    change of about 1.1; with it the history is within 2 sigma of the new neighbourhood mean after the first relit frame and averages on
    with n <= 3.  Measured here: 0.2526 against 0.7458, ratio 0.339."""
    size = (200, 131)
    before, after = ci.relight_truth(size[1], size[0])
    clipped, plain = mirror("relight", size, dict(), 0), mirror("relight", size, None, 0)
    e_clip, e_plain = rmse(clipped[-1][1], after), rmse(plain[-1][1], after)
    print(f"relight 200 x 131 after 4 relit frames: RMSE with the clip {e_clip:.4f}, without {e_plain:.4f}, ratio {e_clip / e_plain:.3f}")
    assert e_clip < 0.5 * e_plain


def test_cost_at_rest_is_small_and_falls_with_the_box_width():
    """frames 1 - 8 of `relight` (nothing changes): the share of pixels the clip touches and the RMSE of the eighth history beside the
    unclipped one's are printed (0.02 % of the pixels per frame at the default, 2.83 % at sigma_scale = 1; RMSE 0.0204 and
    0.0203 against the unclipped 0.0204); asserted: the default box clips fewer pixels than sigma_scale = 1 does"""
    size = (200, 131)
    before, _ = ci.relight_truth(size[1], size[0])
    plain = mirror("relight", size, None, 0)
    shares = {}
    for scale in (1.0, 2.0):
        out = mirror("relight", size, dict(sigma_scale=scale) if scale != 2.0 else dict(), 0)
        touched = [float((bits(H1) != bits(H0)).any(-1).mean()) for H0, H1, _, _ in out[:ci.RELIT_AFTER]]
        shares[scale] = float(np.mean(touched))
        print(f"relight 200 x 131 at rest, sigma_scale {scale:g}: {shares[scale]:.2%} of the pixels clipped per frame, RMSE of frame 8 "
              f"{rmse(out[ci.RELIT_AFTER - 1][1], before):.4f} (unclipped {rmse(plain[ci.RELIT_AFTER - 1][1], before):.4f})")
    assert shares[2.0] < shares[1.0]


# ---------------------------------------------------------------------------------------------- 5. teeth

BOTH_OFF = dict(sigma_normal=0.0, sigma_position=-1.0)
TEETH = {"box_not_widened": ("rest", (7, 5), dict(sigma_scale=0.5)),
         "scale_on_variance": ("relight", (63, 3), dict()),
         "variance_not_clamped": ("specials", (65, 5), dict()),
         "window_5x5": ("rest", (7, 5), dict(sigma_scale=0.5)),
         "kind_unchecked": ("specials", (65, 5), BOTH_OFF),
         "binary_weights": ("rest", (65, 5), dict(sigma_scale=0.5)),
         "n_always_cut": ("rest", (7, 5), dict(sigma_scale=1e6)),
         "n_never_cut": ("relight", (7, 5), dict()),
         "moments_w_stale": ("relight", (7, 5), dict()),
         "s2_fused": ("relight", (63, 3), dict(sigma_scale=0.5))}


def defective(family, size, ps, defect):
    seq = sequence(family, size)
    got = []
    for k, (H0, H1, M0, M1) in enumerate(mirror(family, size, ps)):
        got.append(cm.scalar_clip(H0, M0, *seq[k][:3], defect=defect, **dict(cm.DEFAULTS, **ps)))
    return got


@pytest.mark.parametrize("defect", sorted(TEETH))
def test_a_defect_changes_bits_on_a_listed_case(defect):
    family, size, ps = TEETH[defect]
    assert (family, size, ps, 1) in ci.listed_cases() and defect in cm.DEFECTS
    want = mirror(family, size, ps)
    changed = 0
    for (gh, gm), (H0, H1, M0, M1) in zip(defective(family, size, ps, defect), want):
        for g, w in ((gh, H1), (gm, M1)):
            changed += int((~np.isnan(w) & ~np.isnan(g) & (bits(g) != bits(w))).sum())
    assert changed > 0, f"{defect}: {family} {size} {ps} does not see it"


def test_the_order_of_the_two_clamps_cannot_matter():
    """`hi` applied before `lo` is not a defect a test can see, and none is asked to: e >= 0, so lo = mu - e <= mu <= mu + e = hi by the
    monotonicity of a rounded add, the widening only lowers lo and raises hi, and a NaN bound compares false in either order; with
    lo <= hi the two orders pick the same value and set the same flag.  Held here on every small listed case instead: the scalar
    restatement with the order swapped agrees with the mirror in every bit."""
    assert "hi_before_lo" in cm.DEFECTS and "hi_before_lo" not in TEETH
    for family in sorted(ci.FAMILIES):
        for size in ((2, 2), (7, 5)):
            for ps in (dict(), dict(sigma_scale=0.5), BOTH_OFF):
                for (gh, gm), (H0, H1, M0, M1) in zip(defective(family, size, ps, "hi_before_lo"), mirror(family, size, ps)):
                    assert agrees(gh, H1) and agrees(gm, M1), f"{family} {size} {ps}"
