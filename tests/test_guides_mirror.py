"""tests/guides_mirror.py, the numpy fold of the first-hit planes that tests/test_gpu_guides.py holds the device against: its count, its
arithmetic in binary32, its ids, its restarts -- and that each of three likely defects (a count that is not restarted, prev * n in place
of prev * (n - 1), ids that are averaged) gives other planes on the inputs the device test uses, so the mirror can tell them apart."""
from fractions import Fraction

import numpy as np
import pytest

import guides_mirror as gm

f32 = np.float32
H, W = 19, 27                                             # footprint 16 x 24


def singles(k, seed=0, h=H, w=W):
    """k entries' own planes: floats over several binades, ids of the three kinds"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        s = {p: (g.standard_normal((h, w, 4)) * 10.0 ** g.integers(-3, 4, (h, w, 1))).astype(f32) for p in gm.FLOAT_PLANES}
        s[gm.IDS] = g.integers(0, 5000, (h, w, 4)).astype(np.uint32)
        out.append(s)
    return out


def same(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def test_count_progression():
    assert gm.next_count(0, True) == (1, False) and gm.next_count(7, True) == (1, False)
    assert gm.next_count(1, False) == (2, False) and gm.next_count(41, False) == (42, False)
    assert gm.next_count(5, False, reset_flag=True) == (1, False) and gm.next_count(5, True, reset_flag=True) == (1, False)
    p = gm.Planes(H, W)
    assert (p.n, p.restart) == (0, True)
    s = singles(4)
    p.entry(s[0]); assert (p.n, p.restart) == (1, False)
    p.entry(s[1]); p.entry(s[2]); assert p.n == 3
    p.refused(); assert (p.n, p.restart) == (3, False)
    p.restart_pending(); assert (p.n, p.restart) == (3, True)
    p.refused(); assert (p.n, p.restart) == (3, True)
    p.entry(s[3]); assert (p.n, p.restart) == (1, False)
    p.entry(s[0], reset_flag=True); assert p.n == 1
    p.entry(s[1]); assert p.n == 2


def test_first_entry_is_stored_exactly():
    s = singles(1)[0]
    s[gm.ALBEDO][0, 0] = np.array([0x7FC12345, 0xFFC00001, 0x80000000, 0x00000001], np.uint32).view(f32)      # NaN payloads, -0, a denormal
    s[gm.POSITION][1, 2] = np.array([np.inf, -np.inf, 3.4028235e38, -1e-45], f32)
    p = gm.Planes(H, W).entry(s)
    fh, fw = gm.footprint(H, W)
    for k in (gm.ALBEDO, gm.NORMAL, gm.POSITION, gm.IDS):
        assert same(p.planes[k][:fh, :fw], s[k][:fh, :fw])
        assert not p.planes[k][fh:].any() and not p.planes[k][:, fw:].any()      # outside the footprint: as allocated
    # ... and again after a restart, whatever was there
    p.entry(singles(1, seed=5)[0]).restart_pending()
    p.entry(s)
    assert same(p.planes[gm.ALBEDO][:fh, :fw], s[gm.ALBEDO][:fh, :fw])


def test_each_operation_is_rounded_to_binary32():
    """against exact rational arithmetic rounded after every operation"""
    def r(q):                                             # nearest binary32 of a rational inside the normal range
        return Fraction(float(f32(float(q)))) if abs(q) < Fraction(2) ** 100 else None
    g = np.random.default_rng(3)
    prev, x = g.standard_normal(500).astype(f32), g.standard_normal(500).astype(f32)
    for n in (2, 3, 7, 100):
        got = gm.blend(prev, x, n)
        for a, b, v in zip(prev, x, got):
            prod = r(Fraction(float(a)) * (n - 1))
            want = r(r(Fraction(float(b)) + prod) / n)
            assert Fraction(float(v)) == want


def test_ids_are_the_last_entrys_and_floats_the_running_mean():
    s = singles(5)
    p = gm.fold(s, H, W)
    fh, fw = gm.footprint(H, W)
    assert p.n == 5 and same(p.planes[gm.IDS][:fh, :fw], s[-1][gm.IDS][:fh, :fw])
    want = s[0][gm.NORMAL][:fh, :fw]
    for n in range(2, 6):
        want = ((s[n - 1][gm.NORMAL][:fh, :fw] + want * f32(n - 1)) / f32(n)).astype(f32)
    assert same(p.planes[gm.NORMAL][:fh, :fw], want)
    mean = np.mean([e[gm.NORMAL][:fh, :fw].astype(np.float64) for e in s], axis=0)
    assert np.allclose(p.planes[gm.NORMAL][:fh, :fw], mean, rtol=1e-4, atol=1e-4 * np.abs(mean).max())


def test_masks_hold_only_their_planes():
    s = singles(2)
    for mask in (1, 2, 4, 8, 15, 5):
        p = gm.fold(s, H, W, mask)
        assert sorted(p.planes) == [b for b in (1, 2, 4, 8) if mask & b]


def test_reset_frames_restart():
    s = singles(4)
    p = gm.fold(s, H, W, resets=[0, 0, 1, 0])
    q = gm.fold(s[2:], H, W)
    assert p.n == 2 and all(same(p.planes[k], q.planes[k]) for k in p.planes)


# ---- three defects the mirror must be distinguishable from

class NoRestart(gm.Planes):
    def entry(self, single, reset_flag=False):
        self.restart = self.restart and self.n == 0       # only the very first entry starts a mean
        return super().entry(single, False)


class PrevTimesN(gm.Planes):
    def entry(self, single, reset_flag=False):
        self.n, self.restart = gm.next_count(self.n, self.restart, reset_flag)
        fh, fw = gm.footprint(self.h, self.w)
        for p, held in self.planes.items():
            x = np.asarray(single[p])[:fh, :fw]
            if p == gm.IDS:
                held[:fh, :fw] = x
            elif self.n == 1:
                held[:fh, :fw] = x
            else:
                held[:fh, :fw] = ((x + held[:fh, :fw] * f32(self.n)) / f32(self.n)).astype(f32)
        return self


class IdsAveraged(gm.Planes):
    def entry(self, single, reset_flag=False):
        before = self.planes[gm.IDS].copy()
        super().entry(single, reset_flag)
        if self.n > 1:
            fh, fw = gm.footprint(self.h, self.w)
            self.planes[gm.IDS][:fh, :fw] = ((single[gm.IDS][:fh, :fw].astype(np.uint64) + before[:fh, :fw].astype(np.uint64) * (self.n - 1)) // self.n).astype(np.uint32)
        return self


def run(cls, s):
    """frame, guides, guides, frame; a restart; guides, guides -- the shape of the device test's sequences"""
    p = cls(H, W)
    for e in s[:4]:
        p.entry(e)
    p.restart_pending()
    for e in s[4:6]:
        p.entry(e)
    return p


@pytest.mark.parametrize("cls, differs_in", [(NoRestart, gm.FLOAT_PLANES), (PrevTimesN, gm.FLOAT_PLANES), (IdsAveraged, (gm.IDS,))])
def test_a_defective_copy_gives_other_planes(cls, differs_in):
    s = singles(6, seed=9)
    good, bad = run(gm.Planes, s), run(cls, s)
    for k in differs_in:
        assert not same(good.planes[k], bad.planes[k]), (cls.__name__, k)
    # ... already before the restart for the arithmetic and the ids, and only behind it for the count
    good4, bad4 = gm.fold(s[:4], H, W), cls(H, W)
    for e in s[:4]:
        bad4.entry(e)
    differs_early = any(not same(good4.planes[k], bad4.planes[k]) for k in differs_in)
    assert differs_early == (cls is not NoRestart)
