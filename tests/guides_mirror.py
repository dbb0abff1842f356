"""The fold of the first-hit planes (include/rtgl_amd.h: option "aov", "guide pass") restated in numpy: what the planes hold after a
sequence of frames, guide passes and restarts, given the planes each entry writes on its own (a fresh context, n = 1).

Every operation is rounded to binary32 on its own, as the kernels' aov_blend rounds it: v = (x + prev * (n - 1)) / n, and n == 1 stores x
exactly (no arithmetic: NaN payloads and the sign of zero survive).  The ids plane is never averaged: it holds the last entry's ids.
Pixels outside the dispatch footprint are never written and stay as allocated."""
import numpy as np

f32 = np.float32
ALBEDO, NORMAL, POSITION, IDS = 1, 2, 4, 8
FLOAT_PLANES = (ALBEDO, NORMAL, POSITION)


def next_count(n, restart, reset_flag=False):
    """(n, pending restart) after one more entry: a guide pass (reset_flag False) or a frame with its u_reset_flag"""
    return (1 if (restart or reset_flag) else n + 1), False


def footprint(h, w):
    return h // 8 * 8, w // 8 * 8


def blend(prev, x, n):
    """one float plane after entry number n"""
    prev, x = np.asarray(prev, f32), np.asarray(x, f32)
    if n == 1:
        return x.copy()
    with np.errstate(all="ignore"):
        m, fn = f32(n - 1), f32(n)
        return ((x + (prev * m).astype(f32)).astype(f32) / fn).astype(f32)


class Planes:
    """the planes of a context: {plane bit: (h, w, 4) array}, the count of their mean and the pending restart"""

    def __init__(self, h, w, mask=15):
        self.h, self.w, self.mask = h, w, mask
        self.planes = {p: np.zeros((h, w, 4), np.uint32 if p == IDS else f32) for p in (ALBEDO, NORMAL, POSITION, IDS) if mask & p}
        self.n, self.restart = 0, True                    # as setting "aov" leaves them: zeroed, a restart pending

    def restart_pending(self):
        """rtgl_clear_image, rtgl_adaptive_begin: the contents stay, the next entry starts a new mean"""
        self.restart = True

    def entry(self, single, reset_flag=False):
        """one frame or guide pass whose own planes (n = 1 on a fresh context) are `single`"""
        self.n, self.restart = next_count(self.n, self.restart, reset_flag)
        fh, fw = footprint(self.h, self.w)
        for p, held in self.planes.items():
            x = np.asarray(single[p])[:fh, :fw]
            if p == IDS:
                held[:fh, :fw] = x.view(np.uint32)
            else:
                held[:fh, :fw] = blend(held[:fh, :fw], x, self.n)
        return self

    def refused(self):
        """a refused call: nothing moves"""
        return self


def fold(singles, h, w, mask=15, resets=None):
    """the planes after the entries of `singles` in order, from a fresh restart; resets[i]: entry i is a frame with u_reset_flag"""
    out = Planes(h, w, mask)
    for i, s in enumerate(singles):
        out.entry(s, bool(resets[i]) if resets is not None else False)
    return out
