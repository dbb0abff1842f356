"""numpy restatement of a robust adaptive session (include/rtgl_amd.h, "robust adaptive sampling"): the fold of a sample image into the
bucket of each active tile's next sample, the update (per tile whose count has moved: the record of rtgl_robust_error_estimate's steps 1-9
over the tile's footprint pixels), the resolve with every pixel's N taken from its tile, and a Session that strings them together.  The
arithmetic is robust_mirror's (fold, resolve) and robust_error_mirror's (pixel_error) applied tile by tile with the tile's own count; the
shapes, the mask rule, the lists and the summary are adaptive_mirror's.  No GPU; tests/test_robust_adaptive_mirror.py pins it against a
scalar restatement, tests/test_gpu_robust_adaptive.py compares the device with it bit for bit."""
import numpy as np

import adaptive_mirror as am
import error_mirror as em
import robust_error_mirror as rem
import robust_mirror as rm

f32 = np.float32
TILE = em.TILE
TILE_DTYPE = am.TILE_DTYPE
BUCKETS = rm.BUCKETS
DEST_BUFFER, DEST_IMAGE = rm.DEST_BUFFER, rm.DEST_IMAGE
DEFAULTS = dict(buckets=8, threshold=0.05, floor=0.01, gain=1.0, min_samples=32, max_samples=1024)
MAX_SAMPLES = 1 << 24                                              # (float) of every count up to here is exact


def valid_params(buckets, threshold, floor, gain, min_samples, max_samples, flags=0, reserved=0):
    with np.errstate(over="ignore"):
        threshold, floor, gain = f32(threshold), f32(floor), f32(gain)      # (the record holds binary32)
    return bool(buckets in BUCKETS and np.isfinite(threshold) and threshold > 0 and np.isfinite(floor) and floor > 0 and np.isfinite(gain)
                and gain >= 0 and buckets <= min_samples <= max_samples <= MAX_SAMPLES and flags == 0 and reserved == 0)


def tile_slices(h, w):
    """[(t, rows, columns)]: the footprint pixels of every tile that holds one, t ascending"""
    s = am.shape(h, w)
    out = []
    for t in range(s["ty"] * s["tx"]):
        y0, x0 = t // s["tx"] * TILE, t % s["tx"] * TILE
        y1, x1 = min(y0 + TILE, s["fh"]), min(x0 + TILE, s["fw"])
        if y1 > y0 and x1 > x0:
            out.append((t, slice(y0, y1), slice(x0, x1)))
    return out


def fold(planes, source, n, mask):
    """one fold: per active tile t and footprint pixel of it, with j = n[t] mod K and k = n[t] div K, b_j' = (x + b_j (float)k) / (float)(k + 1),
    all four components; then n[t] = n[t] + 1.  Returns (planes, n); the inputs are left as they are."""
    planes, source = np.array(planes, f32), np.asarray(source, f32)
    K, h, w = planes.shape[:3]
    n = np.array(n, np.uint32).reshape(am.shape(h, w)["ty"], am.shape(h, w)["tx"])
    mask = am.explicit_mask(h, w, mask)
    for t, ys, xs in tile_slices(h, w):
        if mask.ravel()[t]:
            nt = int(n.ravel()[t])
            j, k = rm.next_bucket(nt, K), rm.next_count(nt, K)
            planes[j, ys, xs] = rm.fold(planes[j, ys, xs], source[ys, xs], k)
    return planes, n + mask.astype(np.uint32)


def update(planes, n, m, records, threshold=0.05, floor=0.01, gain=1.0):
    """the device half of rtgl_robust_adaptive_update: per tile with n != m the record {0, 0, 0, 0, n, n} (n < K) or the estimate of its
    footprint pixels, and m = n.  Returns (m, records); the inputs are left as they are."""
    planes = np.asarray(planes, f32)
    K, h, w = planes.shape[:3]
    s = am.shape(h, w)
    n, m = np.asarray(n, np.uint32).reshape(s["ty"], s["tx"]), np.array(m, np.uint32).reshape(s["ty"], s["tx"])
    records = np.array(records).reshape(s["ty"], s["tx"])
    threshold = f32(threshold)
    slices = {t: (ys, xs) for t, ys, xs in tile_slices(h, w)}
    for t in range(n.size):
        at = (t // s["tx"], t % s["tx"])
        nt = int(n[at])
        if nt == int(m[at]):
            continue
        rec = np.zeros((), TILE_DTYPE)
        rec["samples"] = rec["samples_snapshot"] = nt
        if nt >= K and t in slices:
            ys, xs = slices[t]
            e, counts = rem.pixel_error(planes[:, ys, xs], nt, gain, floor)
            leaves, cnt = np.zeros((TILE, TILE), f32), np.zeros((TILE, TILE), bool)
            leaves[:e.shape[0], :e.shape[1]] = np.where(counts, e, f32(0))
            cnt[:e.shape[0], :e.shape[1]] = counts
            total, count = em.tree(leaves.reshape(-1)), int(cnt.sum())
            if count:
                with np.errstate(all="ignore"):
                    mse = f32(f32(total) / f32(count))
                    rec["sum"], rec["mse"], rec["count"], rec["converged"] = total, mse, count, int(mse <= threshold * threshold)
        records[at] = rec
        m[at] = nt
    return m, records


def resolve(planes, n, gain=1.0, dest=DEST_BUFFER):
    """per pixel with N = n[t] of its tile: +0 in all four components outside the footprint or with N == 0, else robust_mirror's resolve
    with that N: {out.rgb, G} (dest BUFFER) or out (dest IMAGE), (h, w, 4)"""
    planes = np.asarray(planes, f32)
    K, h, w = planes.shape[:3]
    n = np.asarray(n, np.uint32).ravel()
    out = np.zeros((h, w, 4), f32)
    for t, ys, xs in tile_slices(h, w):
        if n[t]:
            out[ys, xs] = (rm.image_plane if dest == DEST_IMAGE else rm.output_plane)(planes[:, ys, xs], int(n[t]), gain)
    return out


class Session:
    """The state of a session: begin where the context calls rtgl_robust_adaptive_begin, fold(sample) with the FULL one-frame image of the
    frame's uniforms where it calls rtgl_robust_adaptive_frame, or with the image where it calls _accumulate (only the footprint pixels of
    the active tiles are taken from it), update(), set_mask() and resolve() likewise."""

    def __init__(self, h, w, **params):
        self.h, self.w = h, w
        self.params = dict(DEFAULTS)
        self.params.update({k: v for k, v in params.items() if v is not None})
        assert valid_params(**self.params)
        s = am.shape(h, w)
        self.K = self.params["buckets"]
        self.planes = np.zeros((self.K, h, w, 4), f32)
        self.n, self.m = np.zeros((s["ty"], s["tx"]), np.uint32), np.zeros((s["ty"], s["tx"]), np.uint32)
        self.records = np.zeros((s["ty"], s["tx"]), TILE_DTYPE)
        self.mask = am.full_mask(h, w)

    def blocks(self):
        return am.block_list(self.h, self.w, self.mask)

    def tiles(self):
        return am.tile_list(self.mask)

    def set_mask(self, tiles):
        self.mask = am.explicit_mask(self.h, self.w, tiles)

    def fold(self, sample):
        self.planes, self.n = fold(self.planes, sample, self.n, self.mask)

    def update(self):
        p = self.params
        self.m, self.records = update(self.planes, self.n, self.m, self.records, p["threshold"], p["floor"], p["gain"])
        self.mask = am.rule(self.h, self.w, self.records, p["min_samples"], p["max_samples"])
        return am.summary(self.h, self.w, self.records, self.mask, p["max_samples"])

    def resolve(self, gain=1.0, dest=DEST_BUFFER):
        assert rm.valid_resolve_params(gain, dest)
        return resolve(self.planes, self.n, gain, dest)


def render(frame, threshold, max_samples, min_samples=None, check_every=16, buckets=8, gain=1.0, floor=None, h=None, w=None):
    """HeadlessRenderer.render_robust_adaptive written out: frame(k) gives the k-th full one-sample image.  Returns (frames, the latest
    summary, the session)"""
    sess = Session(h, w, buckets=buckets, threshold=threshold, floor=floor, gain=gain, min_samples=min_samples, max_samples=max_samples)
    done, summary = 0, sess.update()
    while not summary["converged"]:
        for _ in range(check_every):
            sess.fold(frame(done))
            done += 1
        summary = sess.update()
    return done, summary, sess
