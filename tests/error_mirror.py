"""numpy restatement of rtgl_error_estimate (include/rtgl_amd.h, "error estimate"): every operation in binary32 in the order the header
writes, the tile sums by the balanced pairwise tree (repeated a[0::2] + a[1::2]), the whole-picture sum by 256 strided lanes and the same
tree, and the snapshot / epoch rules over a sequence of calls (class Estimator).  No GPU; tests/test_error_mirror.py pins it against a
scalar restatement, tests/test_gpu_error_estimate.py compares the device with it bit for bit."""
import numpy as np

DEFAULTS = dict(threshold=0.05, floor=0.01, quantile_permille=950, first_frames=1, keep_snapshot=False)
TILE = 16
TILE_DTYPE = np.dtype([("sum", np.float32), ("mse", np.float32), ("count", np.uint32), ("converged", np.uint32)])
SUMMARY_INT = ("valid", "converged", "frames_now", "frames_snapshot", "tiles_valid", "tiles_converged", "pixels_ignored")
SUMMARY_FLOAT = ("scale", "mse", "max_tile_mse")

f32 = np.float32


def lum(img):
    img = np.asarray(img, np.float32)
    return (f32(0.25) * img[..., 0] + f32(0.5) * img[..., 1]) + f32(0.25) * img[..., 2]


def tree(a):
    """the balanced pairwise tree over the last axis (a power of two long): adjacent pairs first"""
    a = np.asarray(a, np.float32)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def tiles_of(h, w):
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE          # (ty, tx)


def scales(frames_now, frames_snapshot, first_frames):
    """(g_n, g_m, c) as the host computes them: in float64, rounded once"""
    n, m = frames_now + 1 - first_frames, frames_snapshot + 1 - first_frames
    assert 1 <= m < n
    return f32(float(frames_now + 1) / float(n)), f32(float(frames_snapshot + 1) / float(m)), f32(float(m) / float(n - m))


def empty_result(h, w):
    """what a call without a usable snapshot leaves: valid 0, everything else 0, the tile records zeroed"""
    out = {k: 0 for k in SUMMARY_INT}
    out.update({k: f32(0.0) for k in SUMMARY_FLOAT})
    out["tiles"] = np.zeros(tiles_of(h, w), TILE_DTYPE)
    return out


def estimate(image, snapshot, frames_now, frames_snapshot, threshold=0.05, floor=0.01, quantile_permille=950, first_frames=1):
    """One estimate: `image` (h, w, 4) after the frame rendered with frames = frames_now, `snapshot` (h, w) the raw lum of the image after
    the frame with frames = frames_snapshot.  Returns the summary's fields and "tiles", a structured array (ty, tx)."""
    image = np.asarray(image, np.float32)
    h, w = image.shape[:2]
    fh, fw = h // 8 * 8, w // 8 * 8
    ty, tx = tiles_of(h, w)
    g_n, g_m, c = scales(frames_now, frames_snapshot, first_frames)
    threshold, floor = f32(threshold), f32(floor)
    with np.errstate(all="ignore"):
        Ln = lum(image) * g_n
        Lm = np.asarray(snapshot, np.float32) * g_m
        d = Ln - Lm
        den = np.where(Ln > 0, Ln, f32(0.0)).astype(np.float32) + floor
        q = d / den
        e = q * q
        inside = np.zeros((h, w), bool)
        inside[:fh, :fw] = True
        counts = inside & (e - e == 0)
        padded = np.zeros((ty * TILE, tx * TILE), np.float32)
        padded[:h, :w] = np.where(counts, e, f32(0.0))
        cpad = np.zeros((ty * TILE, tx * TILE), np.uint32)
        cpad[:h, :w] = counts
        per_tile = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)
        tiles = np.zeros((ty, tx), TILE_DTYPE)
        tiles["sum"] = tree(per_tile(padded))
        tiles["count"] = per_tile(cpad).sum(-1, dtype=np.uint32)
        valid = tiles["count"] > 0
        mse = (tiles["sum"] / np.where(valid, tiles["count"], 1).astype(np.float32)) * c
        tiles["mse"] = np.where(valid, mse, f32(0.0))
        tiles["converged"] = valid & (mse <= threshold * threshold)
        tiles["sum"] = np.where(valid, tiles["sum"], f32(0.0))
        # the whole picture: lane t adds the tile sums t, t + 256, ... in ascending order from +0, the 256-leaf tree combines the lanes
        flat = tiles["sum"].ravel()
        rows = -(-len(flat) // 256)
        lanes_in = np.zeros(rows * 256, np.float32)
        lanes_in[:len(flat)] = flat
        lanes = np.zeros(256, np.float32)
        for row in lanes_in.reshape(rows, 256):
            lanes = lanes + row
        total = tree(lanes)
        N = int(tiles["count"].sum(dtype=np.uint64))
        out = dict(valid=1, frames_now=int(frames_now), frames_snapshot=int(frames_snapshot), tiles_valid=int(valid.sum()),
                   tiles_converged=int(tiles["converged"].sum()), pixels_ignored=fh * fw - N, scale=c,
                   mse=(total / f32(np.uint64(N))) * c if N else f32(0.0),
                   max_tile_mse=tiles["mse"][valid].max() if valid.any() else f32(0.0), tiles=tiles)
    out["converged"] = int(out["tiles_valid"] > 0 and out["tiles_converged"] * 1000 >= out["tiles_valid"] * int(quantile_permille))
    return out


class Estimator:
    """The state of a context: the snapshot, its F_m and first_frames, and the epoch.  Tell it what happens to the image (`frame` for
    every rendered frame, `drop` for rtgl_error_reset / rtgl_clear_image / rtgl_write_image_f32 / rtgl_bind_device_image) and call it
    where the context calls rtgl_error_estimate, with the image as it is then."""

    def __init__(self):
        self.epoch, self.snap_epoch = 1, 0
        self.snapshot, self.fm, self.first, self.fn = None, 0, 0, None

    def drop(self):
        self.epoch += 1

    def frame(self, frames, reset_flag=0):
        if reset_flag:
            self.drop()
        self.fn = int(frames)

    def has_snapshot(self):
        return self.snap_epoch == self.epoch

    def __call__(self, image, **params):
        p = dict(DEFAULTS)
        p.update(params)
        keep_flag = p.pop("keep_snapshot")
        assert self.fn is not None, "no frame has been rendered"
        assert self.fn + 1 - p["first_frames"] >= 1, "RTGL_ERR_INVALID: n < 1"
        image = np.asarray(image, np.float32)
        usable = self.has_snapshot() and self.fn > self.fm and p["first_frames"] == self.first
        out = estimate(image, self.snapshot, self.fn, self.fm, **p) if usable else empty_result(*image.shape[:2])
        if not (usable and keep_flag):
            self.snapshot, self.fm, self.first, self.snap_epoch = lum(image), self.fn, p["first_frames"], self.epoch
        return out


def same_result(a, b):
    """bit for bit: the summary's fields and every tile record; returns the names that differ"""
    bad = [k for k in SUMMARY_INT if int(a[k]) != int(b[k])]
    bad += [k for k in SUMMARY_FLOAT if f32(a[k]).view(np.uint32) != f32(b[k]).view(np.uint32)]
    ta, tb = np.ascontiguousarray(a["tiles"]), np.ascontiguousarray(b["tiles"])
    if ta.shape != tb.shape or ta.tobytes() != tb.tobytes():
        bad.append("tiles")
    return bad
