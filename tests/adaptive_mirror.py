"""numpy restatement of adaptive sampling (include/rtgl_amd.h, "adaptive sampling"): the shapes, the merge of a one-frame sample image
into the image with a count per tile, the update (snapshot, tile records, every operation in binary32 in the order the header writes, the
sums by error_mirror's tree), the mask rule, the block list, the summary, and a Session that strings them together.  No GPU;
tests/test_adaptive_mirror.py pins it against a scalar restatement, tests/test_gpu_adaptive.py compares the device with it bit for bit."""
import numpy as np

from error_mirror import TILE, f32, lum, tree

DEFAULTS = dict(threshold=0.05, floor=0.01, min_samples=16, max_samples=1024)
TILE_DTYPE = np.dtype([("sum", np.float32), ("mse", np.float32), ("count", np.uint32), ("converged", np.uint32), ("samples", np.uint32),
                       ("samples_snapshot", np.uint32), ("reserved", np.uint32, (2,))])
SUMMARY_INT = ("tiles_total", "tiles_active", "tiles_converged", "tiles_capped", "blocks_active", "samples_min", "samples_max", "converged",
               "samples_total")


def shape(h, w):
    return dict(h=h, w=w, ty=(h + TILE - 1) // TILE, tx=(w + TILE - 1) // TILE, fh=h // 8 * 8, fw=w // 8 * 8, blocks_x=w // 8, blocks_y=h // 8)


def tile_pixels(h, w):
    """(ty, tx): the footprint pixels of every tile"""
    s = shape(h, w)
    ys = np.clip(s["fh"] - np.arange(s["ty"]) * TILE, 0, TILE)
    xs = np.clip(s["fw"] - np.arange(s["tx"]) * TILE, 0, TILE)
    return (ys[:, None] * xs[None, :]).astype(np.uint32)


def explicit_mask(h, w, tiles):
    """an explicit mask: non-zero = active, a tile without footprint pixels stays inactive"""
    s = shape(h, w)
    return ((np.asarray(tiles).reshape(s["ty"], s["tx"]) != 0) & (tile_pixels(h, w) > 0)).astype(np.uint8)


def full_mask(h, w):
    s = shape(h, w)
    return explicit_mask(h, w, np.ones((s["ty"], s["tx"]), np.uint8))


def block_list(h, w, mask):
    """the indices of the footprint's 8 x 8 blocks that lie in active tiles, ascending"""
    s = shape(h, w)
    by, bx = np.mgrid[0:s["blocks_y"], 0:s["blocks_x"]]
    on = np.asarray(mask).reshape(s["ty"], s["tx"])[by // 2, bx // 2] != 0 if by.size else np.zeros((0, 0), bool)
    return (by * s["blocks_x"] + bx)[on].astype(np.uint32)


def tile_list(mask):
    return np.flatnonzero(np.asarray(mask).ravel()).astype(np.uint32)


def slot_pixels(h, w, blocks):
    """(x, y) of every slot of a masked frame's queue 0: slot idx is pixel (in & 7, in >> 3) of block blocks[idx >> 6], in = idx & 63"""
    s = shape(h, w)
    idx = np.arange(64 * len(blocks))
    blk, inn = np.asarray(blocks, np.int64)[idx >> 6], idx & 63
    return (blk % max(s["blocks_x"], 1)) * 8 + (inn & 7), (blk // max(s["blocks_x"], 1)) * 8 + (inn >> 3)


def pixel_tiles(h, w):
    """(h, w): the tile index of every pixel"""
    s = shape(h, w)
    y, x = np.mgrid[0:h, 0:w]
    return (y // TILE) * s["tx"] + x // TILE


def active_pixels(h, w, mask):
    """(h, w) bool: the footprint pixels of the active tiles -- what a masked frame writes"""
    s = shape(h, w)
    on = np.asarray(mask).ravel()[pixel_tiles(h, w)] != 0
    on[s["fh"]:, :] = False
    on[:, s["fw"]:] = False
    return on


def merge(image, sample, n, mask):
    """one masked frame: v = (x + prev (float)k) / (float)(k + 1) per channel, alpha 1, on the footprint pixels of the active tiles, k = n[t];
    then n[t] = k + 1.  Returns (image, n); the inputs are left as they are."""
    image, sample = np.array(image, np.float32), np.asarray(sample, np.float32)
    h, w = image.shape[:2]
    n = np.array(n, np.uint32).reshape(shape(h, w)["ty"], shape(h, w)["tx"])
    on = active_pixels(h, w, mask)
    k = n.ravel()[pixel_tiles(h, w)]
    fk, fk1 = k.astype(np.float32)[..., None], (k + np.uint32(1)).astype(np.float32)[..., None]
    with np.errstate(all="ignore"):
        v = (sample[..., :3] + image[..., :3] * fk) / fk1
    image[..., :3] = np.where(on[..., None], v, image[..., :3])
    image[..., 3] = np.where(on, f32(1.0), image[..., 3])
    return image, n + (np.asarray(mask).reshape(n.shape) != 0).astype(np.uint32)


def update(image, snapshot, n, m, records, threshold=0.05, floor=0.01):
    """the device half of rtgl_adaptive_update: per tile with n > m the snapshot is taken (m == 0) or the record is estimated and the
    snapshot renewed.  Returns (snapshot, m, records); the inputs are left as they are."""
    image = np.asarray(image, np.float32)
    h, w = image.shape[:2]
    s = shape(h, w)
    ty, tx = s["ty"], s["tx"]
    n, m = np.asarray(n, np.uint32).reshape(ty, tx), np.array(m, np.uint32).reshape(ty, tx)
    snapshot, records = np.array(snapshot, np.float32), np.array(records).reshape(ty, tx)
    threshold, floor = f32(threshold), f32(floor)
    per_tile = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)
    with np.errstate(all="ignore"):
        Ln = lum(image)
        d = Ln - snapshot
        den = np.where(Ln > 0, Ln, f32(0.0)).astype(np.float32) + floor
        q = d / den
        e = q * q
        inside = np.zeros((h, w), bool)
        inside[:s["fh"], :s["fw"]] = True
        counts = inside & (e - e == 0)
        padded = np.zeros((ty * TILE, tx * TILE), np.float32)
        padded[:h, :w] = np.where(counts, e, f32(0.0))
        cpad = np.zeros((ty * TILE, tx * TILE), np.uint32)
        cpad[:h, :w] = counts
        total, count = tree(per_tile(padded)), per_tile(cpad).sum(-1, dtype=np.uint32)
        moved, estimated = n > m, (n > m) & (m > 0)
        c = m.astype(np.float32) / np.where(estimated, n - m, 1).astype(np.float32)
        valid = estimated & (count > 0)
        mse = (total / np.where(valid, count, 1).astype(np.float32)) * c
    new = np.zeros((ty, tx), TILE_DTYPE)
    new["sum"], new["mse"] = np.where(valid, total, f32(0.0)), np.where(valid, mse, f32(0.0))
    new["count"], new["converged"] = np.where(valid, count, 0), valid & (mse <= threshold * threshold)
    new["samples"] = new["samples_snapshot"] = n
    records[moved] = new[moved]
    px_moved = inside & moved.ravel()[pixel_tiles(h, w)]
    snapshot[px_moved] = Ln[px_moved]
    m[moved] = n[moved]
    return snapshot, m, records


def done(records):
    return (records["count"] > 0) & (records["converged"] != 0)


def rule(h, w, records, min_samples=16, max_samples=1024):
    """active[t] = n < min_samples or (n < max_samples and not (valid and converged)); a tile without footprint pixels is never active"""
    s = shape(h, w)
    r = np.asarray(records).reshape(s["ty"], s["tx"])
    n = r["samples"]
    return (((n < min_samples) | ((n < max_samples) & ~done(r))) & (tile_pixels(h, w) > 0)).astype(np.uint8)


def summary(h, w, records, mask, max_samples=1024):
    s = shape(h, w)
    r, mask = np.asarray(records).reshape(s["ty"], s["tx"]), np.asarray(mask).reshape(s["ty"], s["tx"])
    px = tile_pixels(h, w)
    has = px > 0
    n, fin = r["samples"][has], done(r)[has]
    valid = has & (r["count"] > 0)
    return dict(tiles_total=int(has.sum()), tiles_active=int((mask[has] != 0).sum()), tiles_converged=int(fin.sum()),
                tiles_capped=int((~fin & (n >= max_samples)).sum()), blocks_active=len(block_list(h, w, mask)),
                samples_min=int(n.min()) if n.size else 0, samples_max=int(n.max()) if n.size else 0, converged=int(not (mask[has] != 0).any()),
                samples_total=int((r["samples"].astype(np.uint64) * px.astype(np.uint64)).sum()),
                max_tile_mse=r["mse"][valid].max() if valid.any() else f32(0.0))


def same_summary(a, b):
    """the names whose values differ, max_tile_mse by its bits"""
    bad = [k for k in SUMMARY_INT if int(a[k]) != int(b[k])]
    if f32(a["max_tile_mse"]).view(np.uint32) != f32(b["max_tile_mse"]).view(np.uint32):
        bad.append("max_tile_mse")
    return bad


class Session:
    """The state of a session: begin() where the context calls rtgl_adaptive_begin, frame(sample) with the FULL one-frame image of the
    frame's uniforms where it calls rtgl_adaptive_frame (only the active pixels are taken from it), update() and set_mask() likewise."""

    def __init__(self, h, w, **params):
        self.h, self.w = h, w
        self.params = dict(DEFAULTS)
        self.params.update(params)
        s = shape(h, w)
        self.image = np.zeros((h, w, 4), np.float32)
        self.snapshot = np.zeros((h, w), np.float32)
        self.n, self.m = np.zeros((s["ty"], s["tx"]), np.uint32), np.zeros((s["ty"], s["tx"]), np.uint32)
        self.records = np.zeros((s["ty"], s["tx"]), TILE_DTYPE)
        self.mask = full_mask(h, w)

    def blocks(self):
        return block_list(self.h, self.w, self.mask)

    def set_mask(self, tiles):
        self.mask = explicit_mask(self.h, self.w, tiles)

    def frame(self, sample):
        self.image, self.n = merge(self.image, sample, self.n, self.mask)

    def update(self):
        self.snapshot, self.m, self.records = update(self.image, self.snapshot, self.n, self.m, self.records, self.params["threshold"], self.params["floor"])
        self.mask = rule(self.h, self.w, self.records, self.params["min_samples"], self.params["max_samples"])
        return summary(self.h, self.w, self.records, self.mask, self.params["max_samples"])
