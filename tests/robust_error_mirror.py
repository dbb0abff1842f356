"""numpy restatement of rtgl_robust_error_estimate (include/rtgl_amd.h, "robust error estimate"): keys, ranks, G and t from
robust_mirror, the winsorized keys, Yuen's variance of the trimmed mean and the relative error per pixel, every operation in binary32 in
the order the header writes; the tile sums, the records and the whole-picture solve by error_mirror's tree.  No GPU;
tests/test_robust_error_mirror.py pins it against a scalar restatement, tests/test_gpu_robust_error.py compares the device with it bit
for bit."""
import numpy as np

import error_mirror as em
import robust_mirror as rm

f32 = np.float32
DEFAULTS = dict(threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950)
TILE, TILE_DTYPE = em.TILE, em.TILE_DTYPE


def valid_params(threshold, floor, gain, quantile_permille, flags=0, reserved=(0,) * 3):
    with np.errstate(over="ignore"):
        threshold, floor, gain = f32(threshold), f32(floor), f32(gain)      # (the record holds binary32)
    return bool(np.isfinite(threshold) and threshold > 0 and np.isfinite(floor) and floor > 0 and np.isfinite(gain) and gain >= 0
                and 1 <= quantile_permille <= 1000 and flags == 0 and not any(reserved))


def refused(session, N, K):
    """RTGL_ERR_STATE: no session, or a bucket without a sample"""
    return not session or N < K


def pixel_error(planes, N, gain=1.0, floor=0.01):
    """steps 1-9 for planes (K, h, w, 4) after N >= K frames: (e (h, w) binary32, counts (h, w) bool; the footprint is not applied)"""
    planes = np.asarray(planes, f32)
    K = planes.shape[0]
    assert K in rm.BUCKETS and N >= K
    key, rank, G = rm.gini(planes)
    t = rm.trim(G, gain, K, N)
    floor = f32(floor)
    with np.errstate(all="ignore"):
        lo = np.zeros(G.shape, f32)
        hi = np.zeros(G.shape, f32)
        for j in range(K):
            lo = np.where(rank[j] == t, key[j], lo)
            hi = np.where(rank[j] == K - 1 - t, key[j], hi)
        w = []
        for j in range(K):
            wj = np.where(key[j] < lo, lo, key[j]).astype(f32)
            w.append(np.where(wj > hi, hi, wj).astype(f32))
        kept = [(t <= rank[j]) & (rank[j] <= K - 1 - t) for j in range(K)]
        h = (K - 2 * t).astype(np.int32)
        M = np.zeros(G.shape, f32)
        T = np.zeros(G.shape, f32)
        for j in range(K):
            M = M + w[j]
            T = np.where(kept[j], T + key[j], T).astype(f32)
        mw = M / f32(K)
        D = np.zeros(G.shape, f32)
        for j in range(K):
            d = w[j] - mw
            D = D + d * d
        mu = T / h.astype(f32)
        v = D / (h * (h - 1)).astype(f32)
        den = np.where(mu > 0, mu, f32(0)).astype(f32) + floor
        e = (v / (den * den)).astype(f32)
        counts = (e - e == 0)
    return e, counts


def estimate(planes, N, threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950):
    """One estimate of a session's planes (K, h, w, 4) after N >= K frames: the summary's fields and "tiles", a structured array (ty, tx),
    laid out like error_mirror.estimate's result (em.same_result compares two)."""
    planes = np.asarray(planes, f32)
    h, w = planes.shape[1:3]
    fh, fw = h // 8 * 8, w // 8 * 8
    ty, tx = em.tiles_of(h, w)
    e, counts = pixel_error(planes, N, gain, floor)
    threshold = f32(threshold)
    inside = np.zeros((h, w), bool)
    inside[:fh, :fw] = True
    counts = inside & counts
    with np.errstate(all="ignore"):
        padded = np.zeros((ty * TILE, tx * TILE), f32)
        padded[:h, :w] = np.where(counts, e, f32(0))
        cpad = np.zeros((ty * TILE, tx * TILE), np.uint32)
        cpad[:h, :w] = counts
        per_tile = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)
        tiles = np.zeros((ty, tx), TILE_DTYPE)
        tiles["sum"] = em.tree(per_tile(padded))
        tiles["count"] = per_tile(cpad).sum(-1, dtype=np.uint32)
        valid = tiles["count"] > 0
        mse = (tiles["sum"] / np.where(valid, tiles["count"], 1).astype(f32)).astype(f32)
        tiles["mse"] = np.where(valid, mse, f32(0))
        tiles["converged"] = valid & (mse <= threshold * threshold)
        tiles["sum"] = np.where(valid, tiles["sum"], f32(0))
        # the whole picture: error_mirror's solve with c = 1
        flat = tiles["sum"].ravel()
        rows = -(-len(flat) // 256)
        lanes_in = np.zeros(rows * 256, f32)
        lanes_in[:len(flat)] = flat
        lanes = np.zeros(256, f32)
        for row in lanes_in.reshape(rows, 256):
            lanes = lanes + row
        total = em.tree(lanes)
        n = int(tiles["count"].sum(dtype=np.uint64))
        out = dict(valid=1, frames_now=int(np.int32(np.uint32(N))), frames_snapshot=0, tiles_valid=int(valid.sum()), tiles_converged=int(tiles["converged"].sum()),
                   pixels_ignored=(fh * fw - n) & 0xFFFFFFFF, scale=f32(1), mse=(total / f32(np.uint64(n))) * f32(1) if n else f32(0),
                   max_tile_mse=tiles["mse"][valid].max() if valid.any() else f32(0), tiles=tiles)
    out["converged"] = int(out["tiles_valid"] > 0 and out["tiles_converged"] * 1000 >= out["tiles_valid"] * int(quantile_permille))
    return out


def render_until(frame, K, threshold, max_frames, check_every=16, gain=1.0, **params):
    """HeadlessRenderer.render_robust_until written out: frame(k) gives the k-th one-sample image.  Returns (frames, the latest summary or
    None, the session)"""
    first = frame(0)
    sess = rm.Session(first.shape[0], first.shape[1], K)
    done, summary = 0, None
    while done < max_frames:
        for _ in range(min(check_every, max_frames - done)):
            sess.accumulate(first if done == 0 else frame(done))
            done += 1
        if done >= K:
            summary = estimate(sess.planes, sess.N, threshold=threshold, gain=gain, **params)
            if summary["valid"] and summary["converged"]:
                break
    return done, summary, sess
