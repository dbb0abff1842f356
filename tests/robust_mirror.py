"""numpy restatement of robust accumulation (include/rtgl_amd.h, "robust accumulation"): the fold of a one-sample image into the bucket of
the next frame, the counts, and the resolve -- luminance keys, ranks by counting, the Gini coefficient, the trim and the weighted mean
of the kept buckets, every operation in binary32 in the order the header writes -- and a Session that strings them together.  No GPU;
tests/test_robust_mirror.py pins it against a scalar restatement, tests/test_gpu_robust.py compares the device with it bit for bit."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(buckets=8, gain=1.0, dest=0)
DEST_BUFFER, DEST_IMAGE = 0, 1
BUCKETS = (4, 8, 16)
INF = f32(np.inf)


def lum(rgb):
    """(0.25 r + 0.5 g) + 0.25 b: lum of rtgl_error_estimate"""
    rgb = np.asarray(rgb, f32)
    return (f32(0.25) * rgb[..., 0] + f32(0.5) * rgb[..., 1]) + f32(0.25) * rgb[..., 2]


def next_bucket(N, K):
    return N % K


def next_count(N, K):
    return N // K


def bucket_samples(N, K):
    """n_j for j = 0 .. K - 1 after N frames"""
    return np.array([N // K + (1 if j < N % K else 0) for j in range(K)], np.int64)


def trim_cap(K):
    return (K - 1) // 2


def valid_params(buckets, flags=0, reserved=(0,) * 6):
    return buckets in BUCKETS and flags == 0 and not any(reserved)


def valid_resolve_params(gain, dest, flags=0, reserved=(0,) * 5):
    with np.errstate(over="ignore"):
        gain = f32(gain)                                           # (the record holds a binary32: 1e39 is +inf there)
    return bool(np.isfinite(gain)) and gain >= 0 and dest in (DEST_BUFFER, DEST_IMAGE) and flags == 0 and not any(reserved)


def fold(bucket, x, k):
    """b' = (x + b (float)k) / (float)(k + 1), all four components"""
    with np.errstate(all="ignore"):
        return ((np.asarray(x, f32) + np.asarray(bucket, f32) * f32(k)) / f32(k + 1)).astype(f32)


def gini(planes):
    """steps 1-6 for planes (K, ..., 4): keys, ranks and G"""
    planes = np.asarray(planes, f32)
    K = planes.shape[0]
    with np.errstate(all="ignore"):
        l = lum(planes[..., :3])
        key = np.where(np.isfinite(l), l, INF).astype(f32)
        rank = np.zeros(key.shape, np.int32)
        for j in range(K):
            for i in range(K):
                if i != j:
                    rank[j] += (key[i] < key[j]) | ((key[i] == key[j]) & (i < j))
        S = np.zeros(key.shape[1:], f32)
        A = np.zeros(key.shape[1:], f32)
        for j in range(K):
            S = S + key[j]
            A = A + (2 * rank[j] - (K - 1)).astype(f32) * key[j]
        G = np.where(~np.isfinite(S), f32(1), np.where(~(S > 0), f32(0), A / (f32(K) * S))).astype(f32)
        G = np.where(~(G <= 1), f32(1), G).astype(f32)
        G = np.where(~(G >= 0), f32(0), G).astype(f32)
    return key, rank, G


def trim(G, gain, K, N):
    """step 7: t per pixel"""
    cap = trim_cap(K)
    with np.errstate(all="ignore"):
        u = (G * f32(gain)) * f32(K // 2)
        t = np.where(u >= f32(cap), cap, np.where(u >= f32(cap), 0, u).astype(np.int32)).astype(np.int32)
    return t if N >= K else np.zeros_like(t)


def resolve(planes, N, gain=1.0):
    """steps 1-9: (out (..., 4) with every component of the weighted mean, G (...), t (...)) for planes (K, ..., 4) after N >= 1 frames"""
    planes = np.asarray(planes, f32)
    K = planes.shape[0]
    assert K in BUCKETS and N >= 1
    _, rank, G = gini(planes)
    t = trim(G, gain, K, N)
    n = bucket_samples(N, K)
    W = np.zeros(G.shape, f32)
    Csum = np.zeros(G.shape + (4,), f32)
    with np.errstate(all="ignore"):
        for j in range(K):
            if n[j] == 0:
                continue
            keep = (t <= rank[j]) & (rank[j] <= K - 1 - t)
            W = np.where(keep, W + f32(n[j]), W).astype(f32)
            Csum = np.where(keep[..., None], Csum + f32(n[j]) * planes[j], Csum).astype(f32)
        out = (Csum / W[..., None]).astype(f32)
    return out, G, t


def output_plane(planes, N, gain=1.0):
    """what dest = BUFFER stores: {out.x, out.y, out.z, G}"""
    out, G, _ = resolve(planes, N, gain)
    return np.concatenate([out[..., :3], G[..., None]], -1).astype(f32)


def image_plane(planes, N, gain=1.0):
    """what dest = IMAGE stores: out, all four components"""
    return resolve(planes, N, gain)[0]


class Session:
    """rtgl_robust_begin / _accumulate / _resolve over images of one shape"""

    def __init__(self, h, w, buckets=DEFAULTS["buckets"]):
        assert valid_params(buckets)
        self.K, self.N = buckets, 0
        self.planes = np.zeros((buckets, h, w, 4), f32)

    def accumulate(self, image):
        j, k = next_bucket(self.N, self.K), next_count(self.N, self.K)
        self.planes[j] = fold(self.planes[j], image, k)
        self.N += 1

    def resolve(self, gain=DEFAULTS["gain"], dest=DEST_BUFFER):
        assert valid_resolve_params(gain, dest) and self.N >= 1
        return (image_plane if dest == DEST_IMAGE else output_plane)(self.planes, self.N, gain)
