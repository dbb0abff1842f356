# GPU time of rtgl_robust_denoise next to the two calls it replaces and to the frame, from one run.
# One context, planes on, warm-up, then for every case `calls` calls enqueued back to back between two synchronisations, host clock around
# them (the calls only enqueue, so the window is device time once the queue is full).  For K = 4 / 8 / 16 and passes 0 / 5 the two routes
# take turns, three rounds each (new, old, new, old, ...), best of three:
#   * new: rtgl_robust_denoise;
#   * old: rtgl_robust_resolve into the image, then rtgl_denoise_guided with the same passes and the clamp off.
# With passes = 0 the new call is its prepare kernel alone (bucket_guide_kernel); rtgl_robust_error_estimate of the same K (the kernel that
# reads the same 16 K bytes per pixel, and a one-block solve) stands beside it, both with the bytes they move per second: for the new kernel
# 16 K of buckets, 48 of planes, 36 (passes = 0) of stores per pixel, the halo of the guides not counted; for the estimate 16 K per
# footprint pixel.  "spread" is the largest (max - min) / min over the three rounds of any case.
# usage: python tools/diagnostics/robust_denoise_timing.py [calls] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(64)]
BUCKETS, PASSES = (4, 8, 16), (0, 5)
FOOT = (W // 8 * 8) * (H // 8 * 8)
AOV = rt.host.AOV_ALBEDO | rt.host.AOV_NORMAL | rt.host.AOV_POSITION

ctx = rt.host.Context(W, H)
ctx.upload_scene(scene)
ctx.set_aov(AOV)


def frame(k):
    ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k % len(randoms)]), sync=False)


def one_window(call):
    t0 = time.perf_counter()
    for k in range(n):
        call(k)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def alternated(calls, rounds=3):
    """{name: [ms per call of every round]}, the cases taking turns"""
    for call in calls.values():
        for k in range(10):
            call(k)                                       # warm-up: buffers, code objects
    ctx.synchronize()
    out = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            out[k].append(one_window(call))
    return out


def old_route(passes):
    def call(k):
        ctx.robust_resolve(dest=rt.host.ROBUST_DEST_IMAGE)
        ctx.denoise_guided(passes=passes, firefly_ratio=0.0)
    return call


res = alternated({"frame": frame})
for K in BUCKETS:
    ctx.robust_begin(buckets=K)
    for k in range(2 * K):                                # every bucket holds rendered frames
        frame(k)
        ctx.robust_accumulate()
    cases = {}
    for passes in PASSES:
        cases[f"robust_denoise K = {K} passes = {passes}"] = (lambda p: lambda k: ctx.robust_denoise(passes=p))(passes)
        cases[f"resolve + denoise_guided K = {K} passes = {passes}"] = old_route(passes)
    cases[f"robust_resolve image K = {K}"] = lambda k: ctx.robust_resolve(dest=rt.host.ROBUST_DEST_IMAGE)
    cases[f"robust_error_estimate K = {K}"] = lambda k: ctx.robust_error_estimate()
    res.update(alternated(cases))
ctx.robust_end()
ctx.close()

best = {k: min(v) for k, v in res.items()}
spread = max((max(v) - min(v)) / min(v) for v in res.values())
new_bytes = {K: (16.0 * K + 48.0 + 36.0) * W * H for K in BUCKETS}
rate = {f"bucket_guide K = {K}": round(new_bytes[K] / (best[f"robust_denoise K = {K} passes = 0"] * 1e-3) / 1e12, 3) for K in BUCKETS}
rate.update({f"robust_error_estimate K = {K}": round(16.0 * K * FOOT / (best[f"robust_error_estimate K = {K}"] * 1e-3) / 1e12, 3) for K in BUCKETS})
print(json.dumps({"config": name, "calls_per_window": n, "ms_per_call_rounds": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_call": {k: round(v, 4) for k, v in best.items()},
                  "new_over_old": {f"K = {K} passes = {p}": round(best[f"robust_denoise K = {K} passes = {p}"] / best[f"resolve + denoise_guided K = {K} passes = {p}"], 3)
                                   for K in BUCKETS for p in PASSES},
                  "terabytes_per_second": rate, "spread": round(spread, 4)}), flush=True)
