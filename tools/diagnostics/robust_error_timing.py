# GPU time of rtgl_robust_error_estimate next to the frame and to rtgl_robust_resolve of the same K, from one run.
# One context, warm-up, then for every case `calls` calls enqueued back to back between two synchronisations, host clock around them (the
# calls only enqueue, so the window is device time once the queue is full), three rounds, best of three:
#   * the ordinary frame as it runs by default;
#   * rtgl_robust_resolve for K = 4 / 8 / 16 into the output plane;
#   * rtgl_robust_error_estimate for K = 4 / 8 / 16 (the tile kernel and the one-block solve behind it).
# Beside them the byte models at the 5.2 TB/s streaming rate of DESIGN.md 5.4: 16 K + 16 B per pixel for the resolve; for the estimate
# 12 K B per footprint pixel (the loads are narrowed to the three colours) and 16 K B (whole float4 lines).  "spread" is the run-to-run
# spread of this script: the largest (max - min) / min over the three rounds of any case.
# usage: python tools/diagnostics/robust_error_timing.py [calls] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(n + 20)]
BUCKETS = (4, 8, 16)
FOOT = (W // 8 * 8) * (H // 8 * 8)
model = {f"robust_resolve K = {K}": (16.0 * K + 16.0) * W * H / 5.2e12 * 1e3 for K in BUCKETS}
model.update({f"robust_error_estimate K = {K}": 12.0 * K * FOOT / 5.2e12 * 1e3 for K in BUCKETS})
model_wide = {f"robust_error_estimate K = {K}": 16.0 * K * FOOT / 5.2e12 * 1e3 for K in BUCKETS}

ctx = rt.host.Context(W, H)
ctx.upload_scene(scene)


def window(call, rounds=3):
    for k in range(20):
        call(k)                                           # warm-up: buffers, code objects
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for k in range(n):
            call(20 + k)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def frame(k):
    ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)


res = {"frame": window(frame)}
for K in BUCKETS:
    ctx.robust_begin(buckets=K)
    for k in range(K):                                    # every bucket holds a rendered frame
        frame(k)
        ctx.robust_accumulate()
    res[f"robust_resolve K = {K}"] = window(lambda k: ctx.robust_resolve())
    res[f"robust_error_estimate K = {K}"] = window(lambda k: ctx.robust_error_estimate())
    summary = ctx.read_robust_error_summary()
    assert summary["valid"] == 1 and summary["frames_now"] == K
ctx.robust_end()
ctx.close()

best = {k: min(v) for k, v in res.items()}
spread = max((max(v) - min(v)) / min(v) for v in res.values())
print(json.dumps({"config": name, "calls_per_window": n, "ms_per_call_rounds": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_call": {k: round(v, 4) for k, v in best.items()}, "traffic_model_ms": {k: round(v, 5) for k, v in model.items()},
                  "traffic_model_16K_ms": {k: round(v, 5) for k, v in model_wide.items()},
                  "measured_over_model": {k: round(v / model[k], 3) for k, v in best.items() if k != "frame"},
                  "estimate_over_resolve": {K: round(best[f"robust_error_estimate K = {K}"] / best[f"robust_resolve K = {K}"], 3) for K in BUCKETS},
                  "spread": round(spread, 4)}), flush=True)
