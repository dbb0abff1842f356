# GPU time of rtgl_temporal_clip next to the frame whose history it clamps (the sibling of temporal_timing.py, same method).
# One context with the normal and position planes on renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only enqueue, so
#     the window is device time once the queue is full), three rounds, best of three: the defaults, both geometric terms off, and the
#     defaults with option "temporal_moments" = 1 (the length also goes to the moments record).  After the first call of a round the
#     clip is the identity, which costs what any call costs: the kernel has no data-dependent path but the selects;
#   * the ratio to the traffic model at the 5.2 TB/s streaming rate of DESIGN.md 5.4: per pixel 48 B in (image and two planes) and 16 B
#     of history in and out, 80 B; 96 B with the moments record.
# usage: python tools/diagnostics/temporal_clip_timing.py [frames] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); ps = [base.replace(frames=f, random=g.rand()) for f in range(1, n + 21)]

ctx = rt.host.Context(W, H)
ctx.set_aov(rt.host.AOV_NORMAL | rt.host.AOV_POSITION)
ctx.upload_scene(scene)
for p in ps[:20]:
    ctx.render(p, sync=False)                             # warm-up: buffers, grid estimates
ctx.synchronize()
ctx.set_option("kernel_timing", 1)
ctx.timing_reset()
for p in ps[20:]:
    ctx.render(p, sync=False)
t = ctx.accumulated_timing()
frame_ms = t["frame_ms"] / max(t["frames"], 1)
ctx.set_option("kernel_timing", 0)


def calls_ms(moments, **params):
    ctx.set_option("temporal_moments", moments)
    ctx.temporal_accumulate()                             # the history this round clamps
    for k in range(5):
        ctx.temporal_clip(**params)                       # warm-up: code objects
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        ctx.temporal_clip(**params)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


kinds = {"defaults": (0, {}), "terms_off": (0, dict(sigma_normal=0.0, sigma_position=0.0)), "defaults_with_moments": (1, {})}
res = {k: [] for k in kinds}
for _ in range(3):
    for kind, (moments, params) in kinds.items():
        res[kind].append(calls_ms(moments, **params))
hist = ctx.read_temporal()
ctx.close()
floor, floor_m = 80.0 * W * H / 5.2e12 * 1e3, 96.0 * W * H / 5.2e12 * 1e3
best = {k: min(v) for k, v in res.items()}
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "clip_ms_per_call": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "clip_ms": {k: round(v, 4) for k, v in best.items()},
                  "traffic_model_ms": round(floor, 4), "traffic_model_with_moments_ms": round(floor_m, 4),
                  "ratio_to_traffic_model": {"defaults": round(best["defaults"] / floor, 2), "terms_off": round(best["terms_off"] / floor, 2),
                                             "defaults_with_moments": round(best["defaults_with_moments"] / floor_m, 2)},
                  "call_over_frame": {k: round(v / frame_ms, 4) for k, v in best.items()},
                  "mean_history_length_at_the_end": round(float(hist[..., 3].mean()), 2)}), flush=True)
