# GPU time of rtgl_denoise next to the frame it cleans.  One context with the guide planes on renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames (as aov_timing.py);
#   * ms per rtgl_denoise call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only
#     enqueue, so the window is device time once the queue is full), for passes = 1..5 and the defaults, three rounds, the settings alternating;
#   * ms per pass: the increments between consecutive pass counts (pass L has step 2^L, so the passes differ in how far their taps reach);
#   * the ratio to the traffic floor: 64 B per pixel and pass (48 in, 16 out) at the 5.2 TB/s streaming rate of DESIGN.md 5.2.
# usage: python tools/diagnostics/denoise_timing.py [frames] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); ps = [base.replace(frames=f, random=g.rand()) for f in range(1, n + 21)]
GUIDES = rt.host.AOV_ALBEDO | rt.host.AOV_NORMAL | rt.host.AOV_POSITION

ctx = rt.host.Context(W, H)
ctx.set_aov(GUIDES)
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


def calls_ms(passes):
    for _ in range(5):
        ctx.denoise(passes=passes)                        # warm-up: code objects, the scratch buffers
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        ctx.denoise(passes=passes)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


res = {k: [] for k in range(1, 6)}
for _ in range(3):
    for k in res:
        res[k].append(calls_ms(k))
ctx.close()
best = {k: min(v) for k, v in res.items()}
per_pass = [best[1]] + [best[k] - best[k - 1] for k in range(2, 6)]
floor_ms = 64.0 * W * H / 5.2e12 * 1e3
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "ms_per_call_by_passes": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_default_call": round(best[5], 4), "ms_per_pass_step_1_2_4_8_16": [round(x, 4) for x in per_pass],
                  "ms_per_pass_mean": round(best[5] / 5, 4), "traffic_floor_ms_per_pass": round(floor_ms, 4),
                  "ratio_to_traffic_floor": round(best[5] / 5 / floor_ms, 2), "call_over_frame": round(best[5] / frame_ms, 3)}), flush=True)
