# GPU time of rtgl_denoise_guided next to rtgl_denoise and the frame they clean (the sibling of denoise_timing.py, same method).  One
# context with the guide planes on renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only enqueue, so
#     the window is device time once the queue is full): rtgl_denoise_guided for passes = 0..5 (0: the prepare kernel alone) and
#     rtgl_denoise at its defaults, three rounds, the settings alternating, best of three;
#   * ms per pass: the increments between consecutive pass counts (pass L has step 2^L);
#   * the ratio to the traffic floor at the 5.2 TB/s streaming rate of DESIGN.md 5.2: per pixel a pass reads 48 B of records and guides
#     and 4 B of neighbour marks and writes 16 B; the prepare kernel reads 64 B and writes 36 B.
# usage: python tools/diagnostics/denoise_guided_timing.py [frames] [config]
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


def calls_ms(call):
    for _ in range(5):
        call()                                            # warm-up: code objects, the scratch buffers
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


res = {k: [] for k in range(0, 6)}
plain = []
for _ in range(3):
    for k in res:
        res[k].append(calls_ms(lambda: ctx.denoise_guided(passes=k)))
    plain.append(calls_ms(ctx.denoise))
ctx.close()
best = {k: min(v) for k, v in res.items()}
per_pass = [best[k] - best[k - 1] for k in range(1, 6)]
floor_pass, floor_prepare = 68.0 * W * H / 5.2e12 * 1e3, 100.0 * W * H / 5.2e12 * 1e3
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "guided_ms_per_call_by_passes": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "guided_ms_per_default_call": round(best[5], 4), "guided_ms_prepare": round(best[0], 4),
                  "guided_ms_per_pass_step_1_2_4_8_16": [round(x, 4) for x in per_pass], "guided_ms_per_pass_mean": round((best[5] - best[0]) / 5, 4),
                  "traffic_floor_ms_per_pass": round(floor_pass, 4), "traffic_floor_ms_prepare": round(floor_prepare, 4),
                  "pass_ratio_to_traffic_floor": round((best[5] - best[0]) / 5 / floor_pass, 2), "prepare_ratio_to_traffic_floor": round(best[0] / floor_prepare, 2),
                  "denoise_ms_per_default_call": [round(x, 4) for x in plain], "guided_over_denoise": round(best[5] / min(plain), 3),
                  "guided_call_over_frame": round(best[5] / frame_ms, 3)}), flush=True)
