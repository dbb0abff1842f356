# GPU time of rtgl_tonemap next to the frame whose buffer it displays (the sibling of temporal_clip_timing.py, same method).
# One context renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only enqueue, so
#     the window is device time once the queue is full), three rounds, best of three: the defaults (histogram, solve, map), manual
#     exposure (map only), and the defaults with the ACES fit;
#   * the ratio to the traffic model at the 5.2 TB/s streaming rate of DESIGN.md 5.4: per pixel 16 B read by the histogram, 16 B read and
#     4 B written by the map: 36 B with auto exposure, 20 B without;
#   * rtgl_read_image_u8 and rtgl_read_display_u8, ms per call on the host clock (each synchronises): both copy 4 B per pixel to the host,
#     the first launches its conversion kernel before the copy, the second only copies: the difference is that launch.
# usage: python tools/diagnostics/tonemap_timing.py [frames] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); ps = [base.replace(frames=f, random=g.rand()) for f in range(1, n + 21)]

ctx = rt.host.Context(W, H)
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


def calls_ms(**params):
    for k in range(5):
        ctx.tonemap(**params)                             # warm-up: code objects, the display buffer
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        ctx.tonemap(**params)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def readout_ms(read):
    read()
    t0 = time.perf_counter()
    for k in range(20):
        read()
    return (time.perf_counter() - t0) * 1e3 / 20


kinds = {"defaults": {}, "manual_exposure": dict(auto=False, exposure=0.5), "defaults_aces": dict(op=2)}
res = {k: [] for k in kinds}
for _ in range(3):
    for kind, params in kinds.items():
        res[kind].append(calls_ms(**params))
ctx.tonemap()
exposure = float(ctx.read_tonemap_exposure())
hist, ignored = ctx.read_tonemap_histogram()
u8 = min(readout_ms(ctx.read_image_u8) for _ in range(3))
disp = min(readout_ms(ctx.read_display) for _ in range(3))
mean_code = float(ctx.read_display()[..., :3].mean())
ctx.close()
floor_auto, floor_manual = 36.0 * W * H / 5.2e12 * 1e3, 20.0 * W * H / 5.2e12 * 1e3
best = {k: min(v) for k, v in res.items()}
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "tonemap_ms_per_call": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "tonemap_ms": {k: round(v, 4) for k, v in best.items()},
                  "traffic_model_ms": {"auto": round(floor_auto, 4), "manual": round(floor_manual, 4)},
                  "ratio_to_traffic_model": {"defaults": round(best["defaults"] / floor_auto, 2), "manual_exposure": round(best["manual_exposure"] / floor_manual, 2),
                                             "defaults_aces": round(best["defaults_aces"] / floor_auto, 2)},
                  "call_over_frame": {k: round(v / frame_ms, 4) for k, v in best.items()},
                  "read_image_u8_ms": round(u8, 4), "read_display_u8_ms": round(disp, 4), "read_image_u8_conversion_launch_ms": round(u8 - disp, 4),
                  "exposure": exposure, "counted_pixels": int(hist.sum()), "ignored_pixels": ignored, "mean_display_code": round(mean_code, 2)}), flush=True)
