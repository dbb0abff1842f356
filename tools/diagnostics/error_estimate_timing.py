# GPU time of rtgl_error_estimate next to the frame whose image it judges (the sibling of tonemap_timing.py, same method).
# One context renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only enqueue, so
#     the window is device time once the queue is full), three rounds, best of three.  Calls repeated without a frame in between can be
#     of two kinds only: with the keep flag every call estimates against the same snapshot (error_tiles_kernel<1, 1>: 16 B of image and
#     4 B of snapshot read per pixel, and the solve); without it every call after the first finds F_n == F_m and only takes a snapshot
#     (error_tiles_kernel<0, 0>: 16 B read, 4 B written, and the solve).  The default call between frames (error_tiles_kernel<1, 0>) does
#     both, 24 B per pixel; it cannot be repeated without rendering and is not timed here;
#   * the ratio to the traffic model at the 5.2 TB/s streaming rate of DESIGN.md 5.4;
#   * the summary of the estimate itself, and rtgl_read_error_summary on the host clock (it synchronises).
# usage: python tools/diagnostics/error_estimate_timing.py [frames] [config]
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
ctx.error_estimate()                                      # the snapshot: 20 frames
ctx.synchronize()
ctx.set_option("kernel_timing", 1)
ctx.timing_reset()
for p in ps[20:]:
    ctx.render(p, sync=False)
t = ctx.accumulated_timing()
frame_ms = t["frame_ms"] / max(t["frames"], 1)
ctx.set_option("kernel_timing", 0)
ctx.error_estimate(keep_snapshot=True)                    # the estimate: n + 20 frames against 20
summary = ctx.read_error_summary()


def calls_ms(**params):
    for k in range(5):
        ctx.error_estimate(**params)                      # warm-up: code objects
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        ctx.error_estimate(**params)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def readout_ms(read):
    read()
    t0 = time.perf_counter()
    for k in range(20):
        read()
    return (time.perf_counter() - t0) * 1e3 / 20


kinds = {"estimate_keep": dict(keep_snapshot=True), "snapshot_only": dict()}
res = {k: [] for k in kinds}
for _ in range(3):
    res["estimate_keep"].append(calls_ms(keep_snapshot=True))
for _ in range(3):
    res["snapshot_only"].append(calls_ms())               # (the first of them estimates and moves the snapshot; it is among the warm-up calls)
read_ms = min(readout_ms(ctx.read_error_summary) for _ in range(3))
ctx.close()
model = {"estimate_keep": 20.0, "snapshot_only": 20.0, "default_between_frames": 24.0}
floor_ms = {k: b * W * H / 5.2e12 * 1e3 for k, b in model.items()}
best = {k: min(v) for k, v in res.items()}
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "error_estimate_ms_per_call": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "error_estimate_ms": {k: round(v, 4) for k, v in best.items()},
                  "traffic_model_bytes_per_pixel": model, "traffic_model_ms": {k: round(v, 4) for k, v in floor_ms.items()},
                  "ratio_to_traffic_model": {k: round(best[k] / floor_ms[k], 2) for k in best},
                  "call_over_frame": {k: round(v / frame_ms, 5) for k, v in best.items()},
                  "read_error_summary_ms": round(read_ms, 4),
                  "summary": {k: (int(v) if isinstance(v, int) else float(v)) for k, v in summary.items()}}), flush=True)
