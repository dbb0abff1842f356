# GPU time of rtgl_temporal_accumulate next to the frame whose history it carries (the sibling of denoise_guided_timing.py, same method).
# One context with the normal and position planes on renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only enqueue, so
#     the window is device time once the queue is full), defaults, three rounds, best of three:
#       resting: the frame parameters stay put, every call takes the static shortcut (one tap);
#       moving:  the camera position is nudged sideways before every call (rtgl_set_frame_params only: nothing is rendered, the image
#                and the planes stay the last frame's, the reprojection has its four taps and its tests to do);
#   * the ratio to the traffic model at the 5.2 TB/s streaming rate of DESIGN.md 5.2: per pixel 48 B in (image and two planes), up to
#     48 B of previous records (one tap's worth: neighbouring lanes share the rest) and 48 B out.
# usage: python tools/diagnostics/temporal_timing.py [frames] [config]
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
last = ps[-1]
px, py, pz = last.camera_position
rx, ry, rz = last.camera_right
nudged = [last.replace(camera_position=(px + 0.01 * (k % 7 + 1) * rx, py + 0.01 * (k % 7 + 1) * ry, pz + 0.01 * (k % 7 + 1) * rz)) for k in range(2)]


def calls_ms(moving):
    def call(k):
        if moving:
            ctx.set_params(nudged[k & 1])
        ctx.temporal_accumulate()
    ctx.set_params(last)
    for k in range(5):
        call(k)                                           # warm-up: code objects, the history buffers
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        call(k)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


res = {"resting": [], "moving": []}
for _ in range(3):
    for kind in res:
        res[kind].append(calls_ms(kind == "moving"))
hist = ctx.read_temporal()
ctx.close()
floor = 144.0 * W * H / 5.2e12 * 1e3
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "temporal_ms_per_call": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "temporal_ms_resting": round(min(res["resting"]), 4), "temporal_ms_moving": round(min(res["moving"]), 4),
                  "traffic_model_ms": round(floor, 4),
                  "resting_ratio_to_traffic_model": round(min(res["resting"]) / floor, 2), "moving_ratio_to_traffic_model": round(min(res["moving"]) / floor, 2),
                  "moving_call_over_frame": round(min(res["moving"]) / frame_ms, 4), "resting_call_over_frame": round(min(res["resting"]) / frame_ms, 4),
                  "mean_history_length_at_the_end": round(float(hist[..., 3].mean()), 2)}), flush=True)
