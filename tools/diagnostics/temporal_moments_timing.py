# GPU time of rtgl_temporal_accumulate with option "temporal_moments" off / 1 / 2 and of rtgl_denoise_guided with option
# "denoise_variance" 0 / 1, next to the frame (the sibling of temporal_timing.py and denoise_guided_timing.py, same method).
# One context with the albedo, normal and position planes on renders warm-up frames, then:
#   * ms per frame: HIP events of rtgl_accumulated_timing over `frames` back-to-back frames;
#   * ms per temporal call: `frames` calls enqueued back to back between two synchronisations, host clock around them (the calls only
#     enqueue, so the window is device time once the queue is full), defaults, three rounds, best of three, per option value:
#       resting: the frame parameters stay put, every call takes the static shortcut (one tap);
#       moving:  the camera position is nudged sideways before every call (rtgl_set_frame_params only: nothing is rendered);
#   * ms per guided call (defaults, "denoise_source" = 1 over a history with mode 2 moments) with "denoise_variance" 0 and 1, the same way;
#   * the traffic models at the 5.2 TB/s streaming rate of DESIGN.md 5.2: the temporal call's 144 B per pixel plus 16 B
#     out and up to 16 B in for the moments, plus 16 B of albedo in mode 2; the prepare kernel's 100 B plus 16 B in.
# usage: python tools/diagnostics/temporal_moments_timing.py [frames] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); ps = [base.replace(frames=f, random=g.rand()) for f in range(1, n + 21)]

ctx = rt.host.Context(W, H)
ctx.set_aov(rt.host.AOV_ALBEDO | rt.host.AOV_NORMAL | rt.host.AOV_POSITION)
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


def window_ms(call):
    for k in range(5):
        call(k)                                           # warm-up: code objects, the buffers, the history after an option change
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        call(k)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def temporal_call(moving):
    def call(k):
        if moving:
            ctx.set_params(nudged[k & 1])
        ctx.temporal_accumulate()
    return call


temporal = {mode: {"resting": [], "moving": []} for mode in (0, 1, 2)}
for _ in range(3):
    for mode in temporal:
        ctx.set_option("temporal_moments", mode)
        for kind in temporal[mode]:
            ctx.set_params(last)
            temporal[mode][kind].append(window_ms(temporal_call(kind == "moving")))
ctx.set_option("temporal_moments", 2)
ctx.set_params(last)
for k in range(8):
    ctx.temporal_accumulate()                             # a history long enough for the temporal estimate to be taken
ctx.set_option("denoise_source", 1)
guided = {0: [], 1: []}
for _ in range(3):
    for tv in guided:
        ctx.set_option("denoise_variance", tv)
        guided[tv].append(window_ms(lambda k: ctx.denoise_guided()))
moments = ctx.read_temporal_moments()
ctx.close()
rate = 5.2e12
model = {0: 144.0, 1: 176.0, 2: 192.0}
best = lambda v: round(min(v), 4)
print(json.dumps({"config": name, "frames": n, "calls_per_window": n, "ms_per_frame": round(frame_ms, 4),
                  "temporal_ms_per_call": {f"moments_{m}": {k: [round(x, 4) for x in v] for k, v in kinds.items()} for m, kinds in temporal.items()},
                  "temporal_ms_best": {f"moments_{m}": {k: best(v) for k, v in kinds.items()} for m, kinds in temporal.items()},
                  "temporal_traffic_model_ms": {f"moments_{m}": round(b * W * H / rate * 1e3, 4) for m, b in model.items()},
                  "temporal_call_over_frame": {f"moments_{m}": {k: round(min(v) / frame_ms, 4) for k, v in kinds.items()} for m, kinds in temporal.items()},
                  "guided_ms_per_call": {f"denoise_variance_{tv}": [round(x, 4) for x in v] for tv, v in guided.items()},
                  "guided_ms_best": {f"denoise_variance_{tv}": best(v) for tv, v in guided.items()},
                  "prepare_traffic_model_extra_ms": round(16.0 * W * H / rate * 1e3, 4),
                  "guided_call_over_frame": {f"denoise_variance_{tv}": round(min(v) / frame_ms, 4) for tv, v in guided.items()},
                  "share_of_pixels_with_history_of_4_or_more": round(float((moments[..., 3] >= 4).mean()), 4)}), flush=True)
