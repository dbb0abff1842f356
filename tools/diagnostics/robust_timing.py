# GPU time of the two calls of robust accumulation (rtgl_robust_accumulate, rtgl_robust_resolve) next to the frame.
# One context, warm-up, then for every case `calls` calls enqueued back to back between two synchronisations, host clock around them (the
# calls only enqueue, so the window is device time once the queue is full), three rounds, best of three:
#   * the ordinary frame as it runs by default;
#   * rtgl_robust_accumulate for K = 4 / 8 / 16 (the fold does not depend on K but for the plane it lands in);
#   * rtgl_robust_resolve for K = 4 / 8 / 16 into the output plane and into the image.
# Beside them the byte models at the 5.2 TB/s streaming rate of DESIGN.md 5.4: 48 B per pixel for the fold, 16 K + 16 B for the resolve.
# The KERNELS alone are read from a kernel trace of a short run (`python robust_timing.py 20 C2 kernels` under the profiler).
# usage: python tools/diagnostics/robust_timing.py [calls] [config] [kernels]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
kernels_only = len(sys.argv) > 3 and sys.argv[3] == "kernels"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(n + 20)]
BUCKETS = (4, 8, 16)
model = {"robust_accumulate": 48.0 * W * H / 5.2e12 * 1e3}
model.update({f"robust_resolve K = {K}": (16.0 * K + 16.0) * W * H / 5.2e12 * 1e3 for K in BUCKETS})

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


if kernels_only:
    for K in BUCKETS:
        ctx.robust_begin(buckets=K)
        for k in range(n):
            frame(k)
            ctx.robust_accumulate()
        for _ in range(n):
            ctx.robust_resolve()
            ctx.robust_resolve(dest=rt.host.ROBUST_DEST_IMAGE)
        ctx.synchronize()
    ctx.close()
    print(json.dumps({"config": name, "calls": n, "pixels": W * H, "traffic_model_ms": {k: round(v, 5) for k, v in model.items()}}), flush=True)
    sys.exit(0)

res = {"frame": window(frame)}
for K in BUCKETS:
    ctx.robust_begin(buckets=K)
    frame(0)
    res[f"robust_accumulate K = {K}"] = window(lambda k: ctx.robust_accumulate())
    res[f"robust_resolve K = {K} buffer"] = window(lambda k: ctx.robust_resolve())
    res[f"robust_resolve K = {K} image"] = window(lambda k: ctx.robust_resolve(dest=rt.host.ROBUST_DEST_IMAGE))
mbytes = ctx.get_option("device_mbytes")
ctx.robust_end()
held = mbytes - ctx.get_option("device_mbytes")
ctx.close()

best = {k: min(v) for k, v in res.items()}
ratio = {k: round(v / model["robust_accumulate" if "accumulate" in k else k.rsplit(" ", 1)[0]], 3) for k, v in best.items() if k != "frame"}
print(json.dumps({"config": name, "calls_per_window": n, "ms_per_call_rounds": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_call": {k: round(v, 4) for k, v in best.items()}, "traffic_model_ms": {k: round(v, 5) for k, v in model.items()},
                  "measured_over_model": ratio, "session_mbytes_K16": held}), flush=True)
