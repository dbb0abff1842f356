# GPU time per frame with the first-hit planes off and on (option "aov" = 0 / 15), from the HIP events of rtgl_accumulated_timing over
# ~200 back-to-back frames per run; the two settings alternate, twice each, on one context per run.
# usage: python tools/diagnostics/aov_timing.py [frames] [config]
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); ps = [base.replace(frames=f, random=g.rand()) for f in range(1, n + 21)]


def run(mask):
    ctx = rt.host.Context(W, H)
    ctx.set_aov(mask)
    ctx.upload_scene(scene)
    for p in ps[:20]:
        ctx.render(p, sync=False)                         # warm-up: buffers, grid estimates
    ctx.synchronize()
    ctx.set_option("kernel_timing", 1)
    ctx.timing_reset()
    for p in ps[20:]:
        ctx.render(p, sync=False)
    t = ctx.accumulated_timing()
    ctx.close()
    return t["frame_ms"] / max(t["frames"], 1)


res = {0: [], 15: []}
for _ in range(2):
    for mask in (0, 15):
        res[mask].append(run(mask))
off, on = min(res[0]), min(res[15])
print(json.dumps({"config": name, "frames": n, "ms_per_frame_aov0": res[0], "ms_per_frame_aov15": res[15],
                  "best_aov0": round(off, 4), "best_aov15": round(on, 4), "cost_ms": round(on - off, 4), "cost_pct": round(100 * (on - off) / off, 2)}), flush=True)
