# GPU time of a robust adaptive session (rtgl_robust_adaptive_*) next to the calls it is made from, measured in ONE run.
# One context, warm-up calls, then for every case `frames` calls enqueued back to back between two synchronisations, host clock around
# them (the calls only enqueue, so the window is device time once the queue is full), three rounds, best of three:
#   * the ordinary frame as it runs by default;
#   * rtgl_adaptive_frame and rtgl_robust_adaptive_frame (K = 8) with 1, 1/2, 1/4 and 1/16 of the tiles active, scattered: the fold against
#     the merge under the same mask, by the difference of the two frames;
#   * per K = 4, 8, 16: rtgl_robust_adaptive_frame with every tile active; rtgl_robust_adaptive_update with every tile changed and with 1/16
#     of the tiles changed (each behind one frame under that mask, the frame's time taken off: the update synchronises and reads the records,
#     so this is the cost a caller sees, not the kernel's); rtgl_robust_adaptive_resolve next to rtgl_robust_resolve of a plain session of
#     the same K on the same context.
# usage: python tools/diagnostics/robust_adaptive_timing.py [frames] [config]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(n + 20)]
ty, tx = (H + 15) // 16, (W + 15) // 16
rows, cols = np.mgrid[0:ty, 0:tx]
BIG = 1 << 20

ctx = rt.host.Context(W, H)
ctx.upload_scene(scene)


def window(call, rounds=3):
    for k in range(20):
        call(k)                                           # warm-up: buffers, grid estimates, code objects
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for k in range(n):
            call(20 + k)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def ordinary(k):
    ctx.render(base.replace(frames=k + 1, random=randoms[k]), sync=False)


def adaptive(k):
    ctx.adaptive_frame(base.replace(random=randoms[k]), sync=False)


def robust_adaptive(k):
    ctx.robust_adaptive_frame(base.replace(random=randoms[k]), sync=False)


masks = {"1/1": np.ones((ty, tx), np.uint8), "1/2": ((rows + cols) % 2 == 0).astype(np.uint8)}
for d, step in ((4, (2, 2)), (16, (4, 4))):
    masks[f"1/{d}"] = ((rows % step[0] == 0) & (cols % step[1] == 0)).astype(np.uint8)

res = {"ordinary": window(ordinary)}
ctx.adaptive_begin(min_samples=1, max_samples=BIG)
for label, mask in masks.items():
    ctx.adaptive_set_mask(mask)
    res[f"adaptive_frame {label}"] = window(adaptive)
ctx.robust_adaptive_begin(buckets=8, min_samples=8, max_samples=BIG)
for label, mask in masks.items():
    ctx.robust_adaptive_set_mask(mask)
    res[f"robust_adaptive_frame K=8 {label}"] = window(robust_adaptive)

for K in (4, 8, 16):
    ctx.robust_adaptive_begin(buckets=K, min_samples=K, max_samples=BIG)
    res[f"robust_adaptive_frame K={K} 1/1"] = res.get(f"robust_adaptive_frame K={K} 1/1") or window(robust_adaptive)
    for label in ("1/1", "1/16"):
        current = masks[label]

        def frame_only(k):
            ctx.robust_adaptive_set_mask(current)
            robust_adaptive(k)
            ctx.synchronize()

        def frame_and_update(k):
            frame_only(k)
            ctx.robust_adaptive_update()

        res[f"frame, synchronised K={K} {label}"] = window(frame_only)
        res[f"frame + update K={K} {label} changed"] = window(frame_and_update)
    ctx.robust_adaptive_set_mask(masks["1/1"])
    res[f"robust_adaptive_resolve K={K}"] = window(lambda k: ctx.robust_adaptive_resolve())
    ctx.robust_begin(buckets=K)
    for k in range(K):
        ctx.robust_accumulate()
    res[f"robust_resolve K={K}"] = window(lambda k: ctx.robust_resolve())
    ctx.robust_end()
ctx.close()

best = {k: min(v) for k, v in res.items()}
derived = {f"fold minus merge {label}": round(best[f"robust_adaptive_frame K=8 {label}"] - best[f"adaptive_frame {label}"], 4) for label in masks}
for K in (4, 8, 16):
    for label in ("1/1", "1/16"):
        derived[f"update K={K} {label} changed"] = round(best[f"frame + update K={K} {label} changed"] - best[f"frame, synchronised K={K} {label}"], 4)
px = (W // 8 * 8) * (H // 8 * 8)
print(json.dumps({"config": name, "calls_per_window": n, "ms_per_call_rounds": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_call": {k: round(v, 4) for k, v in best.items()}, "ms_by_difference": derived,
                  "active_share_of_tiles": {k: round(float(m.mean()), 4) for k, m in masks.items()},
                  "traffic_model_ms_at_5.2_TB_per_s": {"fold 1/1 (48 B per active pixel)": round(48.0 * px / 5.2e12 * 1e3, 5),
                                                      **{f"resolve K={K} (16 K + 16 B per pixel)": round((16.0 * K + 16) * W * H / 5.2e12 * 1e3, 5) for K in (4, 8, 16)}}}), flush=True)
