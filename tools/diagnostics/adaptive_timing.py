# GPU time of a masked frame of adaptive sampling (rtgl_adaptive_frame) next to the ordinary frame.
# One context, warm-up frames, then for every case `frames` frames enqueued back to back between two synchronisations, host clock around
# them (the calls only enqueue, so the window is device time once the queue is full), three rounds, best of three:
#   * the ordinary frame as it runs by default (kept camera bits, lean camera bounce);
#   * the ordinary frame with option "camera_lean" = 0 and RTGL_AMD_NO_CAMERA_KEEP set: the fair baseline, a masked frame forgoes both;
#   * masked frames with 1, 1/2, 1/4 and 1/16 of the tiles active, contiguous (the lowest tile rows) and scattered (every 2nd, 4th, 16th
#     tile in both directions);
#   * masked frames at 1/1 with an rtgl_adaptive_update behind each: the update's share by difference (it synchronises and reads the
#     records, so this is the cost a caller sees, not the kernel's);
#   * the break-even fraction: where a masked frame costs what the default ordinary frame costs, interpolated between the measured fractions.
# The merge and the update KERNELS alone are read from a kernel trace of a short run (`python adaptive_timing.py 20 C2 kernels` under the
# profiler): their byte models are 48 B (16 sample + 16 image read, 16 written) and 24 B (16 image + 4 snapshot read, 4 written) per
# active pixel at the 5.2 TB/s streaming rate of DESIGN.md 5.4.
# usage: python tools/diagnostics/adaptive_timing.py [frames] [config] [kernels]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
kernels_only = len(sys.argv) > 3 and sys.argv[3] == "kernels"
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(n + 20)]
ty, tx = (H + 15) // 16, (W + 15) // 16
rows, cols = np.mgrid[0:ty, 0:tx]

ctx = rt.host.Context(W, H)
ctx.upload_scene(scene)


def window(frame, rounds=3):
    for k in range(20):
        frame(k)                                          # warm-up: buffers, grid estimates, code objects
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for k in range(n):
            frame(20 + k)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def ordinary(k):
    ctx.render(base.replace(frames=k + 1, random=randoms[k]), sync=False)


def masked(k):
    ctx.adaptive_frame(base.replace(random=randoms[k]), sync=False)


def masked_and_update(k):
    masked(k)
    ctx.adaptive_update()
    ctx.adaptive_set_mask(current)                        # (the update switches tiles off; the mask is put back)


if kernels_only:
    ctx.adaptive_begin(min_samples=1, max_samples=1 << 20)
    for k in range(n):
        masked(k)
        ctx.adaptive_update()
        ctx.adaptive_set_mask(np.ones((ty, tx), np.uint8))
    ctx.close()
    print(json.dumps({"config": name, "frames": n, "active_pixels": (W // 8 * 8) * (H // 8 * 8), "traffic_model_ms": {
        "adaptive_merge_kernel": 48.0 * (W // 8 * 8) * (H // 8 * 8) / 5.2e12 * 1e3, "adaptive_tiles_kernel": 24.0 * (W // 8 * 8) * (H // 8 * 8) / 5.2e12 * 1e3}}), flush=True)
    sys.exit(0)

res = {"ordinary": window(ordinary)}
ctx.set_option("camera_lean", 0)
os.environ["RTGL_AMD_NO_CAMERA_KEEP"] = "1"
res["ordinary_no_keep_no_lean"] = window(ordinary)
del os.environ["RTGL_AMD_NO_CAMERA_KEEP"]
ctx.set_option("camera_lean", 1)

masks = {"1/1": np.ones((ty, tx), np.uint8)}
for d, step in ((2, (2, 1)), (4, (2, 2)), (16, (4, 4))):
    masks[f"1/{d} contiguous"] = (rows < -(-ty // d)).astype(np.uint8)
    masks[f"1/{d} scattered"] = ((rows % step[0] == 0) & (cols % step[1] == 0)).astype(np.uint8) if d != 2 else ((rows + cols) % 2 == 0).astype(np.uint8)
ctx.adaptive_begin(min_samples=1, max_samples=1 << 20)
share = {}
for label, mask in masks.items():
    current = mask
    ctx.adaptive_set_mask(mask)
    share[label] = float(mask.mean())
    res["masked " + label] = window(masked)
current = masks["1/1"]
ctx.adaptive_set_mask(current)
res["masked 1/1 + update"] = window(masked_and_update)
ctx.close()

best = {k: min(v) for k, v in res.items()}
# where the contiguous series crosses the default ordinary frame
xs = sorted((share[k], best["masked " + k]) for k in share if "scattered" not in k)
even = None
for (f0, m0), (f1, m1) in zip(xs, xs[1:]):
    if m0 <= best["ordinary"] <= m1 and m1 > m0:
        even = f0 + (f1 - f0) * (best["ordinary"] - m0) / (m1 - m0)
print(json.dumps({"config": name, "frames_per_window": n, "ms_per_frame_rounds": {k: [round(x, 4) for x in v] for k, v in res.items()},
                  "ms_per_frame": {k: round(v, 4) for k, v in best.items()}, "active_share_of_tiles": {k: round(v, 4) for k, v in share.items()},
                  "update_ms_by_difference": round(best["masked 1/1 + update"] - best["masked 1/1"], 4),
                  "break_even_share_against_the_default_frame": None if even is None else round(even, 3)}), flush=True)
