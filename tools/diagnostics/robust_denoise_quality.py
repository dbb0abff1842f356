# What rtgl_robust_denoise buys on the firefly scenes of DESIGN.md 5.12 (the table of DESIGN.md 5.15), on the device.
# Per scene: a robust session of `frames` one-sample frames (K buckets, planes on), then against the plain accumulation of `truth` other
# frames the RMSE, linear and tone-mapped x / (1 + x), of
#   * the plain mean of the session's frames (what the image would hold without a session);
#   * rtgl_robust_resolve alone;
#   * the resolve into the image followed by rtgl_denoise_guided, at its defaults and with the clamp off;
#   * rtgl_robust_denoise at its defaults.
# It renders 3 x (truth + 2 frames) frames and has no time limit of its own: run it under `timeout` (the defaults take seconds on an MI355X).
# usage: timeout 300 python tools/diagnostics/robust_denoise_quality.py [size] [frames] [buckets] [truth]
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 32
K = int(sys.argv[3]) if len(sys.argv) > 3 else 8
T = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
SCENES = [("scene_c1(True)", lambda: sc.scene_c1(True), sc.params_c1), ("scene_mesh(10, 5, env_size=16)", lambda: sc.scene_mesh(10, 5, env_size=16), sc.params_c2),
          ("scene_c1(False)", lambda: sc.scene_c1(False), sc.params_c1)]
AOV = rt.host.AOV_ALBEDO | rt.host.AOV_NORMAL | rt.host.AOV_POSITION
g = sc.GlibcRand(0); randoms = [g.rand() for _ in range(N + T)]


def errors(img, truth):
    a, b = img[..., :3].astype(np.float64), truth[..., :3].astype(np.float64)
    tm = lambda x: np.maximum(x, 0) / (1 + np.maximum(x, 0))
    return [round(float(np.sqrt(np.mean((a - b) ** 2))), 5), round(float(np.sqrt(np.mean((tm(a) - tm(b)) ** 2))), 5)]


out = {"size": size, "frames": N, "buckets": K, "truth_frames": T, "columns": ["linear RMSE", "tone-mapped RMSE"], "scenes": {}}
for name, scene, params in SCENES:
    base = params()
    ctx = rt.host.Context(size, size)
    ctx.upload_scene(scene())
    for k in range(T):
        ctx.render(base.replace(frames=k, reset_flag=1 if k == 0 else 0, random=randoms[N + k]), sync=False)
    truth = ctx.read_image()
    for k in range(N):
        ctx.render(base.replace(frames=k, reset_flag=1 if k == 0 else 0, random=randoms[k]), sync=False)
    row = {"mean": errors(ctx.read_image(), truth)}
    ctx.set_aov(AOV)
    ctx.robust_begin(buckets=K)
    for k in range(N):
        ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        ctx.robust_accumulate()
    ctx.robust_denoise()
    row["robust_denoise"] = errors(ctx.read_denoised(), truth)
    kept = ctx.read_denoise_variance()[..., 3]
    ctx.robust_resolve(dest=rt.host.ROBUST_DEST_IMAGE)
    row["resolve"] = errors(ctx.read_image(), truth)
    ctx.denoise_guided()
    row["resolve + denoise_guided"] = errors(ctx.read_denoised(), truth)
    ctx.denoise_guided(firefly_ratio=0.0)
    row["resolve + denoise_guided, clamp off"] = errors(ctx.read_denoised(), truth)
    row["pixels trimmed"] = round(float((kept < K).mean()), 4)
    ctx.close()
    out["scenes"][name] = row
print(json.dumps(out), flush=True)
