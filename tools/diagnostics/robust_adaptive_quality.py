# What a robust adaptive session buys on the firefly scenes of DESIGN.md 5.12 (the table of DESIGN.md 5.16), on the device, by the protocol
# of robust_denoise_quality.py: 256 x 256, GlibcRand(0), truth = the plain accumulation of `truth` other frames.
# Per scene, at ONE threshold: the samples spent (samples_total, the sum of the per-tile counts over the footprint's pixels; frames x pixels
# for the session that traces the whole picture every frame) and the RMSE against the truth, linear and tone-mapped x / (1 + x), of
#   * render_robust_adaptive: masked frames into bucket means, each tile stopped by the spread of its own buckets;
#   * render_robust_until: the plain robust session, stopped when 95 % of the tiles are clean;
#   * render_adaptive: masked frames into a plain running mean, each tile stopped on two moments of that mean.
# It renders 3 x truth frames and has no time limit of its own: run it under `timeout` (the defaults take seconds on an MI355X).
# usage: timeout 600 python tools/diagnostics/robust_adaptive_quality.py [size] [threshold] [max_samples] [buckets] [truth]
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
threshold = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
K = int(sys.argv[4]) if len(sys.argv) > 4 else 8
T = int(sys.argv[5]) if len(sys.argv) > 5 else 4096
SCENES = [("scene_c1(True)", lambda: sc.scene_c1(True), sc.params_c1), ("scene_mesh(10, 5, env_size=16)", lambda: sc.scene_mesh(10, 5, env_size=16), sc.params_c2),
          ("scene_c1(False)", lambda: sc.scene_c1(False), sc.params_c1)]


def errors(img, truth):
    a, b = img[..., :3].astype(np.float64), truth[..., :3].astype(np.float64)
    tm = lambda x: np.maximum(x, 0) / (1 + np.maximum(x, 0))
    return [round(float(np.sqrt(np.mean((a - b) ** 2))), 5), round(float(np.sqrt(np.mean((tm(a) - tm(b)) ** 2))), 5)]


def renderer(scene, params, seed_skip):
    r = rt.host.HeadlessRenderer(size, size)
    r.set_scene(scene)
    r.params = params
    for _ in range(seed_skip):                            # the session's frames use words the truth did not
        r._rand.rand()
    return r


out = {"size": size, "threshold": threshold, "max_samples": cap, "buckets": K, "truth_frames": T, "check_every": 16,
       "columns": ["samples_total", "frames", "linear RMSE", "tone-mapped RMSE"], "scenes": {}}
for name, scene, params in SCENES:
    base = params()
    g = sc.GlibcRand(0)
    ctx = rt.host.Context(size, size)
    ctx.upload_scene(scene())
    for k in range(T):
        ctx.render(base.replace(frames=k, reset_flag=1 if k == 0 else 0, random=g.rand()), sync=False)
    truth = ctx.read_image()
    ctx.close()
    row = {}
    r = renderer(scene(), base, T)
    frames, s, picture = r.render_robust_adaptive(threshold, cap, min_samples=2 * K, check_every=16, buckets=K)
    row["render_robust_adaptive"] = [s["samples_total"], frames] + errors(picture, truth)
    row["render_robust_adaptive tiles"] = dict(converged=s["tiles_converged"], capped=s["tiles_capped"], samples_min=s["samples_min"], samples_max=s["samples_max"])
    r.ctx.close()
    r = renderer(scene(), base, T)
    frames, s, picture = r.render_robust_until(threshold, cap, check_every=16, buckets=K)
    row["render_robust_until"] = [frames * size * size, frames] + errors(picture, truth)
    r.ctx.close()
    r = renderer(scene(), base, T)
    frames, s = r.render_adaptive(threshold, cap, min_samples=2 * K, check_every=16)
    row["render_adaptive"] = [s["samples_total"], frames] + errors(r.ctx.read_image(), truth)
    r.ctx.close()
    out["scenes"][name] = row
print(json.dumps(out), flush=True)
