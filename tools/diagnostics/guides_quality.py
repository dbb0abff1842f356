# What guide passes buy the denoisers on the firefly scenes of DESIGN.md 5.12 (the table of DESIGN.md 5.17), on the device, by the protocol
# of robust_adaptive_quality.py: 256 x 256, GlibcRand(0), truth = the plain accumulation of `truth` other frames.  Per scene the RMSE
# against the truth, linear and tone-mapped x / (1 + x), of
#   * render_adaptive alone (masked frames write no planes, so nothing could filter this picture before the guide pass);
#   * the same picture behind 1 and behind 8 guide passes and rtgl_denoise_guided (defaults);
#   * rtgl_robust_denoise (defaults) of a robust session of `frames` frames with the guides the session leaves (its last frame's hit),
#     and with 8 entries in the planes (that frame and 7 guide passes).
# It renders 3 x truth frames and has no time limit of its own: run it under `timeout`.
# usage: timeout 600 python tools/diagnostics/guides_quality.py [size] [threshold] [max_samples] [frames] [buckets] [truth]
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
threshold = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
N = int(sys.argv[4]) if len(sys.argv) > 4 else 64
K = int(sys.argv[5]) if len(sys.argv) > 5 else 8
T = int(sys.argv[6]) if len(sys.argv) > 6 else 4096
GUIDES = rt.host.AOV_ALBEDO | rt.host.AOV_NORMAL | rt.host.AOV_POSITION
SCENES = [("scene_c1(True)", lambda: sc.scene_c1(True), sc.params_c1), ("scene_mesh(10, 5, env_size=16)", lambda: sc.scene_mesh(10, 5, env_size=16), sc.params_c2),
          ("scene_c1(False)", lambda: sc.scene_c1(False), sc.params_c1)]


def errors(img, truth):
    a, b = img[..., :3].astype(np.float64), truth[..., :3].astype(np.float64)
    tm = lambda x: np.maximum(x, 0) / (1 + np.maximum(x, 0))
    return [round(float(np.sqrt(np.mean((a - b) ** 2))), 5), round(float(np.sqrt(np.mean((tm(a) - tm(b)) ** 2))), 5)]


def renderer(scene, params, seed_skip, aov=0):
    r = rt.host.HeadlessRenderer(size, size, aov=aov)
    r.set_scene(scene)
    r.params = params
    for _ in range(seed_skip):                            # the session's frames use words the truth did not
        r._rand.rand()
    return r


out = {"size": size, "threshold": threshold, "max_samples": cap, "robust_frames": N, "buckets": K, "truth_frames": T,
       "columns": ["linear RMSE", "tone-mapped RMSE"], "scenes": {}}
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
    frames, s = r.render_adaptive(threshold, cap, min_samples=2 * K, check_every=16)
    row["render_adaptive"] = errors(r.ctx.read_image(), truth)
    row["render_adaptive frames, samples_total"] = [frames, s["samples_total"]]
    r.set_aov(GUIDES)
    r.render_guides(1)
    r.denoise_guided()
    row["render_adaptive + 1 guide pass + denoise_guided"] = errors(r.read_denoised(), truth)
    r.render_guides(7)
    r.denoise_guided()
    row["render_adaptive + 8 guide passes + denoise_guided"] = errors(r.read_denoised(), truth)
    r.ctx.close()
    r = renderer(scene(), base, T, aov=GUIDES)
    picture = r.render_robust(N, buckets=K)
    row["render_robust"] = errors(picture, truth)
    r.robust_denoise()
    row["robust_denoise, last frame's guides"] = errors(r.read_denoised(), truth)
    r.render_guides(7)
    r.robust_denoise()
    row["robust_denoise, 8 averaged guides"] = errors(r.read_denoised(), truth)
    r.ctx.close()
    out["scenes"][name] = row
print(json.dumps(out), flush=True)
