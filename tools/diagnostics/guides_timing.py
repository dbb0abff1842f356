# GPU time per guide pass (rtgl_guides_frame, option "aov" = 15) beside the two frames it is measured against, in one run: the ordinary
# frame of the configuration ("aov" = 0), and the frame of max_bounce = 1 with "aov" = 15 -- the cheapest way to the same planes without
# the pass, and code the pass does not touch: the yardstick.  Each arm has a context of its own; per round every arm enqueues `calls`
# calls back to back between two synchronisations (the method of denoise_timing.py), the arms take turns, `rounds` rounds.
# "guides_below_yardstick": EVERY round of the pass is below EVERY round of the one-bounce frame.
# usage: python tools/diagnostics/guides_timing.py [calls] [config] [rounds]
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raytracer_glsl_amd as rt
sc = rt.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
name = sys.argv[2] if len(sys.argv) > 2 else "C2"
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
cfg = sc.CONFIGS[name]; W, H = cfg["width"], cfg["height"]; scene = cfg["scene"](); base = cfg["params"]()
g = sc.GlibcRand(0); words = [g.rand() for _ in range(n + 20)]


def arm(mask, params, call):
    ctx = rt.host.Context(W, H)
    if mask:
        ctx.set_aov(mask)
    ctx.upload_scene(scene)
    ps = [params.replace(frames=k + 1, random=w) for k, w in enumerate(words)]
    fn = getattr(ctx, call)
    for p in ps[:20]:                                      # warm-up: buffers, grid estimates, kept camera bits
        fn(p, sync=False)
    ctx.synchronize()

    def one_round():
        t0 = time.perf_counter()
        for p in ps[20:]:
            fn(p, sync=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    return ctx, one_round


arms = {"guides_pass": arm(15, base, "guides_frame"), "frame": arm(0, base, "render"), "frame_1_bounce_aov15": arm(15, base.replace(max_bounce=1), "render")}
res = {k: [] for k in arms}
for _ in range(rounds):
    for k, (_, one_round) in arms.items():
        res[k].append(round(one_round(), 4))
last_ms = arms["guides_pass"][0].last_frame_ms()           # the events of the last pass alone
for ctx, _ in arms.values():
    ctx.close()
print(json.dumps({"config": name, "calls_per_round": n, "rounds": rounds, "ms_per_call": res, "best": {k: min(v) for k, v in res.items()},
                  "worst": {k: max(v) for k, v in res.items()}, "last_pass_event_ms": round(last_ms, 4),
                  "guides_below_yardstick": max(res["guides_pass"]) < min(res["frame_1_bounce_aov15"])}), flush=True)
