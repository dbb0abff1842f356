"""Records what rtgl_set_option, rtgl_get_option and the environment's spellings of the options answer, as tests/golden/option_replies.json:

    python tests/golden/make_option_replies.py CHECKOUT [OUT.json]

imports the package from CHECKOUT (whose library must be built) and needs a GPU.  The committed record was taken from the commit before
the options moved into raytracer.glsl_amd/csrc/rt_options.hpp; tests/test_options.py replays it against that header on the CPU and
tests/test_gpu_options.py against the built library, through record() below.

Every context is 8 x 8 on device 0 and never sees a scene or a frame: each probe is an argument check or a store.

  fresh       {key: [rc, value or message]} of rtgl_get_option on a fresh context, for every readable key
  set         {key: [[rc of rtgl_set_option, message or null, rc of rtgl_get_option(key) afterwards, its value or message], one per probe]}:
              one fresh context per settable key, the values of `probes` in ascending order
  unknown, null_key   {"set": [rc, message], "get": [rc, message]};  null_value: [rc, message] of rtgl_get_option(ctx, "kernel", NULL)
  env         {NAME: {"option": key, "replies": {text: [rc, value or message]}}}: NAME=text while a context is created, then rtgl_get_option(key)
A message is its index into `messages`."""
import ctypes as C
import json
import os
import sys

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
PROBES = sorted(set(range(-2, 71)) | {127, 128, 129, 192, 255, 256, 4032, 4095, 4096, 4097, 4160, 131072, INT_MAX, INT_MIN})
SETTABLE = ["kernel", "wf_rays", "wf_chunk", "debug_skip_exact", "mf_chunk_quads", "scan_waves", "scan_dynamic", "narrow_fused", "camera_lean",
            "shade_pass", "frame_batch", "cull", "sort_min_rays", "mf_group_quads", "wf_packed", "wf_early", "wf_mode", "aov", "denoise_source",
            "temporal_moments", "denoise_variance", "rng_state", "counters", "kernel_timing"]
DERIVED = ["kernel_in_use", "mf_sets", "mf_group_quads", "camera_lean_frames", "shade_pass_launches", "cand_region_pairs", "device_mbytes"]
READABLE = [k for k in SETTABLE if k not in ("debug_skip_exact", "mf_group_quads")] + DERIVED
SPELLINGS = {"RTGL_AMD_KERNEL": "kernel", "RTGL_AMD_SCAN_WAVES": "scan_waves", "RTGL_AMD_FRAME_BATCH": "frame_batch",
             "RTGL_AMD_SCAN_DYNAMIC": "scan_dynamic", "RTGL_AMD_NARROW_FUSED": "narrow_fused", "RTGL_AMD_CAMERA_LEAN": "camera_lean",
             "RTGL_AMD_SHADE_PASS": "shade_pass"}
TEXTS = ["0", "1", "2", "3", "4", "5", "16", "17", "-1", "", "abc", "2x", " 1"]


def record(host):
    """The whole record, taken from the library that `host` (the package's host module) loads."""
    messages = []

    def message(ctx):
        text = ctx.lib.rtgl_last_error(ctx.h).decode()
        if text not in messages:
            messages.append(text)
        return messages.index(text)

    def set_(ctx, key, value):
        rc = ctx.lib.rtgl_set_option(ctx.h, key, value)
        return [rc, message(ctx) if rc else None]

    def get(ctx, key, null_value=False):
        v = C.c_int(-12345)
        rc = ctx.lib.rtgl_get_option(ctx.h, key, None if null_value else C.byref(v))
        return [rc, message(ctx) if rc else int(v.value)]

    def fresh():
        return host.Context(8, 8, device=0)

    out = {"probes": PROBES, "derived": DERIVED}
    ctx = fresh()
    out["fresh"] = {key: get(ctx, key.encode()) for key in READABLE}
    out["unknown"] = {"set": set_(ctx, b"no_such_option", 1), "get": get(ctx, b"no_such_option")}
    out["null_key"] = {"set": set_(ctx, None, 1), "get": get(ctx, None)}
    out["null_value"] = get(ctx, b"kernel", null_value=True)
    ctx.close()
    out["set"] = {}
    for key in SETTABLE:
        ctx = fresh()
        out["set"][key] = [set_(ctx, key.encode(), value) + get(ctx, key.encode()) for value in PROBES]
        ctx.close()
    out["env"] = {}
    for name, key in SPELLINGS.items():
        replies = {}
        for text in TEXTS:
            os.environ[name] = text
            try:
                ctx = fresh()
            finally:
                del os.environ[name]
            replies[text] = get(ctx, key.encode())
            ctx.close()
        out["env"][name] = {"option": key, "replies": replies}
    out["messages"] = messages
    return out


def with_texts(rec):
    """The record with every message's index replaced by the message (what the tests compare)."""
    def pair(rc, x):
        return [rc, rec["messages"][x] if rc else x]
    out = {k: rec[k] for k in ("probes", "derived")}
    out["fresh"] = {k: pair(*v) for k, v in rec["fresh"].items()}
    out["unknown"], out["null_key"] = ({call: pair(*v) for call, v in rec[k].items()} for k in ("unknown", "null_key"))
    out["null_value"] = pair(*rec["null_value"])
    out["set"] = {k: [pair(rc, m) + pair(get_rc, g) for rc, m, get_rc, g in v] for k, v in rec["set"].items()}
    out["env"] = {k: {"option": v["option"], "replies": {t: pair(*r) for t, r in v["replies"].items()}} for k, v in rec["env"].items()}
    return out


def dump(rec, path):
    """One line per key of a section and per message: a diff of two records shows the option that changed."""
    def one(v):
        return json.dumps(v, separators=(",", ":"))
    sections = []
    for name, v in rec.items():
        if isinstance(v, dict):
            sections.append('"%s": {\n%s\n}' % (name, ",\n".join(" %s: %s" % (one(k), one(x)) for k, x in v.items())))
        elif name == "messages":
            sections.append('"messages": [\n%s\n]' % ",\n".join(" " + one(x) for x in v))
        else:
            sections.append('"%s": %s' % (name, one(v)))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(sections) + "\n}\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import raytracer_glsl_amd
    dump(record(raytracer_glsl_amd.host), sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "option_replies.json"))
