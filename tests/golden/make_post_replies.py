"""Records what the six older post-process calls answer (rtgl_denoise, rtgl_denoise_guided, rtgl_temporal_accumulate, rtgl_temporal_clip,
rtgl_tonemap, rtgl_error_estimate), as tests/golden/post_replies.json:

    python tests/golden/make_post_replies.py CHECKOUT [OUT.json]

imports the package from CHECKOUT (whose library must be built) and needs a GPU.  The committed record was taken from the commit before
the host rules of these calls moved into raytracer.glsl_amd/csrc/rt_{denoise,temporal,tonemap,error}_plan.hpp; tests/test_post_plans.py
replays it against those headers on the CPU and tests/test_gpu_post_replies.py against the built library, through record() below.

Every context is 32 x 32 on device 0 and sees the small scene and the frames of tests/test_gpu_tonemap.py.  A state is a context after a
few calls, together with what the host then knows of it as plain values (`values`: what the check programs of tests/cpp are given).  In
every state the calls are probed in the order of CALLS, each with every record of its `probes`, in order: a call that succeeds changes
only what a later call of CALLS does not ask about, except rtgl_error_estimate, whose successful calls take the snapshot (so its replies
are a sequence, and a success is recorded with the summary's valid, frames_now and frames_snapshot).

  calls    the six entry points, in the order they are probed
  probes   {call: [[label, the record's 32-bit words, or null for a NULL pointer], ...]}
  states   {state: {"values": {...}, "replies": {call: [[rc, message, or what a success left], one per probe]}}}
A message is its index into `messages`."""
import ctypes as C
import json
import os
import re
import struct
import sys
import types

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (entry point, its defaults call, the binding's record)
CALLS = [("rtgl_error_estimate", "rtgl_error_defaults", "CErrorParams"), ("rtgl_tonemap", "rtgl_tonemap_defaults", "CTonemapParams"),
         ("rtgl_temporal_clip", "rtgl_temporal_clip_defaults", "CTemporalClipParams"), ("rtgl_denoise", "rtgl_denoise_defaults", "CDenoiseParams"),
         ("rtgl_denoise_guided", "rtgl_denoise_guided_defaults", "CDenoiseGuidedParams"),
         ("rtgl_temporal_accumulate", "rtgl_temporal_defaults", "CTemporalParams")]
# the *_abi.py modules whose invalid_blocks() list a call's refused records (the other four calls have no such list: theirs are below)
ABI_LISTS = {"rtgl_tonemap": "test_tonemap_abi", "rtgl_error_estimate": "test_error_abi"}
NAN, INF = float("nan"), float("inf")
UP, DOWN = struct.unpack("<f", struct.pack("<I", 0x3F800001))[0], struct.unpack("<f", struct.pack("<I", 0x3F7FFFFF))[0]      # about 1.0
EDGE_FLOATS = [0.0, -0.0, 1e-45, -1e-45, 1.0, UP, DOWN, -1.0, INF, -INF, NAN]
EDGE_WORDS = [0, 1, 2, 3, 0x80000000, 0xFFFFFFFF]
VALID = {"rtgl_denoise": dict(passes=2, sigma_color=4.0, sigma_normal=0.0, sigma_position=0.0, flags=0),
         "rtgl_denoise_guided": dict(passes=3, sigma_lum=2.0, sigma_normal=0.0, sigma_position=0.0, firefly_ratio=0.0, flags=0),
         "rtgl_temporal_accumulate": dict(max_history=8.0, sigma_normal=0.0, sigma_position=0.1),
         "rtgl_temporal_clip": dict(sigma_scale=1.5, clip_history=2.0, sigma_normal=0.0, sigma_position=0.0),
         "rtgl_tonemap": dict(op=2, flags=0, exposure=0.5),
         "rtgl_error_estimate": dict(threshold=0.1, floor=0.001, quantile_permille=500, flags=1)}
# beyond the generic edges: the values on both sides of each bound, and the records that pass validation and meet a state
EXTRA = {"rtgl_denoise": [dict(passes=8), dict(passes=9), dict(flags=0), dict(flags=0, sigma_normal=0.0), dict(flags=0, sigma_normal=0.0, sigma_position=0.0)],
         "rtgl_denoise_guided": [dict(passes=8), dict(passes=9), dict(flags=0), dict(flags=0, sigma_normal=0.0), dict(flags=0, sigma_normal=0.0, sigma_position=0.0), dict(passes=0)],
         "rtgl_temporal_accumulate": [dict(sigma_normal=0.0), dict(max_history=1.0), dict(max_history=DOWN)],
         "rtgl_temporal_clip": [dict(sigma_normal=0.0), dict(clip_history=1.0), dict(clip_history=DOWN), dict(sigma_scale=1e-45)],
         "rtgl_tonemap": [dict(source=1), dict(source=2), dict(source=2, flags=0), dict(adapt=1.0), dict(adapt=UP), dict(exposure_min=2.0, exposure_max=2.0),
                          dict(low_permille=999, high_permille=0), dict(low_permille=0, high_permille=999), dict(low_permille=500, high_permille=499),
                          dict(low_permille=0xFFFFFFFF, high_permille=0xFFFFFFFF)],
         "rtgl_error_estimate": [dict(quantile_permille=0), dict(quantile_permille=1), dict(quantile_permille=1000), dict(quantile_permille=1001), dict(first_frames=0),
                                 dict(first_frames=2), dict(first_frames=3), dict(first_frames=5), dict(first_frames=6), dict(first_frames=2 ** 31 - 1),
                                 dict(first_frames=-2 ** 31), dict(flags=1), dict(), dict(flags=1), dict(first_frames=2), dict(first_frames=2, flags=1)]}
# literals of the six bodies that no call on a device can be made to return, by text, each with its reason
UNREACHABLE = {"rtgl_error_estimate: the footprint does not fit 32-bit counts": "a picture of 2^32 footprint pixels does not fit a device"}
UNREACHABLE.update({name + ": this context holds no pixels": "only a strip without rows holds none, and a tiled context is refused before this rule"
                    for name in ("rtgl_denoise", "rtgl_denoise_guided", "rtgl_temporal_accumulate", "rtgl_temporal_clip", "rtgl_tonemap")})


def words_of(block):
    return list(struct.unpack("<%dI" % (C.sizeof(block) // 4), bytes(block)))


def label_of(kw):
    return " ".join("%s=%r" % (k, tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items()) or "defaults"


def probes(host):
    """{call: [[label, words or None]]}: NULL, the defaults, one valid record that differs, the listed invalid records, every field's edges"""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    lib, out = host.load_library(), {}
    for call, defaults, ctype in CALLS:
        def block(**kw):
            p = getattr(host, ctype)()
            assert getattr(lib, defaults)(C.byref(p)) == 0
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        rows = [["NULL", None], ["defaults", words_of(block())], [label_of(VALID[call]), words_of(block(**VALID[call]))]]
        if call in ABI_LISTS:
            listed = __import__(ABI_LISTS[call]).invalid_blocks(types.SimpleNamespace(host=host))
            rows += [["listed %d" % k, words_of(p)] for k, p in enumerate(listed)]
        for name, kind in getattr(host, ctype)._fields_:
            if kind is C.c_float:
                rows += [[label_of({name: v}), words_of(block(**{name: v}))] for v in EDGE_FLOATS]
            elif kind is C.c_uint32:
                rows += [[label_of({name: v}), words_of(block(**{name: v}))] for v in EDGE_WORDS]
            elif kind is C.c_int32:
                rows += [[label_of({name: v}), words_of(block(**{name: v}))] for v in (-1, 0, 1)]
            else:                                                       # reserved[]
                n = C.sizeof(kind) // 4
                rows += [[label_of({name: r}), words_of(block(**{name: kind(*r)}))] for r in ([int(j == k) for j in range(n)] for k in range(n))]
        rows += [[label_of(kw), words_of(block(**kw))] for kw in EXTRA[call]]
        out[call] = rows
    return out


class Tracked:
    """A 32 x 32 context and, kept in step with every call made through this class, what the host knows of it as plain values"""
    def __init__(self, host, **tiling):
        import golden_cases
        self.host, self.ctx = host, host.Context(32, 32, device=0, **tiling)
        sc = __import__("raytracer_glsl_amd").scenes
        self.scene, self.sequence, self.next = sc.scene_mesh(10, 5, env_size=16), golden_cases.frame_sequence(sc, sc.params_c2(), 8), 0
        self.v = dict(tiled=bool(tiling), width=32, height=32, px=self.ctx.local_rows * 32, aov=0, aov_restart=True, aov_n=0, denoise_source=0,
                      denoise_variance=0, temporal_moments=0, tm_moments=0, has_temporal=False, has_denoised=False, rendered=False, fn=0, fm=0, first=0,
                      snap=False)

    def option(self, key, value):
        self.ctx.set_option(key, value)
        self.v[key] = value
        if key == "aov":
            self.v["aov_restart"] = True
        return self

    def frames(self, n=2, skip=0):
        if not self.v["rendered"]:
            self.ctx.upload_scene(self.scene)
        self.next += skip
        for p in self.sequence[self.next:self.next + n]:
            self.ctx.render(p)
            self.v.update(rendered=True, fn=p.frames)
            if self.v["aov"]:
                self.v.update(aov_n=1 if self.v["aov_restart"] else self.v["aov_n"] + 1, aov_restart=False)
        self.next += n
        return self

    def accumulate(self):
        self.ctx.temporal_accumulate()
        self.v.update(has_temporal=True, tm_moments=self.v["temporal_moments"])
        return self

    def denoise(self):
        self.ctx.denoise()
        self.v["has_denoised"] = True
        return self

    def estimate(self, **kw):
        self.ctx.error_estimate(**kw)
        if not (kw.get("keep_snapshot") and self.v["snap"] and self.v["fn"] > self.v["fm"]):
            self.v.update(snap=True, fm=self.v["fn"], first=kw.get("first_frames", 1))
        return self

    def drop(self, how):
        getattr(self.ctx, how)()
        self.v["snap"] = False
        return self


def states(host):
    """(name, Tracked) one at a time: the caller closes the context"""
    ALL = host.AOV_ALL
    def new(**tiling):
        return Tracked(host, **tiling)
    def planes():
        return new().option("aov", ALL)
    yield "fresh", new()
    yield "frames, aov 0", new().frames()
    yield "frames, aov all", planes().frames()
    yield "aov enabled after the frames", new().frames().option("aov", ALL)
    for m in (0, 1, 2):
        yield "temporal_accumulate, temporal_moments %d" % m, planes().option("temporal_moments", m).frames().accumulate()
    yield "a history, then aov 0", planes().frames().accumulate().option("aov", 0)
    yield "a history, then the planes restarted", planes().frames().accumulate().option("aov", ALL)
    yield "denoise_source 1, no history", planes().frames().option("denoise_source", 1)
    yield "denoise_source 1, a history", planes().frames().accumulate().option("denoise_source", 1)
    yield "denoise_variance 1, denoise_source 0", planes().option("temporal_moments", 2).frames().accumulate().option("denoise_variance", 1)
    yield "denoise_variance 1, no moments", planes().frames().accumulate().option("denoise_source", 1).option("denoise_variance", 1)
    for m in (1, 2):
        yield ("denoise_variance 1, temporal_moments %d" % m,
               planes().option("temporal_moments", m).frames().accumulate().option("denoise_source", 1).option("denoise_variance", 1))
    yield "after rtgl_denoise", planes().frames().denoise()
    yield "tiled", new(rank=0, world=2, strip_rows=8)
    yield "frames 4 and 5", new().frames(skip=3)
    yield "snapshot kept", new().frames().estimate().frames(1).estimate(keep_snapshot=True)
    yield "snapshot, then a frame", new().frames().estimate().frames(1)
    yield "snapshot dropped by rtgl_error_reset", new().frames().estimate().frames(1).drop("error_reset")
    yield "snapshot dropped by rtgl_clear_image", new().frames().estimate().frames(1).drop("clear_image")


def entry_literals(source, call):
    """every string literal that the body of an entry point passes to fail(), adjacent literals joined"""
    body = re.search(r'extern "C" int %s\(.*?\n}\n' % call, source, re.S).group(0)
    found = re.findall(r'fail\(ctx, \w+, ((?:"(?:[^"\\]|\\.)*"\s*)+)\)', body)
    return ["".join(json.loads('"%s"' % part) for part in re.findall(r'"((?:[^"\\]|\\.)*)"', text)) for text in found]


def record(host, source=None):
    """The whole record, taken from the library that `host` (the package's host module) loads.  `source`: the text of that library's
    rtgl_amd.hip, to check that the record holds every literal of the six bodies"""
    messages, out = [], {"calls": [c for c, _, _ in CALLS], "probes": probes(host), "states": {}}
    lib = host.load_library()

    def message(ctx):
        text = lib.rtgl_last_error(ctx.h).decode()
        if text not in messages:
            messages.append(text)
        return messages.index(text)

    for name, t in states(host):
        replies = {}
        for call, _, ctype in CALLS:
            rows = []
            for _, words in out["probes"][call]:
                block = None if words is None else getattr(host, ctype).from_buffer_copy(struct.pack("<%dI" % len(words), *words))
                rc = getattr(lib, call)(t.ctx.h, None if block is None else C.byref(block))
                left = None
                if rc == 0 and call == "rtgl_error_estimate":
                    s = t.ctx.read_error_summary()
                    left = [int(s["valid"]), int(s["frames_now"]), int(s["frames_snapshot"])]
                rows.append([rc, message(t.ctx) if rc else left])
            replies[call] = rows
        out["states"][name] = {"values": t.v, "replies": replies}
        t.ctx.close()
    out["messages"] = messages
    if source is not None:
        literals = [text for call, _, _ in CALLS for text in entry_literals(source, call)]
        missing = [text for text in literals if text not in messages and text not in UNREACHABLE]
        assert not missing, missing
        assert not [text for text in UNREACHABLE if text in messages or text not in literals]
    return out


def with_texts(rec):
    """The record with every message's index replaced by the message (what the tests compare)."""
    out = {k: rec[k] for k in ("calls", "probes")}
    out["states"] = {name: {"values": s["values"], "replies": {call: [[rc, rec["messages"][x] if rc else x] for rc, x in rows] for call, rows in s["replies"].items()}}
                     for name, s in rec["states"].items()}
    return out


def dump(rec, path):
    """One line per probe list, per state's values and per call of a state: a diff of two records shows the call that changed."""
    def one(v):
        return json.dumps(v, separators=(",", ":"))
    lines = ['"calls": ' + one(rec["calls"]), '"probes": {\n%s\n}' % ",\n".join(" %s: %s" % (one(k), one(v)) for k, v in rec["probes"].items())]
    states_ = []
    for name, s in rec["states"].items():
        calls = ",\n".join("   %s: %s" % (one(k), one(v)) for k, v in s["replies"].items())
        states_.append(' %s: {\n  "values": %s,\n  "replies": {\n%s\n  }\n }' % (one(name), one(s["values"]), calls))
    lines.append('"states": {\n%s\n}' % ",\n".join(states_))
    lines.append('"messages": [\n%s\n]' % ",\n".join(" " + one(x) for x in rec["messages"]))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    checkout = os.path.abspath(sys.argv[1])
    sys.path[:0] = [checkout, TESTS]
    import raytracer_glsl_amd
    with open(os.path.join(checkout, "raytracer.glsl_amd", "csrc", "rtgl_amd.hip")) as f:
        text = f.read()
    dump(record(raytracer_glsl_amd.host, text), sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "post_replies.json"))
