"""The post-process calls AGAINST EACH OTHER on one context: the sequences of tests/post_sequence_inputs.py on the device against
tests/post_sequence_model.py, the host state of a context restated from include/rtgl_amd.h and composed from the numpy mirrors.

Nothing the model is fed comes from the context under test.  A PLAIN TWIN, a second host.Context that only ever traces frames and has its
image written, cleared and its planes set, supplies the image and the planes after every frame; where the model's image has moved on without
a frame (a masked frame's merge, a resolve into the image) the twin is handed the MODEL's image before it traces the next one.  Every run
of ordinary frames of the twin is held to the CPU oracle, and every one-frame sample of a masked frame of either kind likewise (the merge is
adaptive_mirror's, the fold robust_adaptive_mirror's).  Every comparison is of bits, a NaN counting as one word; there is no tolerance
anywhere.  One printed line per differing step.

POST_SEQ_CASES (default 24: eight per size) and POST_SEQ_SEED (default 0) choose the sequences, as FUZZ_CASES and FUZZ_SEED do elsewhere.
Twin, oracle and model run once per seed and are shared by the tests."""
import os
import re
import time

import numpy as np
import pytest

import adaptive_mirror as am
import error_mirror as em
import post_sequence_inputs as ps
import post_sequence_model as pm

pytestmark = pytest.mark.gpu

f32 = np.float32
REFUSED = pm.REFUSED


def seeds():
    return ps.default_seeds(int(os.environ.get("POST_SEQ_CASES", str(ps.DEFAULT_SEQUENCES))), int(os.environ.get("POST_SEQ_SEED", "0")))


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


# ---------------------------------------------------------------------------------------------- comparison of bits

def words(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    if isinstance(a, dict) and isinstance(b, dict) and "valid" in b:                       # an error summary: the fields of the record
        return (all(int(a[k]) == int(b[k]) for k in em.SUMMARY_INT) and all((words(f32(a[k])) == words(f32(b[k]))).all() for k in em.SUMMARY_FLOAT))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == f32 and b.dtype == f32:
        return bool((words(a) == words(b)).all())
    if a.dtype.names or b.dtype.names:
        return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    return bool((a == b).all())


def differing(got, want):
    return [name for name in pm.READOUTS if not same(got[name], want[name])]


# ---------------------------------------------------------------------------------------------- the context under test

def status_of(call):
    """(status, value) of a binding call: host.Context raises with the status in its text"""
    try:
        return 0, call()
    except Exception as e:                                             # RtglError
        m = re.search(r"\((-?\d+)\)", str(e))
        assert m, str(e)
        return int(m.group(1)), None


def read(call):
    status, value = status_of(call)
    assert status in (0, pm.STATE), f"a read-out returned {status}"
    return REFUSED if status else value


def read_all(ctx):
    out = dict(image=ctx.read_image(), planes={bit: read(lambda: ctx.read_aov(bit)) for bit in pm.BITS}, denoised=read(ctx.read_denoised),
               variance=read(ctx.read_denoise_variance), history=read(ctx.read_temporal), moments=read(ctx.read_temporal_moments), display=read(ctx.read_display),
               exposure=read(ctx.read_tonemap_exposure), histogram=read(ctx.read_tonemap_histogram), error_summary=read(ctx.read_error_summary),
               error_tiles=read(ctx.read_error_tiles), adaptive_tiles=read(ctx.read_adaptive_tiles), adaptive_mask=read(ctx.adaptive_get_mask),
               robust_output=read(ctx.read_robust), robust_frames=read(ctx.robust_frames), robust_error_summary=read(ctx.read_robust_error_summary),
               robust_error_tiles=read(ctx.read_robust_error_tiles))
    frames = out["robust_frames"]
    out["robust_buckets"] = REFUSED if frames == REFUSED else np.stack([ctx.read_robust_bucket(j) for j in range(frames[1])])
    out.update(robust_adaptive_output=read(ctx.read_robust_adaptive), robust_adaptive_tiles=read(ctx.read_robust_adaptive_tiles),
               robust_adaptive_mask=read(ctx.robust_adaptive_get_mask), robust_adaptive_buckets=REFUSED)
    planes = []                                                        # no call tells K: the planes there are, up to the first "bucket >= K"
    for j in range(max(ps.BUCKETS) + 1):
        status, plane = status_of(lambda: ctx.read_robust_adaptive_bucket(j))
        allowed = (0, pm.STATE) if j == 0 else (0,) if j < min(ps.BUCKETS) else (0, pm.INVALID)
        assert status in allowed, f"rtgl_read_robust_adaptive_bucket_f32({j}) returned {status}"
        if status:
            break
        planes.append(plane)
    assert len(planes) in (0,) + tuple(ps.BUCKETS), len(planes)
    if planes:
        out["robust_adaptive_buckets"] = np.stack(planes)
    return out


def normalise(want):
    """the model's read-outs as the binding returns them: the records of both kinds of masked-tile session contiguous"""
    out = dict(want)
    for name in ("adaptive_tiles", "robust_adaptive_tiles"):
        if out[name] is not REFUSED:
            out[name] = np.ascontiguousarray(out[name])
    return out


def apply(ctx, seq, step, rows=None, bound=0, sync=None):
    """one step on the context: (status, what an adaptive_update or robust_adaptive_update returned)"""
    k, a = step.kind, step.args
    lib, h = ctx.lib, ctx.h
    if k in pm.FRAMES:
        ctx.set_params(ps.frame_params(seq.base, a))
        rc = {"render": lib.rtgl_render_frame, "adaptive_frame": lib.rtgl_adaptive_frame, "robust_adaptive_frame": lib.rtgl_robust_adaptive_frame}[k](h)
        if rc == 0 and (a["sync"] if sync is None else sync):
            ctx.synchronize()
        return rc, None
    if k in pm.UPDATES:
        return status_of(ctx.adaptive_update if k == "adaptive_update" else ctx.robust_adaptive_update)
    call = {
        "write_image": lambda: ctx.write_image(a["pixels"] if rows is None else a["pixels"][rows]),
        "clear_image": ctx.clear_image, "bind_image": lambda: ctx.bind_device_image(bound),
        "set_aov": lambda: ctx.set_aov(a["mask"]), "set_option": lambda: ctx.set_option(a["key"], a["value"]),
        "denoise": lambda: ctx.denoise(**a), "denoise_guided": lambda: ctx.denoise_guided(**a),
        "temporal_accumulate": lambda: ctx.temporal_accumulate(**a), "temporal_reset": ctx.temporal_reset, "temporal_clip": lambda: ctx.temporal_clip(**a),
        "tonemap": lambda: ctx.tonemap(**a), "tonemap_reset": ctx.tonemap_reset,
        "error_estimate": lambda: ctx.error_estimate(**a), "error_reset": ctx.error_reset,
        "adaptive_begin": lambda: ctx.adaptive_begin(**a), "adaptive_set_mask": lambda: ctx.adaptive_set_mask(a["tiles"]),
        "robust_begin": lambda: ctx.robust_begin(a["buckets"]), "robust_accumulate": ctx.robust_accumulate, "robust_resolve": lambda: ctx.robust_resolve(**a),
        "robust_end": ctx.robust_end, "robust_error_estimate": lambda: ctx.robust_error_estimate(**a), "robust_denoise": lambda: ctx.robust_denoise(**a),
        "robust_adaptive_begin": lambda: ctx.robust_adaptive_begin(**a), "robust_adaptive_accumulate": ctx.robust_adaptive_accumulate,
        "robust_adaptive_set_mask": lambda: ctx.robust_adaptive_set_mask(a["tiles"]), "robust_adaptive_resolve": lambda: ctx.robust_adaptive_resolve(**a),
        "robust_adaptive_end": ctx.robust_adaptive_end,
    }[k]
    return status_of(call)[0], None


def names_the_entry_point(ctx, step):
    text = ctx.lib.rtgl_last_error(ctx.h)
    if step.kind == "set_option":
        return step.args["key"].encode() in text
    if step.kind == "render":
        return b"u_samples" in text
    return b"rtgl_" + step.kind.encode() + b":" in text          # (robust_adaptive_* included: no name of a call is the head of another's)


# ---------------------------------------------------------------------------------------------- the plain twin and the model, once per seed

class Twin:
    """tracer of post_sequence_model.walk over a second context.  rows: the global rows of a tiled context under test, whose model holds
    only those; the twin holds the whole picture"""

    def __init__(self, rt, oracle, seq, rows=None):
        self.oracle, self.seq, self.rows = oracle, seq, rows
        self.ctx = rt.host.Context(seq.W, seq.H)
        self.ctx.upload_scene(seq.scene)
        self.known = np.zeros((seq.H, seq.W, 4), f32)                  # what the twin's image holds
        self.base, self.run, self.bad, self.frames = None, [], [], 0

    def local(self, a):
        return a if self.rows is None else np.ascontiguousarray(a[self.rows])

    def end_run(self):
        """the run of ordinary frames that just ended, against the CPU oracle"""
        if self.run and self.rows is None:
            img = self.base.copy()
            for p in self.run:
                self.oracle.render(self.seq.scene, p, img, threads=16)
            if not same(img, self.known):
                self.bad.append(f"the twin's image after {len(self.run)} frames ending with frames = {self.run[-1].frames} differs from the oracle")
        self.run = []

    def hold(self, image):
        """the model's image has moved on without the twin: write it"""
        full = image if self.rows is None else self.known.copy()
        if self.rows is not None:
            full[self.rows] = image
        if not same(full, self.known):
            self.end_run()
            self.ctx.write_image(full)
            self.known = np.array(full, f32)

    def __call__(self, step, params, model):
        k, a, ctx = step.kind, step.args, self.ctx
        if k == "set_aov":
            self.end_run()
            ctx.set_aov(a["mask"])
        elif k in ("clear_image", "adaptive_begin"):                   # (rtgl_adaptive_begin clears "exactly as rtgl_clear_image does")
            self.end_run()
            ctx.clear_image()
            self.known = np.zeros_like(self.known)
        elif k == "render":
            self.hold(model.image)
            if not self.run:
                self.base = self.known
            ctx.render(params)
            self.known = ctx.read_image()
            self.run.append(params)
            self.frames += 1
            return dict(image=self.local(self.known), planes={bit: self.local(ctx.read_aov(bit)) for bit in pm.BITS if model.aov & bit})
        elif k in ps.MASKED_FRAMES:                                    # the full one-frame sample: the model takes the active tiles from it
            self.end_run()
            p = params.replace(frames=0, reset_flag=1)
            ctx.clear_image()                                          # (a frame traces the footprint only: outside it the sample is +0, not what the twin held;
            ctx.render(p)                                              #  "aov" is 0 here, so the clear restarts nothing)
            self.known = ctx.read_image()
            want = np.zeros_like(self.known)
            self.oracle.render(self.seq.scene, p, want, threads=16)
            if not same(want, self.known):
                self.bad.append("the twin's one-frame sample of a masked frame differs from the oracle")
            self.frames += 1
            return dict(sample=self.known)
        return None

    def close(self):
        self.end_run()
        self.ctx.close()


_expected = {}


def expected(rt, oracle, seed, tiling=None):
    """(sequence, resolved steps, the model's walk) once per seed and tiling, never written to afterwards"""
    key = (seed, tuple(sorted(tiling.items())) if tiling else None)
    if key not in _expected:
        seq = ps.sequence(seed)
        steps = [ps.resolved(seq, s) for s in seq.steps]
        rows = None
        if tiling:
            probe = rt.host.Context(seq.W, seq.H, **tiling)
            rows = probe.global_rows()
            probe.close()
        local = [ps.Step(s.kind, dict(s.args, pixels=s.args["pixels"][rows])) if rows is not None and s.kind == "write_image" else s for s in steps]
        twin = Twin(rt, oracle, seq, rows)
        model = pm.PostModel(len(rows) if rows is not None else seq.H, seq.W, tiled=bool(tiling))
        walk = pm.walk(model, local, twin, lambda s: ps.frame_params(seq.base, s.args))
        twin.close()
        assert not twin.bad, "\n".join(twin.bad)
        assert twin.frames >= 4
        _expected[key] = (seq, steps, [(st, normalise(out), summary) for st, out, summary in walk], rows)
    return _expected[key]


# ---------------------------------------------------------------------------------------------- the runs

def run_checked(rt, seq, steps, walk, who, rows=None, bound=0, before=None, **tiling):
    """one context through the steps with every read-out after every step: the differing steps, one line each"""
    ctx = rt.host.Context(seq.W, seq.H, **tiling)
    ctx.upload_scene(seq.scene)
    if before:
        before(ctx)
    lines, prev = [], read_all(ctx)
    for i, (s, (status, want, summary)) in enumerate(zip(steps, walk)):
        rc, got_summary = apply(ctx, seq, s, rows, bound)
        d = []
        if rc != status:
            d.append(f"status {rc}, the model says {status}")
        elif rc != 0 and not names_the_entry_point(ctx, s):
            d.append(f"rtgl_last_error does not name the call: {ctx.lib.rtgl_last_error(ctx.h)[:80]!r}")
        got = read_all(ctx)
        d += differing(got, want)
        if rc != 0:
            d += [f"{name} changed by a refused call" for name in differing(got, prev)]
        if summary is not None and (got_summary is None or am.same_summary(got_summary, summary)):
            d.append(f"the summary of {s.kind}: {got_summary}, the model says {summary}")
        if d:
            lines.append(f"{who} step {i} {s.kind} {({k: v for k, v in s.args.items() if not isinstance(v, np.ndarray)})}: " + "; ".join(d) + f" | {seq.W} x {seq.H} {seq.units}")
            print(lines[-1], flush=True)
        prev = got
    return ctx, lines


def run_blind(rt, seq, steps, walk, who, options=()):
    """the same steps, nothing synchronised on purpose and no read-out until the end: the statuses, and every read-out at the end"""
    ctx = rt.host.Context(seq.W, seq.H)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_scene(seq.scene)
    lines = []
    for i, (s, (status, _, summary)) in enumerate(zip(steps, walk)):
        rc, got_summary = apply(ctx, seq, s, sync=False)
        if rc != status:
            lines.append(f"{who} step {i} {s.kind}: status {rc}, the model says {status}")
        if summary is not None and (got_summary is None or am.same_summary(got_summary, summary)):
            lines.append(f"{who} step {i}: the summary of {s.kind}: {got_summary}, the model says {summary}")
    d = differing(read_all(ctx), walk[-1][1])
    if d:
        lines.append(f"{who} at its end: " + "; ".join(d) + f" | {seq.W} x {seq.H} {seq.units}")
    ctx.close()
    for line in lines:
        print(line, flush=True)
    return lines


def test_every_step_matches_the_model(rt, oracle):
    t0, bad, steps_run, refused = time.perf_counter(), 0, 0, 0
    rd = {K: 0 for K in ps.BUCKETS}
    rd.update({pm.INVALID: 0, pm.STATE: 0})                            # robust_denoise: accepted per K of the session, and the two refusals
    ra = {K: 0 for K in ps.BUCKETS}                                    # the robust adaptive session: accepted updates per K, resolves per destination, the refusals
    ra.update({"buffer": 0, "image": 0, pm.INVALID: 0, pm.STATE: 0})
    for seed in seeds():
        seq, steps, walk, _ = expected(rt, oracle, seed)
        t1 = time.perf_counter()
        ctx, lines = run_checked(rt, seq, steps, walk, f"sequence {seed}")
        ctx.close()
        bad += len(lines)
        steps_run += len(steps)
        refused += sum(st != 0 for st, _, _ in walk)
        for s, (st, out, _) in zip(steps, walk):
            if s.kind == "robust_denoise":
                rd[st if st else out["robust_frames"][1]] += 1
            if s.kind.startswith("robust_adaptive") and st:
                ra[st] += 1
            elif s.kind == "robust_adaptive_update":
                ra[out["robust_adaptive_buckets"].shape[0]] += 1
            elif s.kind == "robust_adaptive_resolve":
                ra["image" if s.args["dest"] else "buffer"] += 1
        print(f"sequence {seed} {seq.W} x {seq.H}: {len(steps)} steps, device part {time.perf_counter() - t1:.2f} s", flush=True)
    print(f"sequences {len(seeds())} steps {steps_run} refused {refused} | differing steps: {bad} | {time.perf_counter() - t0:.2f} s with twin, oracle and model", flush=True)
    print("robust_denoise: accepted " + ", ".join(f"{rd[K]} at K = {K}" for K in ps.BUCKETS) + f"; {rd[pm.INVALID]} times -1, {rd[pm.STATE]} times -4", flush=True)
    print("robust_adaptive: accepted updates " + ", ".join(f"{ra[K]} at K = {K}" for K in ps.BUCKETS) + f"; resolves {ra['buffer']} into the buffer, {ra['image']} into the image; "
          f"{ra[pm.INVALID]} times -1, {ra[pm.STATE]} times -4", flush=True)
    assert bad == 0, f"{bad} steps of {len(seeds())} sequences differ from the model (see the lines printed above)"
    assert refused * 10 >= steps_run, "hardly a step was refused"
    if len(seeds()) >= len(ps.ROWS):                                   # every row is among them
        assert all(rd[k] >= 1 for k in rd), rd
        assert all(ra[k] >= 1 for k in ra), ra


def test_the_same_sequence_without_intermediate_read_outs_ends_on_the_same_bits(rt, oracle):
    t0, bad = time.perf_counter(), 0
    for seed in seeds():
        seq, steps, walk, _ = expected(rt, oracle, seed)
        bad += len(run_blind(rt, seq, steps, walk, f"sequence {seed}, no read-outs"))
    print(f"no read-outs: {len(seeds())} sequences, {time.perf_counter() - t0:.2f} s", flush=True)
    assert bad == 0, f"{bad} differences (see the lines printed above)"


def test_batched_frames_change_nothing(rt, oracle):
    """"frame_batch" = 3: the frames of the stretches with "aov" = 0 are held back, and every other call has to submit them first"""
    t0, bad, held = time.perf_counter(), 0, 0
    for seed in seeds():
        seq, steps, walk, _ = expected(rt, oracle, seed)
        aov = 0
        for s, (st, _, _) in zip(steps, walk):
            aov = s.args["mask"] if s.kind == "set_aov" and st == 0 else aov
            held += s.kind == "render" and aov == 0
        bad += len(run_blind(rt, seq, steps, walk, f"sequence {seed}, frame_batch 3", options=(("frame_batch", 3),)))
    print(f"frame_batch 3: {len(seeds())} sequences, {held} frames with aov off, {time.perf_counter() - t0:.2f} s", flush=True)
    assert bad == 0, f"{bad} differences (see the lines printed above)"
    assert held >= 3 * len(seeds())


def test_bound_image_on_a_torch_stream_changes_nothing(rt, oracle):
    """the image in a torch tensor, the context on a torch side stream (tests/test_gpu_torch_plumbing.py).  The bind is the epoch and
    session event the header says it is: before the first step it changes nothing a call can see; a "bind_image" step binds the same tensor"""
    import torch
    t0, bad, done = time.perf_counter(), 0, set()
    dev = torch.device("cuda", 0)
    for seed in seeds():
        seq, steps, walk, _ = expected(rt, oracle, seed)
        accepts = lambda kind: any(s.kind == kind and st == 0 for s, (st, _, _) in zip(steps, walk))
        key = (seq.W, seq.H, accepts("robust_denoise"), accepts("robust_adaptive_update"))
        if key in done:                                                # per size: the first sequence, and the first in which rtgl_robust_denoise, the first in which
            continue                                                   # rtgl_robust_adaptive_update is accepted
        done.add(key)
        tensor = torch.zeros((seq.H, seq.W, 4), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            def bind(ctx):
                ctx.bind_device_image(tensor.data_ptr())
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx, lines = run_checked(rt, seq, steps, walk, f"sequence {seed}, bound image", bound=tensor.data_ptr(), before=bind)
            side.synchronize()
        if not same(tensor.cpu().numpy(), walk[-1][1]["image"]):
            lines.append(f"sequence {seed}: the tensor does not hold the model's image at the end")
            print(lines[-1], flush=True)
        ctx.bind_device_image(0)                                       # detached before the tensor goes away
        ctx.set_stream(0)
        ctx.close()
        bad += len(lines)
    print(f"bound image: {len(done)} sequences, {time.perf_counter() - t0:.2f} s", flush=True)
    assert bad == 0 and len({k[:2] for k in done}) == min(len(ps.SIZES), len(seeds())), f"{bad} differing steps (see the lines printed above)"
    if len(seeds()) >= len(ps.ROWS):
        assert {k[:2] for k in done if k[2]} == set(ps.SIZES), "rtgl_robust_denoise on a torch stream at every size"
        assert {k[:2] for k in done if k[3]} == set(ps.SIZES), "rtgl_robust_adaptive_update on a torch stream at every size"


def test_a_tiled_context_refuses_or_works_as_the_header_says(rt, oracle):
    """rank 1 of 2, strips of 8 rows, 48 x 40: the robust session works on the local rows; every other post-process call that looks at
    the picture, every call of a robust adaptive session among them, is RTGL_ERR_STATE and leaves the context as it was"""
    t0, bad, n, robust_ok, refused, ra_refused = time.perf_counter(), 0, 0, 0, 0, 0
    tiling = dict(rank=1, world=2, strip_rows=8)
    for seed in seeds():
        if ps.size_of(seed) != (48, 40) or n == ps.DEFAULT_SEQUENCES // len(ps.SIZES):
            continue
        n += 1
        seq, steps, walk, rows = expected(rt, oracle, seed, tiling)
        assert len(rows) == 16 and (rows == np.r_[8:16, 24:32]).all()
        for s, (st, out, _) in zip(steps, walk):
            if s.kind in ("denoise", "denoise_guided", "temporal_accumulate", "temporal_clip", "tonemap", "error_estimate", "robust_error_estimate", "robust_denoise") or s.kind.startswith(("adaptive", "robust_adaptive")):
                assert st in (pm.STATE, pm.INVALID), (s.kind, st)
                refused += st == pm.STATE
                ra_refused += s.kind.startswith("robust_adaptive")
            robust_ok += st == 0 and s.kind in ("robust_accumulate", "robust_resolve")
        ctx, lines = run_checked(rt, seq, steps, walk, f"sequence {seed}, rank 1 of 2", rows=rows, **tiling)
        ctx.close()
        bad += len(lines)
    print(f"tiled: {n} sequences, {robust_ok} robust folds and resolves, {refused} refusals, {ra_refused} robust_adaptive steps all refused, {time.perf_counter() - t0:.2f} s", flush=True)
    assert bad == 0, f"{bad} differing steps (see the lines printed above)"
    assert n >= 1 and robust_ok >= 2 and refused >= 10
    if len(seeds()) >= len(ps.ROWS):                                   # the three robust adaptive rows of 48 x 40 are among them
        assert n == ps.DEFAULT_SEQUENCES // len(ps.SIZES) and refused >= 120 and ra_refused >= 60, (n, refused, ra_refused)
