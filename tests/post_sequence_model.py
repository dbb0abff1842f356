"""The host state of ONE context across the post-process calls, restated from include/rtgl_amd.h alone, for the call sequences of
tests/post_sequence_inputs.py.  A helper, not a test; numpy, no device.

PostModel(h, w) composes the mirrors the suite already has -- denoise_mirror, denoise_guided_mirror, temporal_mirror,
temporal_moments_mirror, temporal_clip_mirror, tonemap_mirror.Tonemapper, error_mirror.Estimator, adaptive_mirror.Session,
robust_mirror.Session, robust_error_mirror.estimate, robust_denoise_mirror.robust_denoise, robust_adaptive_mirror.Session -- and adds no
arithmetic of its own: what it adds is WHICH buffer a call reads, which state a call drops, and when a call is refused, each taken from
a sentence of the header (quoted where it is used).  It never reads rtgl_amd.hip and is never fed anything the context under test
produced.

  status_of(step)          the status the header gives the step in the current state: 0, -1 (RTGL_ERR_INVALID) or -4 (RTGL_ERR_STATE).
                           A bad argument is reported before the state (header, "rtgl_status").
  step(step, traced, params)  the same status; on 0 the state moves on.  A refused step changes nothing, with one exception that is not one:
                           a frame step is rtgl_set_frame_params, which succeeds, and then the frame call, so the CURRENT camera of
                           rtgl_temporal_accumulate is that of the latest frame step, refused or not.
                           traced: for an accepted "render" dict(image=the image after the frame, planes={bit: plane after the frame});
                           for an accepted "adaptive_frame" or "robust_adaptive_frame" dict(sample=the full one-frame image of the
                           frame's uniforms).
  readouts()               every read-out of the header, by name: the expected contents, or REFUSED where the header says the read-out
                           returns RTGL_ERR_STATE.  Arrays are never modified in place once handed out.
  image                    the accumulation image as it must be now: what a plain twin has to hold before it traces the next frame.

PostModel(h, w, defect=name) is the model with ONE rule of the host state got wrong, a name of DEFECTS: the mistakes a host body shared by
the adaptive and the robust adaptive session makes plausible.  tests/test_post_sequence_inputs.py walks each over the default sequences:
where the walk differs from the true model's, a library with that mistake would differ from the model on the device.
"""
import numpy as np

import adaptive_mirror as am
import denoise_guided_mirror as dgm
import denoise_mirror as dm
import error_mirror as em
import robust_adaptive_mirror as ram
import robust_denoise_mirror as rdm
import robust_error_mirror as rem
import robust_mirror as rm
import temporal_clip_mirror as tcm
import temporal_mirror as tm
import temporal_moments_mirror as mm
import tonemap_mirror as tmm

f32 = np.float32
OK, INVALID, STATE = 0, -1, -4
REFUSED = "refused"
A, N, P, IDS = 1, 2, 4, 8
BITS = (A, N, P, IDS)
READOUTS = ("image", "planes", "denoised", "variance", "history", "moments", "display", "exposure", "histogram", "error_summary", "error_tiles", "adaptive_tiles",
            "adaptive_mask", "robust_buckets", "robust_output", "robust_frames", "robust_error_summary", "robust_error_tiles", "robust_adaptive_buckets",
            "robust_adaptive_output", "robust_adaptive_tiles", "robust_adaptive_mask")
FRAMES = ("render", "adaptive_frame", "robust_adaptive_frame")         # the steps that begin with rtgl_set_frame_params
UPDATES = ("adaptive_update", "robust_adaptive_update")                # the steps that return a summary
# one wrong rule each (see the module's text); every name is looked up where the rule it breaks is written
DEFECTS = ("render ends the robust adaptive session", "a replaced image ends the robust adaptive session", "adaptive_begin ends the robust adaptive session",
           "adaptive_set_mask also sets the robust adaptive mask", "adaptive_update also sets the robust adaptive mask",
           "robust_adaptive_set_mask also sets the adaptive mask", "robust_adaptive_update also sets the adaptive mask",
           "robust_adaptive_frame merges into the image", "robust_adaptive_frame drops the error snapshot",
           "robust_adaptive_begin clears the image and restarts the planes", "the resolve into the image leaves the adaptive session open",
           "the resolve into the image keeps the error snapshot", "robust_adaptive_accumulate folds the sample buffer", "a second begin keeps n",
           "a second begin keeps the mask", "a second begin leaves the output readable", "robust_adaptive_frame is accepted with aov on",
           "robust_denoise serves a robust adaptive session", "robust_error_estimate serves a robust adaptive session",
           "robust_adaptive_end ends the robust session")


def _finite(*values):
    return all(np.isfinite(f32(v)) for v in values)


class PostModel:
    def __init__(self, h, w, tiled=False, defect=None):
        """tiled: a context of rtgl_create_tiled with more than one rank, holding h x w LOCAL rows: every post-process call but the
        robust session's begin, accumulate, resolve and end is RTGL_ERR_STATE there.  defect: None, or the one rule of DEFECTS to get wrong"""
        assert defect is None or defect in DEFECTS, defect
        self.h, self.w, self.tiled, self.defect = h, w, tiled, defect
        self.image = np.zeros((h, w, 4), f32)                          # "zero-initialised"
        self.aov, self.planes = 0, {}
        self.restarted = True                                          # no frame since the planes last restarted (none yet)
        self.params = None                                             # the current rtgl_frame_params
        self.options = dict(denoise_source=0, temporal_moments=0, denoise_variance=0)
        self.denoised = self.variance = None
        self.history = self.moments = self.tstate = None               # the latest history, the latest moments, what the next accumulate reprojects
        self.stored_mode = 0                                           # the moments mode of the latest successful accumulate
        self.tone, self.display, self.exposure, self.histogram = tmm.Tonemapper(), None, None, None
        self.est, self.error = em.Estimator(), None
        self.session, self.ad_records = None, None                     # an open adaptive session; the records of the latest one
        self.robust, self.robust_output, self.robust_error = None, None, None
        self.ra, self.ra_output = None, None                           # an open robust adaptive session; its output plane once resolved into
        self.ra_sample = None                                          # (the session's sample buffer: only a defect reads it)
        self.summary = None                                            # what the latest accepted adaptive_update or robust_adaptive_update returned

    # -------------------------------------------------------------------------------------------- refusals
    def _planes_state(self, need, always=False):
        """RTGL_ERR_STATE: "a plane the parameters need is not enabled"; "a plane is needed and no frame has been rendered since the
        planes last restarted" (the temporal calls: whether or not, they always need the position plane)"""
        if need & ~self.aov:
            return STATE
        if (need or always) and self.restarted:
            return STATE
        return OK

    def _denoiser_planes(self, a):
        return (A if a["demodulate"] else 0) | (N if a["sigma_normal"] > 0 else 0) | (P if a["sigma_position"] > 0 else 0)

    def status_of(self, step):
        return getattr(self, "_status_" + step.kind, lambda a: OK)(step.args)

    def _status_render(self, a):
        return INVALID if a.get("samples", 1) == 0 else OK              # "RTGL_ERR_INVALID for samples == 0": the session stays open

    def _status_set_aov(self, a):
        return OK if 0 <= a["mask"] <= 15 else INVALID

    def _status_set_option(self, a):
        return OK if a["value"] in dict(denoise_source=(0, 1), temporal_moments=(0, 1, 2), denoise_variance=(0, 1))[a["key"]] else INVALID

    def _status_denoise(self, a):
        if not 0 <= a["passes"] <= 8 or not _finite(a["sigma_color"], a["sigma_normal"], a["sigma_position"]):
            return INVALID
        if self.tiled or self._planes_state(self._denoiser_planes(a)):
            return STATE
        return STATE if self.options["denoise_source"] == 1 and self.history is None else OK

    def _status_denoise_guided(self, a):
        if not 0 <= a["passes"] <= 8 or not _finite(a["sigma_lum"], a["sigma_normal"], a["sigma_position"], a["firefly_ratio"]) or not a["sigma_lum"] > 0:
            return INVALID
        if self.tiled or self._planes_state(self._denoiser_planes(a)):
            return STATE
        if self.options["denoise_source"] == 1 and self.history is None:
            return STATE
        if self.options["denoise_variance"] == 1:
            # "RTGL_ERR_STATE if "denoise_source" is not 1, if the latest rtgl_temporal_accumulate stored no moments, or if the stored mode
            # does not match the call: mode 2 iff RTGL_DENOISE_DEMODULATE is set, mode 1 iff it is not"
            if self.options["denoise_source"] != 1 or self.stored_mode != (2 if a["demodulate"] else 1):
                return STATE
        return OK

    def _status_temporal_accumulate(self, a):
        if not _finite(a["max_history"], a["sigma_normal"], a["sigma_position"]) or not a["max_history"] >= 1:
            return INVALID
        need = P | (N if a["sigma_normal"] > 0 else 0) | (A if self.options["temporal_moments"] == 2 else 0)
        return STATE if self.tiled or self._planes_state(need, always=True) else OK

    def _status_temporal_clip(self, a):
        if not _finite(a["sigma_scale"], a["clip_history"], a["sigma_normal"], a["sigma_position"]) or not a["sigma_scale"] > 0 or not a["clip_history"] >= 1:
            return INVALID
        if self.tiled or self.history is None:
            return STATE
        return self._planes_state(P | (N if a["sigma_normal"] > 0 else 0), always=True)

    def _status_temporal_reset(self, a):
        return OK

    def _status_tonemap(self, a):
        if a["source"] not in (0, 1, 2) or a["op"] not in (0, 1, 2) or not _finite(a["exposure"], a["adapt"]) or not a["exposure"] > 0 or not 0 < a["adapt"] <= 1:
            return INVALID
        if self.tiled or (a["source"] == 1 and self.denoised is None) or (a["source"] == 2 and self.history is None):
            return STATE
        return OK

    def _status_error_estimate(self, a):
        if a["first_frames"] < 0:
            return INVALID
        if self.tiled or self.est.fn is None:                          # "no frame has been rendered on this context": ordinary frames, see step()
            return STATE
        return INVALID if self.est.fn + 1 - a["first_frames"] < 1 else OK      # "n < 1 is RTGL_ERR_INVALID": known only once F_n is

    def _status_adaptive_begin(self, a):
        if not (_finite(a["threshold"]) and a["threshold"] > 0) or a["min_samples"] < 1 or a["max_samples"] < a["min_samples"]:
            return INVALID
        return STATE if self.tiled else OK

    def _status_adaptive_frame(self, a):
        if self.tiled or self.session is None or self.aov:            # "no session"; "option "aov" ... non-zero"
            return STATE
        # "at rtgl_adaptive_frame: samples != 1 ... in the frame parameters"; "Two checks need the context and come after its state: ...
        # samples / max_bounce of rtgl_adaptive_frame and of rtgl_robust_adaptive_frame"
        return INVALID if a.get("samples", 1) != 1 else OK

    def _status_adaptive_update(self, a):
        return STATE if self.tiled or self.session is None else OK

    _status_adaptive_set_mask = _status_adaptive_update

    def _status_robust_begin(self, a):
        return OK if a["buckets"] in rm.BUCKETS else INVALID

    def _status_robust_accumulate(self, a):
        return STATE if self.robust is None else OK

    def _status_robust_resolve(self, a):
        if not rm.valid_resolve_params(a["gain"], a["dest"]):
            return INVALID
        return STATE if self.robust is None or self.robust.N == 0 else OK

    def _status_robust_end(self, a):
        return STATE if self.robust is None else OK

    def _status_robust_error_estimate(self, a):
        if not rem.valid_params(a["threshold"], a["floor"], a["gain"], 950):
            return INVALID
        if self._served_by_defect("robust_error_estimate serves a robust adaptive session"):
            return OK
        # "rtgl_robust_denoise and rtgl_robust_error_estimate serve the plain robust session only"
        if self.tiled or rem.refused(self.robust is not None, self.robust.N if self.robust else 0, self.robust.K if self.robust else 0):
            return STATE
        return OK

    def _served_by_defect(self, name):
        """(a defect) no plain session, and a robust adaptive one in which some tile holds K samples"""
        return self.defect == name and not self.tiled and self.robust is None and self.ra is not None and int(self.ra.n.max()) >= self.ra.K

    def _status_robust_denoise(self, a):
        # "RTGL_ERR_INVALID: ... passes > 8, a non-finite sigma, sigma_lum <= 0, gain NaN, negative or infinite"
        if not rdm.valid_params(a["passes"], a["sigma_lum"], a["sigma_normal"], a["sigma_position"], a["gain"]):
            return INVALID
        # "RTGL_ERR_STATE: no session; N < K (an empty bucket has no luminance); a tiled or multi-device context; ..."
        if self.tiled or ((self.robust is None or self.robust.N < self.robust.K) and not self._served_by_defect("robust_denoise serves a robust adaptive session")):
            return STATE
        # "... a plane the parameters need is not enabled; a plane is needed and no frame has been rendered since the planes last
        # restarted (the conditions of rtgl_denoise_guided)": with no plane needed the restart does not refuse
        return self._planes_state(self._denoiser_planes(a))

    def _status_robust_adaptive_begin(self, a):
        # "RTGL_ERR_INVALID: ... buckets not 4, 8 or 16; threshold or floor not finite or not > 0; gain NaN, negative or infinite;
        # min_samples < K; max_samples < min_samples or > 16777216"
        if not ram.valid_params(a["buckets"], a["threshold"], a["floor"], a["gain"], a["min_samples"], a["max_samples"]):
            return INVALID
        return STATE if self.tiled else OK                             # "a tiled or multi-device context"

    def _status_robust_adaptive_frame(self, a):
        # "RTGL_ERR_STATE: no session (every call but begin and defaults); a tiled or multi-device context; ... rtgl_robust_adaptive_frame
        # ... with option "aov" ... non-zero"
        if self.tiled or self.ra is None or (self.aov and self.defect != "robust_adaptive_frame is accepted with aov on"):
            return STATE
        return INVALID if a.get("samples", 1) != 1 else OK             # "at rtgl_robust_adaptive_frame: samples != 1": after the state, see above

    def _status_robust_adaptive_update(self, a):
        return STATE if self.tiled or self.ra is None else OK

    _status_robust_adaptive_accumulate = _status_robust_adaptive_set_mask = _status_robust_adaptive_end = _status_robust_adaptive_update

    def _status_robust_adaptive_resolve(self, a):
        if not rm.valid_resolve_params(a["gain"], a["dest"]):          # "dest > 1", and the gain of rtgl_robust_resolve_params
            return INVALID
        return STATE if self.tiled or self.ra is None else OK

    # -------------------------------------------------------------------------------------------- events several calls share
    def _image_replaced(self):
        """what rtgl_write_image_f32 does on the host, and with it rtgl_clear_image, rtgl_bind_device_image and rtgl_robust_resolve into
        the image: "an adaptive session ends, the snapshot of rtgl_error_estimate is dropped" """
        self.est.drop()
        self.session = None                                            # "The events that end an adaptive session do not end this one"
        if self.defect == "a replaced image ends the robust adaptive session":
            self._do_robust_adaptive_end(None, None)                   # (a defect)

    def _source(self):
        """what the denoisers filter: "0 (default) ... the image; 1 they take the latest history buffer wherever they take the image" """
        return self.history if self.options["denoise_source"] == 1 else self.image

    def _plane(self, bit):
        return self.planes.get(bit) if self.aov & bit else None

    # -------------------------------------------------------------------------------------------- one step
    def step(self, step, traced=None, params=None):
        """params: the uniforms of a frame step (rtgl_set_frame_params, which comes first and succeeds whatever becomes of the frame)"""
        a = step.args
        if step.kind in FRAMES:
            self.params = params
        status = self.status_of(step)
        if status == OK:
            getattr(self, "_do_" + step.kind)(a, traced)
        return status

    def _do_render(self, a, traced):
        self.session = None                                            # "rtgl_render_frame ... END the session"
        if self.defect == "render ends the robust adaptive session":
            self._do_robust_adaptive_end(a, traced)
        self.est.frame(a["frames"], a["reset_flag"])                   # "any rendered frame with reset_flag != 0" drops the snapshot; F_n
        self.image = traced["image"]
        self.planes = {bit: traced["planes"][bit] for bit in BITS if self.aov & bit}
        if self.aov:                                                   # (without planes nothing restarts or counts: no call can tell)
            self.restarted = False

    def _do_write_image(self, a, traced):
        self.image = np.array(a["pixels"], f32)
        self._image_replaced()

    def _do_clear_image(self, a, traced):
        self.image = np.zeros((self.h, self.w, 4), f32)
        self.restarted = True                                          # "n restarts at 1 ... on the first frame after rtgl_clear_image"
        self._image_replaced()

    def _do_bind_image(self, a, traced):
        self._image_replaced()                                         # (the caller's buffer holds what the image held: the tests see to that)

    def _do_set_aov(self, a, traced):
        self.aov = a["mask"]                                           # "allocates the enabled planes zeroed (and frees the others)"
        self.planes = {bit: np.zeros((self.h, self.w, 4), np.int32 if bit == IDS else f32) for bit in BITS if self.aov & bit}
        self.restarted = True

    def _do_set_option(self, a, traced):
        if a["key"] == "temporal_moments" and a["value"] != self.options["temporal_moments"]:
            self.tstate = None                                         # "acts like rtgl_temporal_reset"
        self.options[a["key"]] = a["value"]

    def _do_denoise(self, a, traced):
        self.denoised = dm.denoise(self._source(), self._plane(A), self._plane(N), self._plane(P), passes=a["passes"], sigma_color=a["sigma_color"],
                                   sigma_normal=a["sigma_normal"], sigma_position=a["sigma_position"], demodulate=a["demodulate"])

    def _do_denoise_guided(self, a, traced):
        ps = dict(passes=a["passes"], sigma_lum=a["sigma_lum"], sigma_normal=a["sigma_normal"], sigma_position=a["sigma_position"], firefly_ratio=a["firefly_ratio"],
                  demodulate=a["demodulate"])
        if self.options["denoise_variance"] == 1:
            self.denoised, self.variance = mm.denoise_guided_tvar(self.history, self.moments, self._plane(A), self._plane(N), self._plane(P), **ps)
        else:
            self.denoised, self.variance = dgm.denoise_guided(self._source(), self._plane(A), self._plane(N), self._plane(P), **ps)

    def _do_temporal_accumulate(self, a, traced):
        mode = self.options["temporal_moments"]
        ps = dict(max_history=a["max_history"], sigma_normal=a["sigma_normal"], sigma_position=a["sigma_position"])
        if mode:
            self.tstate = mm.accumulate(self.tstate, self.image, self._plane(N), self._plane(P), self.params, albedo=self._plane(A), mode=mode, **ps)
        else:
            self.tstate = tm.accumulate(self.tstate, self.image, self._plane(N), self._plane(P), self.params, **ps)
        self.history, self.moments, self.stored_mode = self.tstate["H"], self.tstate.get("M"), mode

    def _do_temporal_reset(self, a, traced):
        self.tstate = None                                             # (the latest history stays readable, and rtgl_temporal_clip still clips it)

    def _do_temporal_clip(self, a, traced):
        self.history, self.moments = tcm.clip(self.history, self.moments, self.image, self._plane(N), self._plane(P), sigma_scale=a["sigma_scale"],
                                               clip_history=a["clip_history"], sigma_normal=a["sigma_normal"], sigma_position=a["sigma_position"])
        if self.tstate is not None:                                    # "the next rtgl_temporal_accumulate reprojects it"
            self.tstate = dict(self.tstate, H=self.history)
            if self.moments is not None:
                self.tstate["M"] = self.moments

    def _do_tonemap(self, a, traced):
        src = (self.image, self.denoised, self.history)[a["source"]]
        out = self.tone(src, op=a["op"], auto=a["auto"], exposure=a["exposure"], adapt=a["adapt"])
        self.display, self.exposure = out["display"], out["exposure"]
        if out["hist"] is not None:                                    # "of the latest call WITH auto exposure"
            self.histogram = (out["hist"], out["ignored"])

    def _do_tonemap_reset(self, a, traced):
        self.tone.reset()

    def _do_error_estimate(self, a, traced):
        self.error = self.est(self.image, keep_snapshot=a["keep_snapshot"], first_frames=a["first_frames"])

    def _do_error_reset(self, a, traced):
        self.est.drop()

    def _do_adaptive_begin(self, a, traced):
        # "zeroes the image exactly as rtgl_clear_image does (the error snapshot is dropped, the planes' count restarts)"
        self._do_clear_image(a, traced)
        self.session = am.Session(self.h, self.w, threshold=a["threshold"], min_samples=a["min_samples"], max_samples=a["max_samples"])
        self.ad_records = self.session.records
        if self.defect == "adaptive_begin ends the robust adaptive session":
            self._do_robust_adaptive_end(a, traced)

    def _do_adaptive_frame(self, a, traced):
        self.est.drop()                                                # "A masked frame drops the snapshot of rtgl_error_estimate"
        self.session.image = self.image                                # (rtgl_robust_accumulate and the read-only calls leave it as it was)
        self.session.frame(traced["sample"])
        self.image = self.session.image

    def _do_adaptive_update(self, a, traced):
        self.session.image = self.image
        self.summary = self.session.update()
        self.ad_records = self.session.records
        if self.defect == "adaptive_update also sets the robust adaptive mask" and self.ra is not None:
            self.ra.mask = self.session.mask

    def _do_adaptive_set_mask(self, a, traced):
        self.session.set_mask(a["tiles"])
        if self.defect == "adaptive_set_mask also sets the robust adaptive mask" and self.ra is not None:
            self.ra.set_mask(a["tiles"])

    def _do_robust_begin(self, a, traced):
        self.robust, self.robust_output, self.robust_error = rm.Session(self.h, self.w, a["buckets"]), None, None

    def _do_robust_accumulate(self, a, traced):
        self.robust.planes = self.robust.planes.copy()                 # (arrays handed out are never modified in place)
        self.robust.accumulate(self.image)

    def _do_robust_resolve(self, a, traced):
        out = self.robust.resolve(a["gain"], a["dest"])
        if a["dest"] == rm.DEST_IMAGE:
            self.image = out
            self._image_replaced()                                     # "the first-hit planes and their count stay as they are"
        else:
            self.robust_output = out

    # a robust adaptive session.  "The session is independent of an adaptive session and of a robust session: either may be open beside
    # it, and neither is read or written.  The events that end an adaptive session do not end this one: only rtgl_robust_adaptive_end does."
    def _do_robust_adaptive_begin(self, a, traced):
        # "a second begin restarts the session ..., zeroes the buckets, n, m and the records and sets active every tile that holds a
        # footprint pixel.  It does not touch the image."
        old, output = self.ra, self.ra_output
        self.ra = ram.Session(self.h, self.w, **a)
        self.ra_output, self.ra_sample = None, np.zeros((self.h, self.w, 4), f32)      # "before a resolve with dest BUFFER": since this begin
        if old is not None:
            if self.defect == "a second begin keeps n":
                self.ra.n = old.n
            if self.defect == "a second begin keeps the mask":
                self.ra.mask = old.mask
            if self.defect == "a second begin leaves the output readable":
                self.ra_output = output
        if self.defect == "robust_adaptive_begin clears the image and restarts the planes":
            self._do_clear_image(a, traced)

    def _do_robust_adaptive_frame(self, a, traced):
        # "into the session's sample buffer, and then runs the FOLD with that buffer as the source.  It writes neither the image nor
        # anything of rtgl_error_estimate."
        on = am.active_pixels(self.h, self.w, self.ra.mask)[..., None]
        self.ra_sample = np.where(on, traced["sample"], self.ra_sample)
        if self.defect == "robust_adaptive_frame merges into the image":
            self.image = am.merge(self.image, traced["sample"], self.ra.n, self.ra.mask)[0]
        if self.defect == "robust_adaptive_frame drops the error snapshot":
            self.est.drop()
        self.ra.fold(traced["sample"])

    def _do_robust_adaptive_accumulate(self, a, traced):
        # "runs the fold with the accumulation image AS IT STANDS as the source"
        self.ra.fold(self.ra_sample if self.defect == "robust_adaptive_accumulate folds the sample buffer" else self.image)

    def _do_robust_adaptive_update(self, a, traced):
        self.summary = self.ra.update()
        if self.defect == "robust_adaptive_update also sets the adaptive mask" and self.session is not None:
            self.session.mask = self.ra.mask

    def _do_robust_adaptive_set_mask(self, a, traced):
        self.ra.set_mask(a["tiles"])
        if self.defect == "robust_adaptive_set_mask also sets the adaptive mask" and self.session is not None:
            self.session.set_mask(a["tiles"])

    def _do_robust_adaptive_resolve(self, a, traced):
        out = self.ra.resolve(a["gain"], a["dest"])
        if a["dest"] == ram.DEST_BUFFER:                               # "in the session's output plane ...; nothing else changes"
            self.ra_output = out
            return
        # "stores all four components in the accumulation image and does on the host exactly what rtgl_robust_resolve with dest IMAGE
        # does: an adaptive session ends, the snapshot of rtgl_error_estimate is dropped.  The session goes on after either."
        self.image = out
        session = self.session
        keep = self.defect == "the resolve into the image keeps the error snapshot"
        if keep:
            saved = dict(vars(self.est))
        self._image_replaced()
        if keep:
            vars(self.est).update(saved)
        if self.defect == "the resolve into the image leaves the adaptive session open":
            self.session = session

    def _do_robust_adaptive_end(self, a, traced):
        self.ra = self.ra_output = self.ra_sample = None
        if self.defect == "robust_adaptive_end ends the robust session":
            self.robust = self.robust_output = self.robust_error = None

    def _do_robust_end(self, a, traced):
        self.robust = self.robust_output = self.robust_error = None

    def _do_robust_error_estimate(self, a, traced):
        if self.defect == "robust_error_estimate serves a robust adaptive session" and self.robust is None:
            return                                                     # (a defect: accepted, and no plain session whose read-outs could show it)
        self.robust_error = rem.estimate(self.robust.planes, self.robust.N, threshold=a["threshold"], floor=a["floor"], gain=a["gain"])

    def _do_robust_denoise(self, a, traced):
        # "The result is in the DENOISED and the VARIANCE buffer of the denoisers ... and nothing else: the buckets, the output plane and
        # the session's error records are only read or not touched, and so are the image, the first-hit planes, the snapshot of
        # rtgl_error_estimate and an adaptive session.  The session goes on."  It filters the buckets, never the image or the history:
        # "denoise_source" and "denoise_variance" do not enter
        planes, n = self.robust.planes if self.robust is not None else None, self.robust.N if self.robust is not None else 0
        if self._served_by_defect("robust_denoise serves a robust adaptive session"):
            planes, n = self.ra.planes, int(self.ra.n.max())           # (a defect: the other session's buckets)
        self.denoised, self.variance = rdm.robust_denoise(planes, n, self._plane(A), self._plane(N), self._plane(P), passes=a["passes"],
                                                          sigma_lum=a["sigma_lum"], sigma_normal=a["sigma_normal"], sigma_position=a["sigma_position"],
                                                          gain=a["gain"], demodulate=a["demodulate"])

    # -------------------------------------------------------------------------------------------- read-outs
    def readouts(self):
        r = lambda v: REFUSED if v is None else v
        if self.tiled:
            out = {k: REFUSED for k in READOUTS}
            out.update(image=self.image, planes={bit: self.planes.get(bit, REFUSED) for bit in BITS})
        else:
            out = dict(image=self.image, planes={bit: self.planes.get(bit, REFUSED) if self.aov & bit else REFUSED for bit in BITS},
                       denoised=r(self.denoised), variance=r(self.variance), history=r(self.history), moments=r(self.moments if self.stored_mode else None),
                       display=r(self.display), exposure=r(self.exposure), histogram=r(self.histogram),
                       error_summary=r(self.error), error_tiles=REFUSED if self.error is None else self.error["tiles"],
                       adaptive_tiles=r(self.ad_records), adaptive_mask=REFUSED if self.session is None else self.session.mask)
        rb = self.robust
        out.update(robust_buckets=REFUSED if rb is None else rb.planes, robust_output=REFUSED if rb is None else r(self.robust_output),
                   robust_frames=REFUSED if rb is None else (rb.N, rb.K))
        ra = None if self.tiled else self.ra                           # "RTGL_ERR_STATE: no session ...; a tiled or multi-device context; rtgl_read_robust_adaptive_f32 before a resolve with dest BUFFER"
        out.update(robust_adaptive_buckets=REFUSED if ra is None else ra.planes, robust_adaptive_output=REFUSED if ra is None else r(self.ra_output),
                   robust_adaptive_tiles=REFUSED if ra is None else ra.records, robust_adaptive_mask=REFUSED if ra is None else ra.mask)
        if not self.tiled:
            out.update(robust_error_summary=REFUSED if rb is None else r(self.robust_error),
                       robust_error_tiles=REFUSED if rb is None or self.robust_error is None else self.robust_error["tiles"])
        return out


def walk(model, steps, tracer, params_of=None):
    """the model through `steps`: [(status, read-outs after the step, the summary an accepted adaptive_update or robust_adaptive_update
    returned or None)].
    tracer(step, params, model) is called before every step the model accepts and returns what step() wants as `traced` (None where the
    step traces nothing); it is where a plain twin follows the writers of the image.  params_of(step): the uniforms of a frame step."""
    out = []
    for s in steps:
        params = params_of(s) if params_of and s.kind in FRAMES else None
        traced = tracer(s, params, model) if model.status_of(s) == OK else None
        status = model.step(s, traced, params)
        out.append((status, model.readouts(), model.summary if status == OK and s.kind in UPDATES else None))
    return out
