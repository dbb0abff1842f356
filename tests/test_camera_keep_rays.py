"""The jitter bound of the kept camera bits (raytracer.glsl_amd/csrc/rt_camera_keep.hpp, widening()) against real camera rays, without a GPU.

packet_cull_kernel widens a granule's origin radius by ro_add and its direction spread by sigma_add when it computes the bits that later
frames of the camera reuse.  The two numbers must bound how far any frame's depth-of-field jitter moves a camera ray.  Here: for every
camera of tests/camera_keep_inputs.py that widening() accepts, the CPU oracle's bounce-0 rays of 16 frames (GlibcRand(3) random words) at
40 x 24 and at 53 x 35 (footprint 48 x 32 of a 53-wide image), and in float64 on the float32 values, over ALL pairs of frames (any frame may
be the one that built the bits):   max |o_k - o_j| <= ro_add   and   max |d_k - d_j| <= sigma_add.

Rays with a NaN component are left out; their share is 0 in every family but skew, where the camera with a zero forward vector has exactly
one such pixel per frame at 40 x 24 (ndc (0, 0): the direction is 0 / 0) and none at 53 x 35, and every other skew camera none.
Cameras that widening() refuses are refused for the documented reasons only (refusal_reasons).  For the tame family the largest observed direction
chord is at least 0.7 of sigma_add: the bound is not slack by construction.

The header's widening() and decide() are reached through tests/cpp/camera_keep_shim.cpp, built with the host compiler.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_keep_inputs as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((40, 24), (53, 35))
FRAMES = 16
CAMERAS = ck.cameras()


def build_shim(directory):
    so = os.path.join(str(directory), "camera_keep_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "raytracer.glsl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "camera_keep_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.camera_keep_widening.restype = C.c_int
    lib.camera_keep_widening.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.camera_keep_decide.restype = None
    lib.camera_keep_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def shim_widening(lib, words):
    w = np.ascontiguousarray(words, np.uint32)
    ro, sigma = C.c_float(), C.c_float()
    ok = lib.camera_keep_widening(w.ctypes.data_as(C.c_void_p), C.byref(ro), C.byref(sigma))
    return bool(ok), np.float32(ro.value), np.float32(sigma.value)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("camera_keep"))


_rays = {}


def rays_of(oracle, cam, W, H):
    """(FRAMES, h, w, 6) float32, computed once per camera and size, never written to"""
    key = (cam.name, W, H)
    if key not in _rays:
        g = ck.sc.GlibcRand(3)
        base = ck.sc.params_c1().replace(**cam.fields)
        out = np.stack([ck.oracle_rays(oracle, base.replace(frames=k + 1, random=g.rand()), W, H) for k in range(FRAMES)])
        out.setflags(write=False)
        _rays[key] = out
    return _rays[key]


def largest_chords(rays):
    """(largest |o_k - o_j|, largest |d_k - d_j|, NaN rays, rays) over all pairs of frames and all pixels, in float64"""
    r = rays.reshape(rays.shape[0], -1, 6).astype(np.float64)
    nan = np.isnan(r).any(axis=2)
    mo = md = 0.0
    for j in range(r.shape[0]):
        for k in range(j + 1, r.shape[0]):
            ok = ~(nan[j] | nan[k])
            if ok.any():
                diff = r[k, ok] - r[j, ok]
                mo = max(mo, float(np.sqrt((diff[:, :3] ** 2).sum(axis=1)).max()))
                md = max(md, float(np.sqrt((diff[:, 3:] ** 2).sum(axis=1)).max()))
    return mo, md, int(nan.sum()), int(nan.size)


def refusal_reasons(fields):
    """why widening() may refuse a camera with depth of field on"""
    a, f = abs(np.float32(fields["camera_aperture"])), abs(np.float32(fields["camera_focal_length"]))
    pn = float(np.sqrt(sum(float(np.float32(x)) ** 2 for x in fields["camera_position"])))
    out = set()
    if not np.isfinite([a, f, pn]).all():
        out.add("non-finite")
    elif f >= 1.0e18 or pn >= 1.0e18:
        out.add("huge")
    else:
        if a >= np.float32(0.25) * f:
            out.add("aperture >= focal / 4")
        if float(f) - float(a) < 4.0 * 2.0 ** -21 * (pn + float(f)) * (1.0 + 1.0e-6):
            out.add("focal - aperture within 4 x 2^-21 (|pos| + focal): the jitter is a few ulps of the position")
    return out


EXPECT_REFUSED = {"limit_0.25", "limit_above", "limit_neg_aperture_above", "far_5e5_x"}


@pytest.mark.parametrize("cam", CAMERAS, ids=[c.name for c in CAMERAS])
def test_every_frames_rays_stay_inside_the_widening(cam, oracle, shim):
    ok, ro_add, sigma_add = shim_widening(shim, ck.camera_words(cam.fields))
    if not ok:
        assert cam.name in EXPECT_REFUSED or cam.name.startswith("far_drawn"), f"{cam.name} is refused"
        assert cam.fields["use_dof"] and refusal_reasons(cam.fields), f"{cam.name}: refused without a documented reason"
        assert ro_add == 0.0 and sigma_add == 0.0
        return
    for W, H in SIZES:
        rays = rays_of(oracle, cam, W, H)
        mo, md, n_nan, n = largest_chords(rays)
        print(f"{cam.name} {W}x{H}: origins {mo:.6g} of ro_add {float(ro_add):.6g}, directions {md:.6g} of sigma_add {float(sigma_add):.6g}, NaN rays {n_nan} of {n}")
        want_nan = FRAMES if (cam.name, W, H) == ("skew_zero_forward", 40, 24) else 0
        assert n_nan == want_nan, f"{cam.name} {W}x{H}: {n_nan} rays with a NaN, expected {want_nan}"
        if cam.family == "no_dof":
            assert all(rays[k].tobytes() == rays[0].tobytes() for k in range(1, FRAMES)), f"{cam.name} {W}x{H}: the rays change between frames without depth of field"
            assert ro_add == 0.0 and sigma_add == 0.0
            continue
        assert mo <= float(ro_add), f"{cam.name} {W}x{H}: origins of two frames {mo:.6g} apart, ro_add = {float(ro_add):.6g}"
        assert md <= float(sigma_add), f"{cam.name} {W}x{H}: directions of two frames {md:.6g} apart, sigma_add = {float(sigma_add):.6g}"
        if cam.family == "tame":
            assert md >= 0.7 * float(sigma_add), f"{cam.name} {W}x{H}: the largest chord {md:.6g} is under 0.7 of sigma_add = {float(sigma_add):.6g}"
    assert not cam.fields["use_dof"] or not refusal_reasons(cam.fields), f"{cam.name}: accepted although {refusal_reasons(cam.fields)}"
    assert cam.name not in EXPECT_REFUSED, f"{cam.name} is accepted (and its rays stay inside the widening)"


def test_families_are_all_there_and_most_cameras_are_accepted(shim):
    by_family = {f: [c for c in CAMERAS if c.family == f] for f in ck.FAMILIES}
    assert all(len(v) >= 5 for v in by_family.values())
    accepted = {f: sum(shim_widening(shim, ck.camera_words(c.fields))[0] for c in v) for f, v in by_family.items()}
    assert accepted["tame"] == len(by_family["tame"]) and accepted["tiny"] == len(by_family["tiny"]) and accepted["skew"] == len(by_family["skew"])
    assert accepted["far"] >= 8 and accepted["limit"] >= 6
    assert any(np.signbit(x) and x == 0.0 for c in CAMERAS for k in ("camera_position", "camera_up", "camera_forward", "camera_right") for x in c.fields[k])
    assert len({c.fields["camera_fov"] for c in CAMERAS}) >= 4
