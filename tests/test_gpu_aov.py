"""First-hit planes (option "aov": albedo, normal, position, hit ids; include/rtgl_amd.h) on the device.

The reference for the planes is the CPU oracle, read only: oracle_set_ray_dump records the ray that enters a bounce, so the dump of
bounce 0 is the camera ray (o, d) and the dump of bounce 1 starts at the exact first-hit point p.  The image itself must not change: with
every plane on, each golden case stays bit-identical to the reference shader's output on kernels 0, 1, 2 and 4."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_cases as gc
import raytracer_glsl_amd
from mesh_fuzz_inputs import spans as mesh_spans
from test_oracle_golden import CASE_FILES, load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host
ALBEDO, NORMAL, POSITION, IDS, ALL = H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS, H_.AOV_ALL
PLANES = (ALBEDO, NORMAL, POSITION, IDS)
FLOAT_PLANES = (ALBEDO, NORMAL, POSITION)
ERR_INVALID, ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as the suite's earlier modules do): started the other
    way round, torch found no device on the test machines (test_errors_restarts_and_device_pointer shares a plane with a tensor)"""
    import torch
    torch.cuda.init()


def render(rt, W, H, scene, frames, options=(), aov=ALL, init=None, rng=False, **kw):
    ctx = rt.host.Context(W, H, **kw)
    for k, v in options:
        ctx.set_option(k, v)
    if rng:
        ctx.set_option("rng_state", 1)
    if aov:
        ctx.set_aov(aov)
    ctx.upload_scene(scene)
    if init is not None:
        ctx.write_image(init)
    for p in frames:
        ctx.render(p)
    out = dict(img=ctx.read_image(), seeds=ctx.read_rng_state() if rng else None,
               planes={p: ctx.read_aov(p) for p in PLANES if aov & p}, rows=ctx.global_rows())
    ctx.close()
    return out


def named_case(rt, name):
    case = gc.build_cases(rt.scenes)[name]
    return case, case["scene"](), case["width"], case["height"]


# ---------------------------------------------------------------------------------------------- 1. the image does not change

@pytest.mark.parametrize("path", CASE_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_image_unchanged_and_planes_agree_across_kernels(path, rt):
    """every golden case with every plane on: the image bit-identical to the reference shader's, the final RNG states those of a run
    without the planes, on kernels 0, 1, 2 and 4 -- and the planes bit-identical across the four."""
    meta, scene, frames, expected = load_case(path, rt)
    W, H = meta["width"], meta["height"]
    init = gc.initial_image(meta["init"], W, H)
    first = None
    for kernel in (0, 1, 2, 4):
        on = render(rt, W, H, scene, frames, options=(("kernel", kernel),), init=init, rng=True)
        off = render(rt, W, H, scene, frames, options=(("kernel", kernel),), aov=0, init=init, rng=True)
        assert same(on["img"], expected), f"kernel {kernel}: the image changed with the planes on"
        fh, fw = H // 8 * 8, W // 8 * 8                  # (outside the dispatch footprint the RNG buffer is never written)
        assert (on["seeds"][:fh, :fw] == off["seeds"][:fh, :fw]).all(), f"kernel {kernel}: the RNG states changed with the planes on"
        if first is None:
            first = on["planes"]
        for p in PLANES:
            assert same(on["planes"][p], first[p]), f"kernel {kernel}: plane {p} differs from kernel 0's"


# ---------------------------------------------------------------------------------------------- 2-4. against the oracle's rays

def oracle_dump(oracle, scene, p, W, H, bounce):
    """(H, W, 6) o.xyz d.xyz of the ray that enters `bounce`, NaN where the path ended before"""
    buf = np.full((H * W, 6), np.nan, np.float32)
    oracle.lib.oracle_set_ray_dump(buf.ctypes.data_as(C.c_void_p), C.c_uint32(bounce))
    try:
        oracle.render(scene, p.replace(max_bounce=bounce + 1), np.zeros((H, W, 4), np.float32), threads=8)
    finally:
        oracle.lib.oracle_set_ray_dump(None, C.c_uint32(0))
    return buf.reshape(H, W, 6)


def triangle_material(w):
    """TriPlane.material: int(vertices[3v].w), -1 where the float is not representable"""
    w = np.asarray(w, np.float32)
    ok = (w > np.float32(-2147483648.0)) & (w < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, w, 0)).astype(np.int64), -1).astype(np.int32)


GEOMETRY_CASES = ["c1_light_8f", "glass_inside_tir", "spheres_two_level_tree", "spheres_deep_chain", "mesh_degenerate_inputs", "mesh_backfacing",
                  "mesh_two_meshes_overlap", "mesh_odd_materials", "mesh_env_dof", "env_noise_cube", "env_incomplete_cube", "env_disabled_background"]


@pytest.mark.parametrize("name", GEOMETRY_CASES)
def test_planes_match_the_oracles_first_hit(name, rt, oracle):
    case, scene, W, H = named_case(rt, name)
    p = case["frames"][0].replace(reset_flag=1, samples=1, max_bounce=2)
    got = render(rt, W, H, scene, [p])["planes"]
    fw, fh = W // 8 * 8, H // 8 * 8
    alb, nrm, pos, ids = (got[k][:fh, :fw] for k in PLANES)
    d0 = oracle_dump(oracle, scene, p, W, H, 0)[:fh, :fw]
    d1 = oracle_dump(oracle, scene, p, W, H, 1)[:fh, :fw]
    assert not np.isnan(d0).any()
    o, d = d0[..., :3], d0[..., 3:]
    kind, obj, prim, mat = ids[..., 0], ids[..., 1], ids[..., 2], ids[..., 3]
    assert np.isin(kind, (0, 1, 2)).all()
    hit, miss = kind != 0, kind == 0
    assert hit.any()
    traced = ~np.isnan(d1[..., 0])

    # 2. position: exactly the origin of the next ray; o + d t in float32; misses start no next ray; a hit that starts none is a
    #    transmissive material (total internal reflection at bounce 0)
    assert not (traced & miss).any()
    assert same(pos[traced][:, :3], d1[traced][:, :3])
    t = pos[..., 3]
    recon = o + d * t[..., None]
    assert same(recon[hit], pos[hit][:, :3])
    mats = np.asarray(scene.materials, np.float32).reshape(-1, 8)
    nm = mats.shape[0]
    in_range = (mat >= 0) & (mat < nm)
    mtype = np.where(in_range, mats[:, 7].view(np.uint32)[np.clip(mat, 0, max(nm - 1, 0))] if nm else 0, 0)
    assert (mtype[hit & ~traced] == 2).all(), "a hit that ends its path at bounce 0 must be total internal reflection in glass"

    # 3. ids and normals agree with the geometry
    sph, tri = kind == 1, kind == 2
    spheres = np.asarray(scene.spheres, np.float32).reshape(-1, 8)
    if sph.any():
        assert (obj[sph] == prim[sph]).all()
        s_ok = sph & (obj >= 0)
        assert (obj[s_ok] < spheres.shape[0]).all()
        rec = spheres[obj[s_ok]]
        want = (pos[s_ok][:, :3] - rec[:, :3]) / rec[:, 3:4]
        assert same(nrm[s_ok][:, :3], want)
        assert (mat[s_ok] == rec[:, 4].view(np.int32)).all()
    if tri.any():
        V = np.asarray(scene.vertices, np.float32).reshape(-1, 4)
        assert (prim[tri] >= 0).all() and (3 * prim[tri] + 2 < V.shape[0]).all()
        v = np.stack([V[3 * prim[tri] + k, :3] for k in range(3)], axis=1).astype(np.float64)      # (n, 3 vertices, xyz)
        assert (mat[tri] == triangle_material(V[3 * prim[tri], 3])).all()
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        n = np.cross(e1, e2)
        fine = np.isfinite(v).all(axis=(1, 2)) & (np.abs(v).max(axis=(1, 2)) < 1e6) & (np.linalg.norm(n, axis=1) > 1e-12)
        assert fine.any()
        n = n[fine] / np.linalg.norm(n[fine], axis=1, keepdims=True)
        assert np.abs(nrm[tri][fine][:, :3] - n).max() <= 1e-6
        P = pos[tri][fine][:, :3].astype(np.float64)
        rel = P - v[fine, 0]
        scale = 1.0 + np.abs(v[fine]).max(axis=(1, 2))
        assert (np.abs((rel * n).sum(axis=1)) <= 1e-4 * scale).all(), "hit point off the named triangle's plane"
        a, b = e1[fine], e2[fine]                        # rel = u a + v b: the normal equations
        M = np.empty((a.shape[0], 2, 2))
        M[:, 0, 0], M[:, 0, 1], M[:, 1, 1] = (a * a).sum(1), (a * b).sum(1), (b * b).sum(1)
        M[:, 1, 0] = M[:, 0, 1]
        uv = np.linalg.solve(M, np.stack([(rel * a).sum(1), (rel * b).sum(1)], axis=-1)[..., None])[..., 0]
        assert (uv > -1e-4).all() and (uv.sum(axis=1) < 1 + 1e-4).all(), "hit point outside the named triangle"
        # the mesh: the first one that lists the triangle (hits merge by visit index, and a mesh's visits come before the next one's)
        n_tris = V.shape[0] // 3
        first_mesh = np.full(n_tris, -1, np.int64)
        for m, a, b in reversed(mesh_spans(scene.meshes, n_tris)):      # the shader's 32-bit loop bounds (tests/mesh_fuzz_inputs.py)
            first_mesh[a:b] = m
        assert (obj[tri] == first_mesh[prim[tri]]).all()
        if name == "mesh_two_meshes_overlap":
            assert (obj[tri] == 1).any(), "the second mesh's own triangles are never reported"

    # 4. albedo: the material's on a hit, what the camera ray received on a miss
    mat_alb = np.where(in_range[..., None], mats[np.clip(mat, 0, max(nm - 1, 0)), :3] if nm else 0, 0).astype(np.float32)
    assert same(alb[hit][:, :3], mat_alb[hit]) and (alb[hit][:, 3] == 1).all()
    if miss.any():
        if p.use_envmap and scene.env is not None:
            bg = oracle.env_lookup(scene, d[miss])
        else:
            bg = np.broadcast_to(np.asarray(p.background, np.float32), (int(miss.sum()), 3))
        assert same(alb[miss][:, :3], bg) and (alb[miss][:, 3] == 0).all()
        assert (nrm[miss] == 0).all() and (pos[miss] == 0).all()
        assert (ids[miss] == np.array([0, -1, -1, -1], np.int32)).all()
    assert (nrm[..., 3] == 0).all()
    if name in ("env_noise_cube", "env_incomplete_cube", "env_disabled_background"):
        assert miss.any()


# ---------------------------------------------------------------------------------------------- 5. accumulation

@pytest.mark.parametrize("name", ["mesh_env_dof", "dof_wide_c5"])
def test_planes_accumulate_as_the_documented_running_mean(name, rt):
    """K frames with depth of field (the first hits move) and a reset frame in the middle, against a float32 replay of
    v = (x + prev (n - 1)) / n from the per-frame planes x_k of a second context that renders every frame alone as a reset frame."""
    case, scene, W, H = named_case(rt, name)
    frames = gc.frame_sequence(rt.scenes, case["frames"][0].replace(reset_flag=0), 6, seed=3, reset_at=(4,))
    assert frames[3].reset_flag == 1 and frames[0].use_dof
    acc, one = rt.host.Context(W, H), rt.host.Context(W, H)
    for c in (acc, one):
        c.set_aov(ALL)
        c.upload_scene(scene)
    prev, n = None, 0
    xs = []
    for k, p in enumerate(frames):
        one.render(p.replace(reset_flag=1))
        x = {pl: one.read_aov(pl) for pl in PLANES}
        xs.append(x)
        acc.render(p)
        n = 1 if (k == 0 or p.reset_flag) else n + 1
        want = {}
        for pl in FLOAT_PLANES:
            want[pl] = x[pl].copy() if n == 1 else (x[pl] + prev[pl] * np.float32(n - 1)) / np.float32(n)
            assert same(acc.read_aov(pl), want[pl]), f"frame {k} (n = {n}): plane {pl} is not the running mean"
        assert (acc.read_aov(IDS) == x[IDS]).all(), f"frame {k}: the ids are not the last frame's"
        prev = want
    acc.close(); one.close()
    assert not same(xs[0][POSITION], xs[1][POSITION]), "the first hits did not move between frames: the test has no teeth"


@pytest.mark.parametrize("kernel", [0, 1, 4])
def test_several_samples_write_the_planes_once(kernel, rt):
    case, scene, W, H = named_case(rt, "mesh_three_samples")
    frames = case["frames"]
    assert frames[0].samples == 3
    three = render(rt, W, H, scene, frames, options=(("kernel", kernel),))["planes"]
    one = render(rt, W, H, scene, [p.replace(samples=1) for p in frames], options=(("kernel", kernel),))["planes"]
    for p in PLANES:
        assert same(three[p], one[p])


def test_zero_bounces_give_miss_values_with_albedo_zero(rt):
    case, scene, W, H = named_case(rt, "zero_bounces_three_samples")
    got = render(rt, W, H, scene, case["frames"], init=gc.initial_image(case["init"], W, H))["planes"]
    fw, fh = W // 8 * 8, H // 8 * 8
    for p in FLOAT_PLANES:
        assert (got[p] == 0).all()
    assert (got[IDS][:fh, :fw] == np.array([0, -1, -1, -1], np.int32)).all()


# ---------------------------------------------------------------------------------------------- 6. every variant agrees

VARIANTS = [(("kernel", 0),), (("kernel", 1),), (("kernel", 1), ("wf_mode", 0), ("wf_rays", 1)), (("kernel", 2),),
            (("kernel", 4), ("cull", 0)), (("kernel", 4), ("cull", 1)), (("kernel", 4), ("cull", 2)),
            (("kernel", 4), ("cull", 3), ("sort_min_rays", 0)), (("kernel", 4), ("scan_waves", 1)), (("kernel", 4), ("scan_waves", 2)),
            (("kernel", 4), ("frame_batch", 8)), (("kernel", 4), ("counters", 1)), (("kernel", 2), ("counters", 1)), (("kernel", 0), ("counters", 1))]


@pytest.mark.parametrize("name", ["mesh_env_dof", "mesh_two_meshes_overlap", "mesh_stacked_duplicates", "c1_light_8f"])
def test_planes_identical_across_variants(name, rt):
    case, scene, W, H = named_case(rt, name)
    frames = case["frames"][:3]
    ref = render(rt, W, H, scene, frames, options=VARIANTS[0])
    for opts in VARIANTS[1:]:
        got = render(rt, W, H, scene, frames, options=opts)
        assert same(got["img"], ref["img"]), opts
        for p in PLANES:
            assert same(got["planes"][p], ref["planes"][p]), f"{opts}: plane {p} differs from kernel 0's"


# ---------------------------------------------------------------------------------------------- 7. layout

def test_tiled_and_multi_device_planes_hold_the_right_rows(rt):
    case, scene, W, H = named_case(rt, "dof_wide_c5")
    frames = case["frames"]
    full = render(rt, W, H, scene, frames)["planes"]
    for rank in (0, 1):
        part = render(rt, W, H, scene, frames, rank=rank, world=2, strip_rows=16)
        assert len(part["rows"]) < H
        for p in PLANES:
            assert same(part["planes"][p], full[p][part["rows"]]), f"rank {rank}: plane {p}"
    multi = render(rt, W, H, scene, frames, devices=[0, 0], strip_rows=8)
    for p in PLANES:
        assert same(multi["planes"][p], full[p]), f"multi-device handle: plane {p}"
    ctx = rt.host.Context(W, H, devices=[0, 0], strip_rows=8)
    ctx.set_aov(ALL)
    assert ctx.device_aov_ptr(ALBEDO) == 0 and ctx.lib.rtgl_last_error(ctx.h)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 8. errors, restarts, sharing

class _DeviceArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def test_errors_restarts_and_device_pointer(rt):
    import torch
    sc = rt.scenes
    W, H = 64, 64
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 4)
    lib = rt.host.load_library()
    ctx = rt.host.Context(W, H)
    ctx.upload_scene(scene)
    buf = np.zeros((H, W, 4), np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.rtgl_read_aov(ctx.h, ALBEDO, ptr) == ERR_STATE          # off by default
    ctx.set_aov(ALBEDO | IDS)
    assert ctx.get_option("aov") == ALBEDO | IDS
    ctx.render(frames[0])
    assert lib.rtgl_read_aov(ctx.h, NORMAL, ptr) == ERR_STATE
    for bad in (0, 3, 16, -1):
        assert lib.rtgl_read_aov(ctx.h, bad, ptr) == ERR_INVALID
    assert lib.rtgl_read_aov(ctx.h, ALBEDO, None) == ERR_INVALID
    assert ctx.device_aov_ptr(NORMAL) == 0
    for bad in (16, -1):
        with pytest.raises(rt.host.RtglError):
            ctx.set_aov(bad)
    assert (ctx.read_aov(ALBEDO)[..., 3] == 1).any()

    # off and on again: zeroed, and the next frame starts the mean afresh (n = 1 without a reset flag)
    ctx.set_aov(0)
    assert lib.rtgl_read_aov(ctx.h, ALBEDO, ptr) == ERR_STATE
    ctx.set_aov(ALL)
    for p in PLANES:
        assert (ctx.read_aov(p) == 0).all()
    alone = render(rt, W, H, scene, [frames[1].replace(reset_flag=1)])["planes"]
    ctx.render(frames[1])
    for p in PLANES:
        assert same(ctx.read_aov(p), alone[p])
    # rtgl_write_image_f32 leaves the planes alone; rtgl_clear_image restarts the mean
    before = {p: ctx.read_aov(p) for p in PLANES}
    ctx.write_image(np.full((H, W, 4), 0.5, np.float32))
    for p in PLANES:
        assert same(ctx.read_aov(p), before[p])
    ctx.render(frames[2])
    assert not same(ctx.read_aov(POSITION), render(rt, W, H, scene, [frames[2].replace(reset_flag=1)])["planes"][POSITION])
    ctx.clear_image()
    ctx.render(frames[3])
    alone = render(rt, W, H, scene, [frames[3].replace(reset_flag=1)])["planes"]
    for p in PLANES:
        assert same(ctx.read_aov(p), alone[p])

    # torch interop: a tensor on the device pointer reads what rtgl_read_aov copies
    for p, typestr, dtype in ((ALBEDO, "<f4", np.float32), (POSITION, "<f4", np.float32), (IDS, "<i4", np.int32)):
        dptr = ctx.device_aov_ptr(p)
        assert dptr
        t = torch.as_tensor(_DeviceArray(dptr, (H, W, 4), typestr), device="cuda:0")
        torch.cuda.synchronize()
        assert same(t.cpu().numpy().astype(dtype), ctx.read_aov(p))
    ctx.close()

    # the headless renderer passes the mask through
    hr = rt.host.HeadlessRenderer(W, H, aov=NORMAL)
    hr.set_scene(scene)
    hr.params = sc.params_c2()
    hr.run(2)
    assert hr.ctx.get_option("aov") == NORMAL and hr.read_aov(NORMAL).shape == (H, W, 4)
    hr.ctx.close()
