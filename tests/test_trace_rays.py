"""rt_trace_rays (batched world.hit): the closest hit and hit record of many rays in one
launch, against a numpy restatement of the reference's hittable_list::hit
(hittable_list.h:25-39) over sphere::hit (sphere.h:30-57) and set_face_normal
(hittable.h:15-21).

Tolerance: fp64 -- bit-exact (t, p, normal, front face, id, material); fp32 -- the same
sphere for >= 99.9 % of rays and |t - t64| <= 1e-4 * max(1, t) where both agree.
The restatement is test infrastructure (it sits here, not in the product)."""
import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

SEED = 0x5EED


def _rays(n: int, seed: int = 1) -> np.ndarray:
    """Camera-like rays from around the reference camera and rays from inside the scene,
    unnormalised directions (as get_ray and the scatter functions produce), times in [0, 1)."""
    g = np.random.default_rng(seed)
    o = np.concatenate([np.array([13.0, 2.0, 3.0]) + g.normal(0, 0.3, (n // 2, 3)),
                        g.uniform([-11, 0.05, -11], [11, 2.5, 11], (n - n // 2, 3))])
    target = g.uniform([-11, -0.5, -11], [11, 1.5, 11], (n, 3))
    d = (target - o) * g.uniform(0.05, 2.0, (n, 1))
    t = g.uniform(0, 1, (n, 1))
    return np.concatenate([o, d, t], axis=1)


def world_hit_reference(S: np.ndarray, M: np.ndarray, rays: np.ndarray):
    """hittable_list::hit over the spheres in list order, fp64, the reference's operation
    order: -> (t, p, normal, front, id) with id = -1 for a miss."""
    n = len(rays)
    o, d, tm = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    best_t = np.full(n, np.inf)
    best = np.full(n, -1)
    a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]   # length_squared (vec3.h:46-48)
    for k in range(len(S)):
        c = S["center"][k]
        if S["moving"][k]:   # sphere.h:68-72: center1 + time * center_vec
            c = c[None, :] + tm[:, None] * S["center_vec"][k][None, :]
        else:
            c = np.broadcast_to(c, o.shape)
        oc = o - c
        half_b = oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1] + oc[:, 2] * d[:, 2]
        cc = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]) - S["radius"][k] * S["radius"][k]
        disc = half_b * half_b - a * cc
        ok = disc >= 0
        sq = np.sqrt(np.where(ok, disc, 0.0))
        r1 = (-half_b - sq) / a
        r2 = (-half_b + sq) / a
        in1 = (0.001 < r1) & (r1 < best_t)
        in2 = (0.001 < r2) & (r2 < best_t)
        root = np.where(in1, r1, r2)
        hit = ok & (in1 | in2)
        best_t = np.where(hit, root, best_t)
        best = np.where(hit, k, best)
    found = best >= 0
    t = np.where(found, best_t, 0.0)
    p = o + t[:, None] * d                                   # ray.at (ray.h:19-21)
    idx = np.maximum(best, 0)
    c = S["center"][idx] + np.where(S["moving"][idx][:, None] != 0, tm[:, None] * S["center_vec"][idx], 0.0)
    inv_r = 1.0 / S["radius"][idx]                             # vec3 / double = (1/t) * v (vec3.h:101-103)
    outward = inv_r[:, None] * (p - c)
    front = (d[:, 0] * outward[:, 0] + d[:, 1] * outward[:, 1] + d[:, 2] * outward[:, 2]) < 0
    normal = np.where(front[:, None], outward, -outward)
    return t, p, normal, front, best


@pytest.fixture(scope="module")
def random_world():
    rtweekend.reset_stream()
    return api.flatten(scenes.random_spheres())


# ---- negative radii (the reference's hollow spheres: sphere.h:35 squares the radius, :52
# divides the normal by it) ---------------------------------------------------------------
def neg_field(S: np.ndarray, ground: bool = False) -> np.ndarray:
    """NEG: the random field with the radius negated on indices 1::3 (and on the ground)."""
    S = S.copy()
    S["radius"][1::3] *= -1
    if ground:
        S["radius"][0] *= -1
    return S


def shell_field(S: np.ndarray, M: np.ndarray, inner: float = -0.8) -> np.ndarray:
    """SHELL: the random field plus, for every dielectric sphere, a concentric sphere of
    `inner` times its radius with the same material and the same motion (504 spheres)."""
    glass = S[M["type"][S["mat"]] == N.RT_DIELECTRIC].copy()
    glass["radius"] *= inner
    return np.concatenate([S, glass])


def hollow_world():
    """HOLLOW: scenes.hollow_glass(), the ten spheres of the reference-made golden."""
    return api.flatten(scenes.hollow_glass())


def negative_rays(S: np.ndarray, n: int = 20000, seed: int = 1) -> np.ndarray:
    """_rays(n) and n // 4 rays that start inside a negative-radius sphere (within half its
    radius of where its centre is at the ray's time), in every direction: the segments of a
    path inside a hollow sphere.  From outside, a shell within a sphere is never the closest
    hit, so _rays alone would leave the shells of SHELL and HOLLOW untested."""
    g = np.random.default_rng(seed + 1000)
    m = n // 4
    neg = np.flatnonzero(S["radius"] < 0)
    k = neg[g.integers(0, len(neg), m)]
    t = g.uniform(0, 1, (m, 1))
    c = S["center"][k] + np.where(S["moving"][k][:, None] != 0, t * S["center_vec"][k], 0.0)
    off = g.normal(size=(m, 3))
    off *= (0.5 * np.abs(S["radius"][k]) * g.uniform(0, 1, m) / np.linalg.norm(off, axis=1))[:, None]
    d = g.normal(size=(m, 3)) * g.uniform(0.05, 2.0, (m, 1))
    return np.concatenate([_rays(n, seed), np.concatenate([c + off, d, t], axis=1)])


_NEG_CASES = {}


def negative_case(name: str, random_world):
    """(S, M, rays, world_hit_reference of them), computed once per scene."""
    if name not in _NEG_CASES:
        S, M = random_world
        if name == "NEG":
            S = neg_field(S)
        elif name == "NEG_GROUND":
            S = neg_field(S, ground=True)
        elif name == "SHELL":
            S = shell_field(S, M)
        elif name == "HOLLOW":
            S, M = hollow_world()
        else:
            raise ValueError(name)
        rays = negative_rays(S)
        _NEG_CASES[name] = (S, M, rays, world_hit_reference(S, M, rays))
    return _NEG_CASES[name]


def test_reference_is_blind_to_the_radius_sign(random_world):
    """The numpy restatement itself (no GPU): on the field with radii negated it returns the
    plain field's ids, t and normals bit for bit, and front_face differs exactly on the hits
    of negated spheres."""
    S, M = random_world
    Sn = neg_field(S)
    rays = negative_rays(Sn, 4000)
    t0, p0, n0, f0, i0 = world_hit_reference(S, M, rays)
    t1, p1, n1, f1, i1 = world_hit_reference(Sn, M, rays)
    assert np.array_equal(i0, i1) and np.array_equal(t0, t1) and np.array_equal(p0, p1)
    hit = i0 >= 0
    assert np.array_equal(n0[hit], n1[hit])
    flipped = hit & (Sn["radius"][np.maximum(i0, 0)] < 0)
    assert flipped.mean() >= 0.05 and np.array_equal(f0 != f1, flipped)


@pytest.mark.gpu
@pytest.mark.parametrize("front", [None, 0, 16], ids=["front_default", "front0", "front16"])
@pytest.mark.parametrize("scene", ["NEG", "SHELL", "HOLLOW"])
def test_trace_rays_negative_radius_fp64_bit_exact(random_world, scene, front):
    """fp64 first hits on scenes with negative radii: id, t, p, normal, front face and
    material equal the list-order reference bit for bit, with the largest spheres in the
    front list (default), every sphere in the tree (0) and 16 in front of it."""
    S, M, rays, (t, p, nrm, ff, ids) = negative_case(scene, random_world)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
        if front is not None:
            r.set_tuning(front_spheres=front)
        r.upload_scene(S, M)
        h = r.trace_rays_host(rays)
    hit = ids >= 0
    on_negative = hit & (S["radius"][np.maximum(ids, 0)] < 0)
    print(scene, "rays hitting", hit.mean(), "hitting a negative-radius sphere", on_negative.mean())
    assert on_negative.mean() >= 0.05
    assert np.array_equal(h["id"], ids)
    assert np.array_equal(h["t"][hit], t[hit])
    assert np.array_equal(h["p"][hit], p[hit]) and np.array_equal(h["normal"][hit], nrm[hit])
    assert np.array_equal(h["front_face"][hit].astype(bool), ff[hit])
    assert np.array_equal(h["mat"][hit], S["mat"][ids[hit]])
    assert (h["t"][~hit] == 0).all() and (h["mat"][~hit] == 0).all()


@pytest.mark.gpu
def test_trace_rays_negative_radius_fp32_identity(random_world):
    """fp32 on NEG is an identity, not a tolerance: the root test sees the radius only as
    r * r and the tree's boxes only |r|, so id and t (and p) equal what the same build returns
    for the plain field bit for bit; (p - c) * rcp(r) flips with r exactly, so front_face
    differs exactly where the hit sphere was negated and the normal is unchanged."""
    S, M = random_world
    Sn, _, rays, (_, _, _, _, ids) = negative_case("NEG", random_world)
    out = []
    for arr in (S, Sn):
        with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
            r.upload_scene(arr, M)
            out.append(r.trace_rays_host(rays.astype(np.float32)))
    a, b = out
    assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["p"], b["p"])
    assert np.array_equal(a["mat"], b["mat"])
    hit = a["id"] >= 0
    flipped = hit & (Sn["radius"][np.maximum(a["id"], 0)] < 0)
    assert flipped.mean() >= 0.05 and (a["id"] == ids).mean() >= 0.999
    assert np.array_equal(a["front_face"] != b["front_face"], flipped)
    assert np.array_equal(a["normal"], b["normal"])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["SHELL", "HOLLOW", "NEG_GROUND"])
def test_trace_rays_negative_radius_fp32_within_tolerance(random_world, scene):
    """fp32 on the shells, the hollow scene and NEG with the ground negated as well (the
    big-sphere record with r = -1000) under this file's bounds: the same sphere for >= 99.9 %
    of rays, |t - t64| <= 1e-4 * max(1, t) and the reference's front face where both agree.
    (Measured on MI355X, max |t - t64| / max(1, t): SHELL 9.4e-6, HOLLOW 6.2e-6, NEG_GROUND
    4.7e-6 -- 1.8e-3 while the r = -1000 ground's fp32 record took centre + r n, its far
    point, for its near point; all ids and front faces the reference's.)"""
    S, M, rays, (t, _, _, ff, ids) = negative_case(scene, random_world)
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        h = r.trace_rays_host(rays.astype(np.float32))
    same = h["id"] == ids
    both = same & (ids >= 0)
    err = np.abs(h["t"][both] - t[both]) / np.maximum(1.0, t[both])
    print(scene, "same id", same.mean(), "max |t - t64| / max(1, t)", err.max(),
          "front face differs on", int((h["front_face"][both].astype(bool) != ff[both]).sum()))
    assert same.mean() >= 0.999, same.mean()
    assert np.all(err <= 1e-4)
    assert np.array_equal(h["front_face"][both].astype(bool), ff[both])


@pytest.mark.gpu
def test_trace_rays_radius_zero_sphere(random_world):
    """A sphere of radius 0 appended to the field: the upload succeeds in both precisions, no
    ray reports it, and every other result is unchanged -- fp64 the reference's bit for bit,
    fp32 the run without it."""
    S, M = random_world
    Z = np.concatenate([S, S[-1:]])
    Z[-1]["center"], Z[-1]["radius"], Z[-1]["moving"], Z[-1]["mat"] = (1.0, 0.2, 1.0), 0.0, 0, 0
    Z[-1]["center_vec"] = 0.0
    rays = _rays(20000)
    t, p, nrm, ff, ids = world_hit_reference(S, M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
        r.upload_scene(Z, M)
        h = r.trace_rays_host(rays)
    hit = ids >= 0
    assert (h["id"] != len(S)).all() and np.array_equal(h["id"], ids)
    assert np.array_equal(h["t"][hit], t[hit]) and np.array_equal(h["p"][hit], p[hit])
    assert np.array_equal(h["normal"][hit], nrm[hit])
    assert np.array_equal(h["front_face"][hit].astype(bool), ff[hit])
    assert np.array_equal(h["mat"][hit], S["mat"][ids[hit]])
    out = []
    for arr in (S, Z):
        with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
            r.upload_scene(arr, M)
            out.append(r.trace_rays_host(rays.astype(np.float32)))
    assert (out[1]["id"] != len(S)).all()
    for f in ("id", "t", "p", "normal", "front_face", "mat"):
        assert np.array_equal(out[0][f], out[1][f]), f


@pytest.mark.gpu
def test_trace_rays_fp64_bit_exact(random_world):
    S, M = random_world
    rays = _rays(20000)
    t, p, nrm, front, ids = world_hit_reference(S, M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
        r.upload_scene(S, M)
        h = r.trace_rays_host(rays)
    assert (ids >= 0).mean() > 0.5
    assert np.array_equal(h["id"], ids)
    hit = ids >= 0
    assert np.array_equal(h["t"][hit], t[hit])
    assert np.array_equal(h["p"][hit], p[hit]) and np.array_equal(h["normal"][hit], nrm[hit])
    assert np.array_equal(h["front_face"][hit].astype(bool), front[hit])
    assert np.array_equal(h["mat"][hit], S["mat"][ids[hit]])
    assert (h["t"][~hit] == 0).all() and (h["mat"][~hit] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("front", [0, 3])
def test_trace_rays_fp32_within_tolerance(random_world, front):
    S, M = random_world
    rays = _rays(20000, seed=2)
    t, _, _, _, ids = world_hit_reference(S, M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        r.set_tuning(front_spheres=front)
        r.upload_scene(S, M)
        h = r.trace_rays_host(rays.astype(np.float32))
    same = h["id"] == ids
    assert same.mean() >= 0.999, same.mean()
    both = same & (ids >= 0)
    assert np.all(np.abs(h["t"][both] - t[both]) <= 1e-4 * np.maximum(1.0, t[both]))


@pytest.mark.gpu
def test_trace_rays_triangle_ids_and_edge_cases():
    """Triangle ids map back to the caller's input order (host-built and GPU-built trees);
    an empty batch is a no-op; a ray that misses everything reports id -1."""
    S, M = api.flatten(scenes.ground_only())
    V = np.array([[0, 1, 0], [1, 1, 0], [0, 2, 0], [3, 1, 0], [4, 1, 0], [3, 2, 0]], dtype=np.float64)
    F = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    M2 = np.concatenate([M, M[:1]])
    T = N.triangles(V, F, len(M))
    cent = V[F].mean(axis=1)
    rays = np.concatenate([cent + [0, 0, 5], np.tile([0, 0, -1.0], (2, 1)), np.zeros((2, 1))], axis=1)
    rays = np.concatenate([rays, [[0, 5, 0, 0, 1, 0, 0.5]]])      # straight up: the sky
    for builder in (N.RT_MESH_BUILD_HOST, N.RT_MESH_BUILD_GPU, N.RT_MESH_BUILD_GPU_LBVH):
        for prec in (N.RT_PREC_F64, N.RT_PREC_F32):
            with N.Renderer(0, SEED, prec) as r:
                r.set_tuning(mesh_builder=builder)
                r.upload_scene(S, M2, T)
                h = r.trace_rays_host(rays)
                assert h["id"].tolist() == [len(S) + 0, len(S) + 1, -1], (builder, prec)
                assert np.allclose(h["t"][:2], 5.0) and (h["mat"][:2] == len(M)).all()
                r.trace_rays(0, 0, 0)   # nothing to do


@pytest.mark.gpu
def test_trace_rays_axis_aligned_fp32(random_world):
    """Directions with exact-zero components (axis-aligned rays): the fp32 slab test must
    not turn them into misses (1/0 = inf made lo * inf - o * inf a NaN slab before r03)."""
    S, M = random_world
    g = np.random.default_rng(3)
    o = g.uniform([-11, 0.3, -11], [11, 2, 11], (4000, 3))
    axes = np.eye(3)[g.integers(0, 3, 4000)] * g.choice([-1, 1], (4000, 1))
    rays = np.concatenate([o, axes, g.uniform(0, 1, (4000, 1))], axis=1)
    _, _, _, _, ids = world_hit_reference(S, M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        h = r.trace_rays_host(rays.astype(np.float32))
    assert (ids >= 0).sum() > 500
    assert (h["id"] == ids).mean() >= 0.999


@pytest.mark.gpu
def test_trace_rays_fp64_conservative_boxes(random_world):
    """The fp64 path tests boxes in fp32 with widened slabs (TRAV_F32BOX): rays whose
    slabs are hardest to bound -- exact-zero and tiny direction components, origins far
    out on the ground (|o| up to ~900), origins on sphere surfaces, grazing rays along a
    box face -- still find exactly the list-order reference's closest hit."""
    S, M = random_world
    g = np.random.default_rng(11)
    n = 6000
    o = g.uniform([-11, 0.3, -11], [11, 2, 11], (n, 3))
    d = g.normal(size=(n, 3))
    k = g.integers(0, 3, n)
    d[np.arange(n), k] = g.choice([0.0, 1e-35, -1e-35, 1e-20, 1e-12, 1e-7], n)   # (near-)axis-parallel
    far = np.concatenate([g.uniform(-900, 900, (n, 1)), np.full((n, 1), 0.05), g.uniform(-900, 900, (n, 1))], axis=1)
    d_far = g.uniform([-11, 0, -11], [11, 1.5, 11], (n, 3)) - far
    rays = np.concatenate([np.concatenate([o, d, g.uniform(0, 1, (n, 1))], axis=1),
                           np.concatenate([far, d_far, g.uniform(0, 1, (n, 1))], axis=1)])
    # origins on the spheres hit by the first batch, scattered in random directions
    t0, p0, nrm0, _, ids0 = world_hit_reference(S, M, rays)
    hit = ids0 >= 0
    sec = np.concatenate([p0[hit], nrm0[hit] + g.normal(size=(hit.sum(), 3)), rays[hit, 6:7]], axis=1)
    # grazing: origins on a sphere's bounding-box face plane, moving along it
    c = S["center"][g.integers(0, len(S), n)]
    r = np.abs(S["radius"][g.integers(0, len(S), n)])
    graze_o = c + np.array([1.0, 0, 0]) * r[:, None] + np.array([0, 0, -3.0])
    graze = np.concatenate([graze_o, np.tile([0, 0, 1.0], (n, 1)), np.zeros((n, 1))], axis=1)
    rays = np.concatenate([rays, sec, graze])
    t, p, nrm, front, ids = world_hit_reference(S, M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as rr:
        rr.upload_scene(S, M)
        h = rr.trace_rays_host(rays)
    assert (ids >= 0).sum() > 5000
    assert np.array_equal(h["id"], ids)
    m = ids >= 0
    assert np.array_equal(h["t"][m], t[m]) and np.array_equal(h["p"][m], p[m])


@pytest.mark.gpu
def test_trace_rays_gpu_trees_report_input_triangles():
    """r06: the treelet-restructured GPU tree stores its triangles in depth-first leaf order,
    not Morton order; rt_trace_rays still reports each hit as the input triangle index -- fp64
    hits through the host tree and both GPU trees are identical, ids and distances, over the
    config-4 blob and ground."""
    from test_mesh import mesh_arrays
    S, M, T = mesh_arrays("mesh")
    g = np.random.default_rng(11)
    n = 4096
    o = g.uniform([-3, 0.2, -3], [3, 3, 3], (n, 3))
    tgt = g.uniform([-1.2, 0.0, -1.2], [1.2, 2.2, 1.2], (n, 3))
    rays = np.concatenate([o, tgt - o, g.uniform(0, 1, (n, 1))], axis=1)
    out = []
    for builder in (N.RT_MESH_BUILD_HOST, N.RT_MESH_BUILD_GPU, N.RT_MESH_BUILD_GPU_LBVH):
        with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
            r.set_tuning(mesh_builder=builder)
            r.upload_scene(S, M, T)
            out.append(r.trace_rays_host(rays))
    assert (out[0]["id"] >= len(S)).mean() > 0.5   # mostly triangles
    for h in out[1:]:
        assert np.array_equal(h["id"], out[0]["id"])
        assert np.array_equal(h["t"], out[0]["t"])
