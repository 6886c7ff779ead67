"""The life of a context's device memory, on the GPU: scenes replaced in one context, uploads that
fail before and after the old scene is freed, scratch that grows and is reused, and contexts
created and destroyed one after another.  Every check is bit equality with a fresh context that
was given only the scene in question (or with the same context's first call at the same size);
nothing here reads memory figures -- the device is shared.

Scenes: four_spheres; the random field (fp32: a sphere grid); the field plus meshgen.blob(0)
built on the device (rt_tuning.mesh_builder = RT_MESH_BUILD_GPU), as tests/test_pack.py's
_blob(True).  Camera: main.cpp's, 48 pixels wide; 2 spp, depth 8."""
import ctypes as C
import functools

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, meshgen, rtweekend, scenes

pytestmark = pytest.mark.gpu

SPP, DEPTH, WIDTH = 2, 8, 48
PRECS = [pytest.param(N.RT_PREC_F32, id="f32"), pytest.param(N.RT_PREC_F64, id="f64")]
# Case 3: the random field tiled TILES times along x is the smallest tiling (1..64 tried in turn)
# whose fp64 upload the parent of this change refuses after it has freed the old scene, with
# RT_ERR_LIMIT and "scene needs TILES_LDS_BYTES B of LDS per workgroup (> 160 KiB)".
TILES, TILES_LDS_BYTES = 4, 193488
TILE_PITCH = 30.0   # (the field spans x in [-11, 11])


def _cam(width=WIDTH):
    cam = scenes.main_camera()
    cam.image_width = width
    return cam.native


def _field():
    rtweekend.reset_stream()
    return api.flatten(scenes.random_spheres())


def _tiled(k):
    S, M = _field()
    T = np.concatenate([S] * k)
    T["center"][:, 0] += np.repeat(np.arange(k) * TILE_PITCH, len(S))
    return T, M


def _scene(name):
    """(spheres, materials, triangles or None, tuning the upload needs)"""
    if name == "four":
        return (*api.flatten(scenes.four_spheres()), None, {})
    if name == "field":
        return (*_field(), None, {})
    if name == "mesh":   # (tests/test_pack.py's _blob(False): no sphere, so no sphere grid)
        V, F = meshgen.blob(0, radius=meshgen.MESH_RADIUS, center=meshgen.MESH_CENTER)
        M = np.zeros(1, dtype=N.MATERIAL_DTYPE)
        M[0]["type"], M[0]["albedo"] = N.RT_METAL, (0.7, 0.6, 0.5)
        return np.zeros(0, dtype=N.SPHERE_DTYPE), M, N.triangles(V, F, 0), {}
    assert name == "mixed"
    V, F = meshgen.blob(0, radius=meshgen.MESH_RADIUS, center=meshgen.MESH_CENTER)
    return (*_field(), N.triangles(V, F, 3), dict(mesh_builder=N.RT_MESH_BUILD_GPU))


def _upload(r, name):
    S, M, T, tune = _scene(name)
    r.set_tuning(**tune)
    r.upload_scene(S, M, T)
    r.set_tuning(mesh_builder=N.RT_MESH_BUILD_HOST)


def _rays(n=256):
    """Fixed rays from around main.cpp's camera into the field (origin, direction, time)."""
    g = np.random.default_rng(20260)
    o = np.array((13.0, 2.0, 3.0)) + g.uniform(-1.0, 1.0, (n, 3))
    d = g.uniform((-6.0, 0.0, -6.0), (6.0, 1.5, 6.0), (n, 3)) - o
    return np.concatenate([o, d, g.uniform(0.0, 1.0, (n, 1))], axis=1)


def _info(r):
    i = r.scene_info()
    return {n: (list(v) if hasattr(v, "__len__") else v) for n, _ in i._fields_ for v in [getattr(i, n)]}


def _jobs(n, cam):
    j = np.zeros(n, N.RtPixelJob)
    j["pixel"] = (np.arange(n) * 37) % (cam.image_width * cam.image_height)
    j["sample_count"] = SPP
    return j


def _moments(r, cam, jobs):
    import torch
    n = len(jobs)
    tdt = torch.from_numpy(np.zeros(0, r.dtype)).dtype
    d_j = torch.from_numpy(jobs.view(np.uint8)).to("cuda")
    d_s, d_q = (torch.full((n, 3), float("nan"), dtype=tdt, device="cuda") for _ in range(2))
    d_g = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.render_pixels_moments(cam, d_j.data_ptr(), n, DEPTH, d_s.data_ptr(), d_q.data_ptr(), d_g.data_ptr())
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_q.cpu().numpy(), d_g.cpu().numpy()


def _bits(x):
    """What a call returned, as bytes per array (hit records: per field, their padding aside)."""
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_bits(v) for v in x]
    if isinstance(x, np.ndarray) and x.dtype == N.HIT_DTYPE:
        return {f: x[f].tobytes() for f in x.dtype.names if f != "pad"}
    return np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x


def _observe(r):
    """Everything case 1 compares: the frame (sums, rgb, segments), scene_info, 256 traced rays."""
    return _bits(dict(frame=r.render_frame(_cam(), SPP, DEPTH), info=_info(r), hits=r.trace_rays_host(_rays())))


@functools.lru_cache(maxsize=None)
def _fresh(prec, name):
    """What a fresh context that was given only this scene shows (computed once per process)."""
    with N.Renderer(0, 0x5EED, prec) as r:
        _upload(r, name)
        return _observe(r)


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differs" + (f": {got[k]} != {want[k]}" if k == "info" else "")


@pytest.mark.parametrize("prec", PRECS)
def test_scene_replacement(prec):
    """Case 1: field, mixed (device-built mesh: the builder's scratch and the id-map read-back run),
    four_spheres in one context; after each nothing of the earlier scenes shows.  After four_spheres
    no triangle and no mesh node is left, and the grid is four_spheres' own (5 x 1 x 1 cells: that
    scene has one too), not the field's; a mesh without spheres, uploaded last, leaves no grid."""
    with N.Renderer(0, 0x5EED, prec) as r:
        for name in ("field", "mixed", "four"):
            _upload(r, name)
            _same(_observe(r), _fresh(prec, name), name)
        info = _info(r)
        _upload(r, "mesh")
        _same(_observe(r), _fresh(prec, "mesh"), "mesh")
        last = _info(r)
    frames = [_fresh(prec, name)["frame"] for name in ("field", "mixed", "four", "mesh")]
    assert all(a != b for k, a in enumerate(frames) for b in frames[:k])   # (four scenes, four frames)
    field, mixed = _fresh(prec, "field")["info"], _fresh(prec, "mixed")["info"]
    assert mixed["num_spheres"] > 0 and mixed["num_triangles"] == 20 and mixed["mesh_nodes"] > 0
    assert all(v > 0 for v in field["grid_res"]) and field["grid_res"] != info["grid_res"]
    assert (info["num_triangles"], info["mesh_nodes"], info["mesh_depth"], info["mesh_leaves"]) == (0, 0, 0, 0)
    assert (last["num_spheres"], last["bvh_leaves"], last["grid_res"], last["grid_entries"]) == (0, 0, [0, 0, 0], 0), last


@pytest.mark.parametrize("prec", PRECS)
def test_upload_refused_before_the_free_keeps_the_scene(prec):
    """Case 2: a sphere naming a material out of range is found by the packing, before anything
    is freed: RT_ERR_INVALID, and the old scene renders the same bits."""
    S, M, _, _ = _scene("four")
    bad = S.copy()
    bad["mat"][1] = len(M)
    with N.Renderer(0, 0x5EED, prec) as r:
        _upload(r, "four")
        rc = r._L.rt_upload_scene(r.ctx, N._ptr(bad), len(bad), N._ptr(M), len(M))
        assert rc == N.RT_ERR_INVALID and b"references material" in r._L.rt_last_error(r.ctx)
        _same(_observe(r), _fresh(prec, "four"), "four after a refused upload")


def test_upload_refused_after_the_free_leaves_no_scene():
    """Case 3 (fp64): TILES tiles of the field pack, and need more LDS than a workgroup has: the
    old scene is gone by then.  No scene, for rendering and for scene_info; then four_spheres as in
    a fresh context."""
    S, M = _tiled(TILES)
    cam = _cam()
    with N.Renderer(0, 0x5EED, N.RT_PREC_F64) as r:
        _upload(r, "four")
        rc = r._L.rt_upload_scene(r.ctx, N._ptr(S), len(S), N._ptr(M), len(M))
        msg = r._L.rt_last_error(r.ctx).decode()
        print(f"tiles {TILES}: status {rc}, {msg}")
        assert rc == N.RT_ERR_LIMIT and f"scene needs {TILES_LDS_BYTES} B of LDS per workgroup" in msg
        sums = np.empty((cam.image_height, cam.image_width, 3), np.float64)
        assert r._L.rt_render_frame(r.ctx, C.byref(cam), SPP, DEPTH, N._ptr(sums), None, None) == N.RT_ERR_NO_SCENE
        assert r._L.rt_scene_info_get(r.ctx, C.byref(N.RtSceneInfo())) == N.RT_ERR_NO_SCENE
        _upload(r, "four")
        _same(_observe(r), _fresh(N.RT_PREC_F64, "four"), "four after a failed upload")


def _sized_calls(r):
    """Every call of case 4 at (small, large, small): name -> the three results."""
    out = {"render_frame": [_bits(r.render_frame(_cam(w), SPP, DEPTH)) for w in (48, 96, 48)]}
    cam = _cam()
    for name, call in (("render_pixels", lambda j: r.render_pixels_host(cam, j, DEPTH, segments=True)),
                       ("moments", lambda j: _moments(r, cam, j)),
                       ("aov", lambda j: r.render_pixels_aov_host(cam, j))):
        out[name] = [_bits(call(_jobs(n, cam))) for n in (10, 500, 10)]
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_scratch_grows_and_is_reused(prec):
    """Case 4: each call small, large, small on one context: the third result is the first's."""
    with N.Renderer(0, 0x5EED, prec) as r:
        _upload(r, "field")
        for name, (first, large, again) in _sized_calls(r).items():
            assert again == first and large != first, name


def _every_entry_point(r):
    cam, rays = _cam(), _rays()
    seen = dict(_observe(r), sized=_sized_calls(r))
    seen["u8"] = _bits(r.render_frame_u8(cam, SPP, DEPTH))
    seen["occluded"] = _bits(r.occluded_host(rays))
    seen["radiance"] = _bits(r.radiance_rays_host(rays, max_depth=DEPTH, segments=True))
    seen["camera_rays"] = _bits(r.camera_rays_host(cam, _jobs(10, cam)))
    if r.precision == N.RT_PREC_F32:
        assert r.render_diag(cam, SPP, DEPTH)   # (cycle counters among them: run, not compared)
    return seen


@pytest.mark.parametrize("prec", PRECS)
def test_contexts_one_after_another(prec):
    """Case 5: eight contexts, each created, given four_spheres, run through every entry point
    and destroyed; each shows what the first did, and a ninth the fresh context's frame."""
    first = None
    for k in range(8):
        with N.Renderer(0, 0x5EED, prec) as r:
            _upload(r, "four")
            seen = _every_entry_point(r)
        first = first or seen
        assert seen == first, f"context {k}: " + ", ".join(n for n in first if seen[n] != first[n])
    with N.Renderer(0, 0x5EED, prec) as r:
        _upload(r, "four")
        _same(_observe(r), _fresh(prec, "four"), "the ninth context")
