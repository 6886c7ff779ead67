"""GPU parity: the HIP path (through the C ABI) against the reference's goldens and the
oracle.  Needs an MI355X.

Tolerances (stated here, referenced from DESIGN.md):
  fp64 path  -- bit-exact: per-pixel fp64 sums, 8-bit values and world.hit counts equal
                the reference's (counter RNG, seed 0x5EED).
  fp32 path  -- same random numbers, fp32 arithmetic.  Per 8-bit channel |d| <= F32_MAX_LSB
                for every pixel, >= F32_EXACT_FRAC of channels identical, mean |d| <=
                F32_MEAN_LSB; image mean bias |mean d| <= F32_BIAS_LSB.
"""
import json

import numpy as np
import pytest

import oracle_bind as O
from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
# measured on MI355X (r01): max 1 LSB, >= 99.91% exact, mean |d| <= 0.0008, bias <= 0.0007
F32_MAX_LSB = 2
F32_EXACT_FRAC = 0.997
F32_MEAN_LSB = 0.005
F32_BIAS_LSB = 0.003

GOLDENS = sorted(p.stem for p in O.GOLDEN.glob("counter_*.npz"))


def world_for(name: str):
    if name == "random":
        rtweekend.reset_stream()
        return scenes.random_spheres()
    if name == "four":
        return scenes.four_spheres()
    if name == "ground":
        return scenes.ground_only()
    if name == "hollow":
        return scenes.hollow_glass()
    raise ValueError(name)


_WORLDS = {}


def arrays_for(name: str):
    if name not in _WORLDS:
        _WORLDS[name] = api.flatten(world_for(name))
    return _WORLDS[name]


class Rig:
    """One renderer per precision, re-uploading only when the scene changes."""

    def __init__(self, precision):
        self.r = N.Renderer(0, SEED, precision)
        self.scene = None

    def use(self, name):
        if self.scene != name:
            self.r.upload_scene(*arrays_for(name))
            self.scene = name
        return self.r


@pytest.fixture(scope="module")
def f64():
    rig = Rig(N.RT_PREC_F64)
    yield rig
    rig.r.close()


@pytest.fixture(scope="module")
def f32():
    rig = Rig(N.RT_PREC_F32)
    yield rig
    rig.r.close()


def native_camera(width, spp, depth=50, aspect=None, vfov=None, defocus_angle=None):
    cam = scenes.main_camera()
    cam.image_width, cam.samples_per_pixel, cam.max_depth = width, spp, depth
    if aspect is not None:
        cam.aspect_ratio = aspect
    if vfov is not None:
        cam.vfov = vfov
    if defocus_angle is not None:
        cam.defocus_angle = defocus_angle
    return cam.native


def render_golden(rig, name):
    g, meta = O.load_golden(name)
    kw = O.golden_camera_args(meta)
    cam = native_camera(**kw)
    sums, rgb, segs = rig.use(O.golden_scene_name(meta)).render_frame(cam, kw["spp"], kw.get("depth", 50))
    i, j = g["ij"][:, 0], g["ij"][:, 1]
    return g, sums[j, i], rgb[j, i], segs[j, i]


@pytest.mark.parametrize("name", GOLDENS)
def test_f64_bit_exact_vs_reference(f64, name):
    g, sums, rgb, segs = render_golden(f64, name)
    assert np.array_equal(segs.astype(np.int64), g["segments"]), "path structure differs"
    bad = ~(sums == g["sums"]).all(axis=1)
    assert not bad.any(), f"{bad.sum()} of {len(bad)} pixels differ; max |d| {np.abs(sums - g['sums']).max()}"
    assert np.array_equal(rgb, g["rgb"])


def f32_stats(rgb, ref_rgb):
    d = rgb.astype(np.int64) - ref_rgb.astype(np.int64)
    return {"max": int(np.abs(d).max()), "exact": float((d == 0).mean()), "mean_abs": float(np.abs(d).mean()),
            "bias": float(d.mean())}


@pytest.mark.parametrize("name", GOLDENS)
def test_f32_within_tolerance_vs_reference(f32, name):
    g, sums, rgb, segs = render_golden(f32, name)
    st = f32_stats(rgb, g["rgb"])
    print(name, json.dumps(st), "same-path pixels", float((segs.astype(np.int64) == g["segments"]).mean()))
    assert np.isfinite(sums).all()
    assert st["max"] <= F32_MAX_LSB
    assert st["exact"] >= F32_EXACT_FRAC
    assert st["mean_abs"] <= F32_MEAN_LSB
    assert abs(st["bias"]) <= F32_BIAS_LSB


@pytest.mark.parametrize("kernel", [3, 4, 5, "5-3d"])
@pytest.mark.parametrize("name", [n for n in GOLDENS if n.startswith(("counter_c2", "counter_c3", "counter_depth3"))])
def test_f64_kernels_bit_exact(kernel, name):
    """Every fp64 kernel (rt_tuning.f64_kernel: 3 = conservative fp32 slab tests on
    persistent lanes with stored samples, 4 = the same with coherent primaries, 5 = 4 over
    the uniform sphere grid -- on these scenes' grids, one cell tall in y, with the flat walk
    (r06), and "5-3d" with the 3-D walk kept, traversal | RT_TRAV_G3D) renders the reference
    goldens bit for bit."""
    rig = Rig(N.RT_PREC_F64)
    try:
        if kernel == "5-3d":
            rig.r.set_tuning(f64_kernel=5, traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D)
        else:
            rig.r.set_tuning(f64_kernel=kernel)
        g, sums, rgb, segs = render_golden(rig, name)
    finally:
        rig.r.close()
    assert np.array_equal(segs.astype(np.int64), g["segments"])
    assert np.array_equal(sums, g["sums"]) and np.array_equal(rgb, g["rgb"])


def test_f64_full_frame_vs_oracle(f64):
    """Every pixel of a small random-spheres frame against the C restatement."""
    cam_o = O.camera(96, 3)
    sums_o, rgb_o, segs_o = O.render_counter_full(O.OracleScene("random"), cam_o, SEED)
    sums, rgb, segs = f64.use("random").render_frame(native_camera(96, 3), 3, 50)
    assert np.array_equal(segs, segs_o.astype(np.uint32))
    assert np.array_equal(sums, sums_o)
    assert np.array_equal(rgb, rgb_o)


@pytest.mark.parametrize("kernel", [3, 4, 5])
def test_f64_more_than_65535_samples_per_pixel(kernel):
    """The coherent fp64 kernel's FIFO entries hold a sample's index within its pass in 16
    bits; passes are capped at 65535 samples, so a 70,000-spp frame on a tiny image
    (one pass under the default sample buffer otherwise) still equals the oracle."""
    spp = 70000
    sums_o, rgb_o, segs_o = O.render_counter_full(O.OracleScene("four"), O.camera(4, spp), SEED)
    rig = Rig(N.RT_PREC_F64)
    try:
        rig.r.set_tuning(f64_kernel=kernel)
        sums, rgb, segs = rig.use("four").render_frame(native_camera(4, spp), spp, 50)
    finally:
        rig.r.close()
    assert np.array_equal(segs, segs_o.astype(np.uint32))
    assert np.array_equal(sums, sums_o)
    assert np.array_equal(rgb, rgb_o)


def test_pixelmatch_through_reference_api():
    """tests/tests.cpp:35-45 verbatim in shape: get_ray on the host stream, ray_color on
    the GPU continuing that stream -- equal to the reference's value and consumption."""
    pm = json.loads((O.GOLDEN / "pixelmatch.json").read_text())
    rtweekend.reset_stream()
    world = scenes.ground_only()
    cam = scenes.main_camera()
    cam.initialize()
    w, h = cam.image_size()
    r = cam.get_ray(w // 2, h // 2)
    assert rtweekend.stream().copy().idx == 2 * pm["draws_before_ray_color"]
    c = cam.ray_color(r, cam.max_depth, world)
    assert list(c) == pm["ray_color"]
    assert rtweekend.stream().idx == 2 * (pm["draws_before_ray_color"] + pm["draws_in_ray_color"])
    assert all(abs(a - b) < 1e-3 for a, b in zip(c, pm["expected_similar_to"]))


def test_trace_tape_matches_oracle(f64):
    """Random rays through the random scene on explicit tapes vs orc_trace_tape."""
    rng = np.random.default_rng(3)
    sc = O.OracleScene("random")
    r = f64.use("random")
    for _ in range(64):
        ray = [*rng.uniform(-3, 3, 3) + [0, 2, 0], *rng.normal(size=3), rng.uniform()]
        tape = rng.uniform(size=400)
        col, used = r.trace_tape(ray, 50, tape)
        out, used_o = O.trace_tape(sc, ray, 50, tape)
        assert used == used_o and list(col) == out


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_tiling_is_invisible(f32, nshards):
    """Rendering the frame as N interleaved shards and unsharding gives the 1-shard frame
    bit for bit (the multi-GPU split cannot change a pixel)."""
    import torch
    W, H, spp = 203, 117, 4
    cam = native_camera(W, spp)
    cam.image_height = H
    r = f32.use("random")
    ref, _, _ = r.render_frame(cam, spp, 50)
    mx = N.shard_layout(W, H, 0, nshards).max_shard_tiles
    gathered = torch.zeros(nshards * mx * 64 * 3, dtype=torch.float32, device="cuda")
    # the renderer's own stream is non-blocking: order torch's fill before it
    torch.cuda.synchronize()
    for s in range(nshards):
        r.render(cam, spp, 50, s, nshards, gathered.data_ptr() + s * mx * 64 * 3 * 4)
    frame = torch.empty(H * W * 3, dtype=torch.float32, device="cuda")
    r.unshard(gathered.data_ptr(), W, H, nshards, frame.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().reshape(H, W, 3), ref)


@pytest.mark.parametrize("prec", [N.RT_PREC_F32, N.RT_PREC_F64])
@pytest.mark.parametrize("nctx", [2, 3])
def test_multi_context_frame(prec, nctx):
    """rt_render_frame_multi with `nctx` contexts (all on device 0 here; one per GPU in
    production) assembles the same frame as one context's rt_render_frame, bit for bit."""
    W, H, spp = 131, 77, 3
    cam = native_camera(W, spp)
    cam.image_height = H
    rs = [N.Renderer(0, SEED, prec) for _ in range(nctx)]
    try:
        for r in rs:
            r.upload_scene(*arrays_for("random"))
        ref, ref_rgb, _ = rs[0].render_frame(cam, spp, 50)
        sums, rgb = N.render_frame_multi(rs, cam, spp, 50)
        assert np.array_equal(sums, ref) and np.array_equal(rgb, ref_rgb)
        sums2, _ = N.render_frame_multi(rs[::-1], cam, spp, 50)   # gather on another context
        assert np.array_equal(sums2, ref)
        small = native_camera(12, spp)                             # 2 tiles: a context gets none
        small.image_height = 8
        ref, _, _ = rs[0].render_frame(small, spp, 50)
        assert np.array_equal(N.render_frame_multi(rs, small, spp, 50)[0], ref)
        with pytest.raises(N.RtError):
            N.render_frame_multi([rs[0], rs[0]], cam, spp, 50)
    finally:
        for r in rs:
            r.close()


def test_device_quantize_equals_write_color(f32):
    sums, rgb, _ = f32.use("four").render_frame(native_camera(64, 5), 5, 50)
    host = np.array([O.write_color(c, 5) for c in sums.reshape(-1, 3).astype(np.float64)]).reshape(rgb.shape)
    assert np.array_equal(rgb, host)


def test_edge_cases(f32, f64):
    r = f32.use("random")
    cam = native_camera(16, 1)
    s, rgb, segs = r.render_frame(cam, 0, 50)             # spp = 0: nothing summed
    assert not s.any() and not segs.any()
    s, rgb, segs = r.render_frame(cam, 4, 0)             # depth 0: ray_color returns 0 (camera_cpu.h:12-13)
    assert not s.any() and not segs.any()
    one = native_camera(1, 2)                              # 1-pixel image: H = max(1, int(1/aspect))
    assert one.image_height == 1
    s, _, segs = r.render_frame(one, 2, 50)
    assert s.shape == (1, 1, 3) and segs[0, 0] >= 2
    # ragged width (not a multiple of the 8x8 tile) against the oracle
    cam_o = O.camera(37, 2)
    so, ro, go = O.render_counter_full(O.OracleScene("four"), cam_o, SEED)
    s64, r64, g64 = f64.use("four").render_frame(native_camera(37, 2), 2, 50)
    assert np.array_equal(s64, so) and np.array_equal(g64, go.astype(np.uint32))


def test_degenerate_scenes():
    sky = N.Renderer(0, SEED, N.RT_PREC_F64)
    empty_s = np.zeros(0, dtype=N.SPHERE_DTYPE)
    empty_m = np.zeros(0, dtype=N.MATERIAL_DTYPE)
    sky.upload_scene(empty_s, empty_m)                   # no spheres: every ray sees the sky
    s, _, segs = sky.render_frame(native_camera(24, 2), 2, 50)
    assert (segs == 2).all() and (s > 0).all()
    w = api.hittable_list(api.sphere((0, 1, 0), 0.5, api.lambertian((0.2, 0.4, 0.6))))  # single-leaf BVH
    sky.upload_scene(*api.flatten(w))
    info = sky.scene_info()
    assert info.bvh_nodes == 1 and info.big_spheres == 0
    sky.render_frame(native_camera(24, 2), 2, 50)
    bad = np.zeros(1, dtype=N.SPHERE_DTYPE)
    bad[0]["radius"], bad[0]["mat"] = 1.0, 3
    with pytest.raises(N.RtError):
        sky.upload_scene(bad, np.zeros(1, dtype=N.MATERIAL_DTYPE))
    sky.close()


@pytest.mark.parametrize("coherent", [{}, dict(traversal=88), dict(front_spheres=0)],
                         ids=["default", "no_cull", "no_front"])
@pytest.mark.parametrize("case", ["empty", "one_sphere", "four", "random"])
def test_coherent_kernel_equals_one_path_per_lane(case, coherent):
    """The coherent-primary kernel (default) against the one-path-per-lane kernel on the
    edge cases of its batching and FIFO: no spheres (no BVH: every camera ray ends in the
    batch), a single-leaf BVH, ragged and 1-pixel frames, depth 0 / 1 / 2 (paths that end
    at the camera hit or the first bounce), 1 spp and a sample range with accumulation --
    same sums and segment counts bit for bit; also without pop culling (88)."""
    import torch
    if case == "empty":
        arrays = (np.zeros(0, dtype=N.SPHERE_DTYPE), np.zeros(0, dtype=N.MATERIAL_DTYPE))
    elif case == "one_sphere":
        arrays = api.flatten(api.hittable_list(api.sphere((0, 1, 0), 0.5, api.lambertian((0.2, 0.4, 0.6)))))
    else:
        arrays = arrays_for(case)
    rs = []
    for tune in (coherent, dict(block=512, traversal=8)):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        r.set_tuning(**tune)
        r.upload_scene(*arrays)
        rs.append(r)
    try:
        for W, spp, depth in ((37, 3, 50), (1, 2, 50), (24, 1, 1), (24, 2, 2), (16, 4, 0), (64, 5, 50)):
            cam = native_camera(W, spp)
            a = rs[0].render_frame(cam, spp, depth)
            b = rs[1].render_frame(cam, spp, depth)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (case, W, spp, depth)
        # progressive: [0, 3) + [3, 7) accumulated equals the other kernel's one launch
        W = 40
        cam = native_camera(W, 7)
        lay = N.shard_layout(W, cam.image_height, 0, 1)
        buf = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rs[0].render_range(cam, 0, 3, 50, 0, 1, 0, buf.data_ptr(), None)
        rs[0].render_range(cam, 3, 4, 50, 0, 1, 1, buf.data_ptr(), None)
        ref = torch.zeros_like(buf)
        torch.cuda.synchronize()   # the zero fills run on torch's stream, the renders on their own
        rs[1].render_range(cam, 0, 7, 50, 0, 1, 0, ref.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(buf, ref), case
    finally:
        for r in rs:
            r.close()


def test_full_size_c3_properties(f32):
    """Config 3 (1920x1080 @ 256 spp) at full size: deterministic, finite, and the path
    statistics of the survey (2.58 world.hit calls per primary ray)."""
    cam = native_camera(1920, 256)
    r = f32.use("random")
    a, rgb_a, segs = r.render_frame(cam, 256, 50)
    b, _, _ = r.render_frame(cam, 256, 50)
    assert np.array_equal(a, b)
    assert np.isfinite(a).all() and (a >= 0).all()
    per_primary = segs.astype(np.float64).sum() / (1920 * 1080 * 256)
    assert 2.50 < per_primary < 2.70, per_primary


@pytest.mark.parametrize("scene,width", [("random", 1920), ("random", 3840), ("four", 1920)])
def test_sphere_grid_equals_tree_at_full_size(scene, width):
    """The uniform sphere grid finds every closest hit the tree finds: full-size frames
    (C3's 1080p and C5's 4K view of the random field, C2's four spheres) at 4 spp, sums
    and per-pixel world.hit counts bit for bit, grid (the default: on these grids, one cell
    tall in y, the flat walk, r06) against the grid's 3-D walk and the tree."""
    out = []
    for trav in (N.RT_TRAV_DEFAULT, N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D, N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        try:
            r.set_tuning(traversal=trav)
            r.upload_scene(*arrays_for(scene))
            info = r.scene_info()
            assert bool(info.render_traversal & N.RT_TRAV_GRID) == bool(trav & N.RT_TRAV_GRID)
            assert info.grid_res[1] == 1
            assert bool(info.render_traversal & N.RT_TRAV_GFLAT) == (trav == N.RT_TRAV_DEFAULT)
            sums, _, segs = r.render_frame(native_camera(width, 4), 4, 50)
            out.append((sums, segs))
        finally:
            r.close()
    for k in (1, 2):
        assert np.array_equal(out[0][1], out[k][1])
        assert np.array_equal(out[0][0], out[k][0])


@pytest.mark.parametrize("width", [1920, 3840])
def test_f64_grid_kernel_equals_tree_kernel_at_full_size(width):
    """fp64 kernel 5 (the sphere grid, cells picked in fp32; its flat walk here, and the 3-D
    walk) against kernel 4 (the tree with conservative fp32 boxes): full-size C3 / C5-view
    frames at 2 spp, bit for bit."""
    out = []
    for kernel, trav in ((4, N.RT_TRAV_DEFAULT), (5, N.RT_TRAV_DEFAULT), (5, N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D)):
        r = N.Renderer(0, SEED, N.RT_PREC_F64)
        try:
            r.set_tuning(f64_kernel=kernel, traversal=trav)
            r.upload_scene(*arrays_for("random"))
            out.append(r.render_frame(native_camera(width, 2), 2, 50))
        finally:
            r.close()
    for k in (1, 2):
        assert np.array_equal(out[0][2], out[k][2])
        assert np.array_equal(out[0][0], out[k][0])


@pytest.mark.parametrize("prec", [N.RT_PREC_F32, N.RT_PREC_F64])
@pytest.mark.parametrize("scale,shift", [(100.0, (1.0e4, 0.0, -1.0e4)), (1.0e-3, (0.0, 0.0, 0.0))])
def test_sphere_grid_equals_tree_scaled_scene(scale, shift, prec):
    """The grid's padding is relative to the scene (its span and largest coordinate): the
    random field scaled by 100 and moved 1e4 away from the origin (the R = 1 spheres join
    the R >= 64 class there), and scaled by 1e-3, renders the tree's frame bit for bit
    (camera scaled with it)."""
    S, M = arrays_for("random")
    S = S.copy()
    S["center"] = S["center"] * scale + np.array(shift)
    S["center_vec"] = S["center_vec"] * scale
    S["radius"] = S["radius"] * scale
    cam = scenes.main_camera()
    cam.image_width, cam.samples_per_pixel = 320, 4
    cam.lookfrom = tuple(np.array((13.0, 2.0, 3.0)) * scale + np.array(shift))
    cam.lookat = tuple(np.array(shift, dtype=float))
    cam.focus_dist = 10.0 * scale
    out = []
    for trav in (N.RT_TRAV_DEFAULT, N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID):
        r = N.Renderer(0, SEED, prec)
        try:
            r.set_tuning(traversal=trav)   # (fp64: f64_kernel 0 picks 5 with the grid flag, else 4)
            r.upload_scene(S, M)
            assert bool(r.scene_info().render_traversal & N.RT_TRAV_GRID) == (trav == N.RT_TRAV_DEFAULT)
            out.append(r.render_frame(cam.native, 4, 50))
        finally:
            r.close()
    assert np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0])


def far_cameras(dist, width=160, spp=2):
    """main.cpp's view of the random field from `dist` units away (same direction, the field
    filling the frame, no defocus): the native camera and the oracle's."""
    look = np.array((13.0, 2.0, 3.0))
    frm = tuple(look / np.linalg.norm(look) * dist)
    vfov = float(np.degrees(2 * np.arctan(3.0 / dist)))
    cam = scenes.main_camera()
    cam.image_width, cam.samples_per_pixel = width, spp
    cam.lookfrom, cam.vfov, cam.defocus_angle, cam.focus_dist = frm, vfov, 0.0, float(dist)
    oc = O.OrcCamera()
    O.lib().orc_camera_defaults(O.C.byref(oc))
    oc.image_width, oc.samples_per_pixel, oc.max_depth = width, spp, 50
    oc.lookfrom = O.D3(*frm)
    oc.vfov, oc.defocus_angle, oc.focus_dist = vfov, 0.0, float(dist)
    O.lib().orc_camera_initialize(O.C.byref(oc))
    return cam, oc


def field_arrays(ground: bool):
    """The random scene's arrays, with or without its R = 1000 ground."""
    S, M = arrays_for("random")
    return (S, M) if ground else (S[S["radius"] < 64].copy(), M)


def test_grid_reach():
    """VERDICT r05 #1 / ADVICE r05 (r06): the grid walk is exact and ends only for ray origins
    within +-grid_far_o (~250 units for the random field); a launch whose camera or scene could
    start a ray beyond it renders with the tree.  main.cpp's camera walks (its rays start on
    the field, at the camera, or on the ground within the tangent distance from them -- 66
    units); a camera 150 units out sees ground ~350 units away (the tree); without the ground
    it walks again; 2e4 units out never walks."""
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        r.upload_scene(*field_arrays(True))
        info = r.scene_info()
        assert 200 < info.grid_far_o < 400, info.grid_far_o
        assert r.grid_reach(native_camera(320, 1))
        assert not r.grid_reach(far_cameras(150.0)[0].native)
        assert not r.grid_reach(far_cameras(2.0e4)[0].native)
        r.upload_scene(*field_arrays(False))
        assert r.grid_reach(far_cameras(150.0)[0].native)
        assert not r.grid_reach(far_cameras(2.0e4)[0].native)
        assert r.scene_info().render_traversal & N.RT_TRAV_GRID   # (the plan of a launch within reach)
    finally:
        r.close()


FAR_CASES = [(150.0, False, True), (150.0, True, False), (2.0e4, True, False), (2.0e7, True, False)]


@pytest.mark.parametrize("dist,ground,walks", FAR_CASES)
def test_f64_grid_walk_from_far_cameras(dist, ground, walks):
    """fp64 with the grid asked for (the default, f64_kernel 0 -> 5) from far cameras: kernel 5
    where the launch is within the grid's reach, else the tree's kernel 4 -- either way equal to
    kernel 4 bit for bit and to the oracle on sampled pixels."""
    cam, oc = far_cameras(dist)
    S, M = field_arrays(ground)
    out = []
    for kernel in (4, 0):
        r = N.Renderer(0, SEED, N.RT_PREC_F64)
        try:
            r.set_tuning(f64_kernel=kernel)
            r.upload_scene(S, M)
            if kernel == 0:
                assert r.grid_reach(cam.native) == walks
            out.append(r.render_frame(cam.native, 2, 50))
        finally:
            r.close()
    assert np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0])
    sums = out[1][0]
    assert (out[1][2] > 1).mean() > 0.3   # the field, not the sky: many primaries hit something
    rng = np.random.default_rng(int(dist))
    ij = np.stack([rng.integers(0, 160, 24), rng.integers(0, 90, 24)], axis=1).astype(np.int32)
    os_, _, oseg = O.render_counter(O.OracleScene.from_arrays(S, M), oc, SEED, ij)
    assert np.array_equal(sums[ij[:, 1], ij[:, 0]], os_)
    assert np.array_equal(out[1][2][ij[:, 1], ij[:, 0]].astype(np.uint64), oseg)


@pytest.mark.parametrize("dist,ground,walks", FAR_CASES[:3])
def test_f32_grid_walk_from_far_cameras(dist, ground, walks):
    """The fp32 path from the same cameras: the grid (within reach) or the tree renders the
    tree's frame bit for bit."""
    cam, _ = far_cameras(dist)
    out = []
    for trav in (N.RT_TRAV_DEFAULT, N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        try:
            r.set_tuning(traversal=trav)
            r.upload_scene(*field_arrays(ground))
            if trav == N.RT_TRAV_DEFAULT:
                assert r.grid_reach(cam.native) == walks
            out.append(r.render_frame(cam.native, 2, 50))
        finally:
            r.close()
    assert np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.parametrize("prec", [N.RT_PREC_F32, N.RT_PREC_F64])
def test_sphere_grid_time_slabs_with_motion_on_every_axis(prec):
    """The time slabs (ABI 9) with spheres moving along every axis, many by more than a cell
    over the shutter (main.cpp's spheres only move up): each ray's walk clipped to its time
    slab's box renders the tree's frame and hit counts bit for bit at 1, 7 and 64 slabs."""
    S, M = arrays_for("random")
    S = S.copy()
    g = np.random.default_rng(7)
    small = S["radius"] < 0.5
    S["moving"][small] = 1
    S["center_vec"][small] = g.uniform(-0.6, 0.6, (int(small.sum()), 3))
    cam = native_camera(160, 6)
    r = N.Renderer(0, SEED, prec)
    try:
        r.set_tuning(traversal=N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID)
        r.upload_scene(S, M)
        ref = r.render_frame(cam, 6, 50)
    finally:
        r.close()
    for slabs in (1, 7, 64):
        r = N.Renderer(0, SEED, prec)
        try:
            r.set_tuning(traversal=N.RT_TRAV_DEFAULT, sphere_grid_time_slabs=slabs)
            r.upload_scene(S, M)
            assert r.scene_info().render_traversal & N.RT_TRAV_GRID, slabs
            got = r.render_frame(cam, 6, 50)
        finally:
            r.close()
        assert np.array_equal(got[2], ref[2]), slabs
        assert np.array_equal(got[0], ref[0]), slabs


def test_statistically_equivalent_to_committed_image(f32):
    """Counter RNG vs the reference's sequential stream: the same image up to sampling
    noise (400x225 @ 30 spp against /root/reference/image.ppm's pixels).  Block means
    of the difference are z-tested against their own spread; thresholds calibrated on
    the fp64 oracle over several seeds (max block |z| 2.7-4.3, global |z| <= 1.4), which
    shows the same numbers as the GPU for seed 0x5EED."""
    import gzip
    raw = gzip.open(O.GOLDEN / "image_ref_p6.ppm.gz").read()
    ref = np.frombuffer(raw[len(b"P6\n400 225\n255\n"):], dtype=np.uint8).reshape(225, 400, 3).astype(np.float64)
    _, rgb, _ = f32.use("random").render_frame(native_camera(400, 30), 30, 50)
    d = rgb.astype(np.float64) - ref
    assert abs(d.mean()) < 0.1
    assert abs(d.mean() / (d.std() / np.sqrt(d.size))) < 4.0
    b = d.reshape(9, 25, 16, 25, 3)
    z = b.mean(axis=(1, 3)) / (b.std(axis=(1, 3)) / 25 + 1e-3)
    assert np.abs(z).max() < 6.0


@pytest.mark.parametrize("tuning", [dict(block=512, traversal=8),   # one path per lane
                                    dict(traversal=88),    # the default without pop culling
                                    dict(traversal=728),   # the default without LDS pixel sums
                                    dict(traversal=216),   # ... and without pop culling
                                    dict(max_leaf=4),   # its LDS pixel sums would cost occupancy: auto NOSUM
                                    dict(max_leaf=2, cost_intersect=1.0),
                                    dict(item_balance=0.0), dict(item_samples=2, item_balance=0.0),
                                    dict(item_samples=1), dict(coh_refill=1), dict(coh_refill=64),
                                    dict(front_spheres=0),   # every sphere in the tree
                                    dict(front_spheres=16), dict(front_spheres=0, block=512, traversal=8),
                                    dict(grid_workgroups=3), dict(grid_workgroups=4096),
                                    # the uniform sphere grid instead of the tree, at several densities
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID, sphere_grid_density=2.0),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID, sphere_grid_density=0.25),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID, sphere_grid_density=8.0),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID, front_spheres=0),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID | N.RT_TRAV_NOSUM),
                                    # the grid's 3-D walk instead of the flat one (r06)
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D | N.RT_TRAV_NOSUM),
                                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GFLAT | N.RT_TRAV_NOSUM),
                                    # the walk clipped to the spheres' box over the whole shutter, or
                                    # over 3 / 64 time slabs of it (the default: 32)
                                    dict(sphere_grid_time_slabs=1), dict(sphere_grid_time_slabs=3),
                                    dict(sphere_grid_time_slabs=64),
                                    dict(traversal=600)])   # the tree, whatever the default
def test_tuning_never_changes_pixels(tuning):
    """BVH shape, traversal order, the kernel (one path per lane, coherent primaries with and
    without LDS sums or pop culling), shade rounds and the work-queue item sizes only change speed:
    the closest hit is order-independent, the fixed-point sums are order-free and every
    inlined copy of a step rounds alike (-ffp-contract=on), so every tuning gives the
    default frame bit for bit."""
    W, spp = 160, 6
    base = N.Renderer(0, SEED, N.RT_PREC_F32)
    base.upload_scene(*arrays_for("random"))
    ref, _, ref_segs = base.render_frame(native_camera(W, spp), spp, 50)
    base.close()
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    r.set_tuning(**tuning)
    r.upload_scene(*arrays_for("random"))
    got, _, segs = r.render_frame(native_camera(W, spp), spp, 50)
    r.close()
    assert np.array_equal(segs, ref_segs)
    assert np.array_equal(got, ref)


def test_sphere_grid_plan():
    """RT_TRAV_GRID renders through the uniform sphere grid where rt_upload_scene built one
    (the random field; the four-sphere scene's three R = 1 spheres) and through the tree where
    it did not (the ground alone is in the big-sphere class; density 0 builds none)."""
    grid = N.RT_TRAV_DEFAULT | N.RT_TRAV_GRID
    for scene, density, used in (("random", 2.0, True), ("four", 2.0, True), ("ground", 2.0, False),
                                 ("random", 0.0, False)):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        try:
            r.set_tuning(traversal=grid, sphere_grid_density=density)
            r.upload_scene(*arrays_for(scene))
            info = r.scene_info()
            assert bool(info.render_traversal & N.RT_TRAV_GRID) == used, (scene, density)
            res = list(info.grid_res)
            if used:   # every sphere outside the front list / ground class is listed at least once
                assert min(res) >= 1 and info.grid_entries >= info.num_spheres - 3 - info.big_spheres
            else:
                assert res == [0, 0, 0] or density > 0
            r.render_frame(native_camera(16, 1), 1, 50)
        finally:
            r.close()
    # r06: the flat walk (TRAV_GFLAT) exactly where the grid is one cell tall in y and the 3-D
    # walk is not asked for; the field stretched 20x in y gets a 3-D grid and walk, which
    # renders the tree's frame
    S, M = arrays_for("random")
    tall = S.copy()
    tall["center"][:, 1] *= 20.0
    tall["center_vec"][:, 1] *= 20.0
    for arrays, trav, flat in ((arrays_for("random"), grid, True), (arrays_for("random"), grid | N.RT_TRAV_G3D, False),
                               ((tall, M), grid, False)):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        try:
            r.set_tuning(traversal=trav)
            r.upload_scene(*arrays)
            info = r.scene_info()
            assert info.render_traversal & N.RT_TRAV_GRID and (info.grid_res[1] == 1) == (arrays[0] is not tall)
            assert bool(info.render_traversal & N.RT_TRAV_GFLAT) == flat, (trav, list(info.grid_res))
        finally:
            r.close()
    out = []
    for trav in (grid, N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        try:
            r.set_tuning(traversal=trav)
            r.upload_scene(tall, M)
            out.append(r.render_frame(native_camera(160, 4), 4, 50))
        finally:
            r.close()
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][0], out[1][0])
    # two far-apart clusters (most cells of a grid over both empty): the tree, not a grid
    S, M = arrays_for("random")
    S = S.copy()
    S["center"][1::2, 0] += 500.0
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        r.upload_scene(S, M)
        assert list(r.scene_info().grid_res) == [0, 0, 0]
        assert not r.scene_info().render_traversal & N.RT_TRAV_GRID
        r.render_frame(native_camera(16, 1), 1, 50)
    finally:
        r.close()
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        for bad in (dict(sphere_grid_density=-1.0), dict(sphere_grid_density=float("nan")),
                    dict(sphere_grid_density=100.0), dict(sphere_grid_time_slabs=0),
                    dict(sphere_grid_time_slabs=65)):
            with pytest.raises(N.RtError):
                r.set_tuning(**bad)
    finally:
        r.close()


def test_item_tuning_is_validated():
    """rt_set_tuning rejects work-queue item sizes outside 1..32, negative balances, fp64
    kernels that are not built and unknown traversal flags."""
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        for bad in (dict(item_samples=0), dict(item_samples=33), dict(item_balance=-1.0),
                    dict(mesh_item_balance=float("nan")), dict(f64_kernel=-1), dict(f64_kernel=6),
                    dict(f64_kernel=1), dict(f64_kernel=2),   # removed in r04
                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_TBIN),   # removed in r04
                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_MTOP),   # removed in r04
                    dict(traversal=2048), dict(traversal=8192),
                    dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_GFLAT | N.RT_TRAV_G3D),
                    dict(traversal=N.RT_TRAV_DEFAULT | (1 << 19))):
            with pytest.raises(N.RtError):
                r.set_tuning(**bad)
        r.set_tuning(item_samples=32, item_balance=0.0, mesh_item_balance=100.0)
        # the mesh if-if flag is accepted and dropped for sphere scenes
        r.set_tuning(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_MIFIF, f64_kernel=3)
        r.upload_scene(*arrays_for("four"))
        # (its grid is one cell tall in y: the flat walk is added)
        assert r.scene_info().render_traversal == N.RT_TRAV_DEFAULT | N.RT_TRAV_GFLAT
        r.render_frame(native_camera(16, 1), 1, 50)
    finally:
        r.close()


def untile(buf: np.ndarray, W: int, H: int, C: int) -> np.ndarray:
    """One shard's buffer (rt_shard_info layout: 8x8 tiles in row-major tile order, pixel
    (x%8, y%8) at (y%8)*8 + x%8 of its tile) -> [H, W, C]."""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    t = buf[: tiles_x * tiles_y * 64 * C].reshape(tiles_y, tiles_x, 8, 8, C)
    return t.transpose(0, 2, 1, 3, 4).reshape(tiles_y * 8, tiles_x * 8, C)[:H, :W]


def quantize_sums(sums: np.ndarray, spp: int) -> np.ndarray:
    """write_color (color.h:14-35) of fp sums, through the oracle's restatement."""
    flat = sums.reshape(-1, 3)
    return np.array([O.write_color(c, spp) for c in flat.tolist()], np.int64).reshape(sums.shape)


@pytest.mark.parametrize("prec", [N.RT_PREC_F32, N.RT_PREC_F64])
def test_progressive_ranges_equal_one_launch(prec):
    """§8(f)4: a frame rendered as sample ranges [0,5) + [5,6) + [6,12) with accumulation
    is bit-identical to one 12-sample launch (sums continue in sample order), and after
    each range it is the oracle's frame of that many samples (camera.h:40-44 keys samples
    0..k-1): fp64 bit for bit (sums, world.hit counts), fp32 within the F32_* tolerance."""
    import torch
    W, spp = 96, 12
    cam = native_camera(W, spp)
    H = cam.image_height
    r = N.Renderer(0, SEED, prec)
    r.upload_scene(*arrays_for("random"))
    lay = N.shard_layout(W, cam.image_height, 0, 1)
    dt = torch.float64 if prec == N.RT_PREC_F64 else torch.float32
    one = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=dt, device="cuda")
    one_s = torch.zeros(lay.max_shard_tiles * 64, dtype=torch.int32, device="cuda")
    prog = torch.full_like(one, 123.0)
    prog_s = torch.zeros_like(one_s)
    # the renderer's own stream is non-blocking: torch's fills must finish first
    torch.cuda.synchronize()
    r.render(cam, spp, 50, 0, 1, one.data_ptr(), one_s.data_ptr())
    osc = O.OracleScene("random")
    for i, (b, n) in enumerate([(0, 5), (5, 1), (6, 6)]):
        r.render_range(cam, b, n, 50, 0, 1, i > 0, prog.data_ptr(), prog_s.data_ptr())
        torch.cuda.synchronize()
        k = b + n
        osums, orgb, osegs = O.render_counter_full(osc, O.camera(W, k), SEED)
        got = untile(prog.cpu().numpy(), W, H, 3)
        got_s = untile(prog_s.cpu().numpy(), W, H, 1)[..., 0]
        if prec == N.RT_PREC_F64:
            assert np.array_equal(got_s.astype(np.int64), osegs.astype(np.int64)), f"{k} samples: path structure"
            bad = ~(got == osums).all(axis=2)
            assert not bad.any(), f"{k} samples: {bad.sum()} of {bad.size} pixels differ from the oracle"
        else:
            st = f32_stats(quantize_sums(got, k), orgb)
            print(k, "samples vs oracle", json.dumps(st))
            assert st["max"] <= F32_MAX_LSB and st["exact"] >= F32_EXACT_FRAC
            assert st["mean_abs"] <= F32_MEAN_LSB and abs(st["bias"]) <= F32_BIAS_LSB
    r.close()
    d = (one - prog).abs()
    assert torch.equal(one_s, prog_s), f"segment counts differ at {(one_s != prog_s).sum().item()} pixels"
    assert torch.equal(one, prog), (f"{(d > 0).sum().item()} of {d.numel()} sums differ, max |d| {d.max().item()} "
                                    f"at {d.argmax().item()}: {one[d.argmax()].item()} vs {prog[d.argmax()].item()}")


@pytest.mark.parametrize("prec", [N.RT_PREC_F32, N.RT_PREC_F64])
def test_sample_chunking_is_bit_identical(prec):
    """A sample buffer capped at 16 MiB forces the fp64 kernels into several passes (each
    with its ordered reduction); sums and world.hit counts must equal the one-pass launch
    exactly.  (rt_tuning.chunk_waves is reserved since r04 -- the one-wave-per-tile fp64
    kernels it split were removed -- and must change nothing.)"""
    W, spp = 120, 10
    cam = native_camera(W, spp)
    S, M = arrays_for("random")
    frames = {}
    for cw, cap in [(0, 16384), (1 << 20, 16384), (300, 16384), (1 << 20, 16)]:
        r = N.Renderer(0, SEED, prec)
        r.set_tuning(chunk_waves=cw, sample_buffer_mb=cap)
        r.upload_scene(S, M)
        frames[(cw, cap)] = r.render_frame(cam, spp, 50)
        r.close()
    ref = frames[(0, 16384)]
    for k, f in frames.items():
        assert np.array_equal(f[0], ref[0]) and np.array_equal(f[2], ref[2]), k


def test_sample_chunking_shards_and_ranges():
    """Shards of a 3-way split rendered as accumulated sample ranges agree bit for bit
    whatever the (reserved) chunk_waves field holds."""
    import torch
    W, spp = 96, 12
    cam = native_camera(W, spp)
    S, M = arrays_for("random")
    H = cam.image_height
    outs = []
    for cw in (0, 1 << 20):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
        r.set_tuning(chunk_waves=cw)
        r.upload_scene(S, M)
        lay = N.shard_layout(W, H, 0, 3)
        buf = torch.zeros(3 * lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
        segs = torch.zeros(3 * lay.max_shard_tiles * 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for sh in range(3):
            off = sh * lay.max_shard_tiles * 64
            for i, (b, n) in enumerate([(0, 5), (5, 7)]):
                r.render_range(cam, b, n, 50, sh, 3, i > 0, buf.data_ptr() + off * 3 * 4, segs.data_ptr() + off * 4)
        torch.cuda.synchronize()
        outs.append((buf.cpu().numpy(), segs.cpu().numpy()))
        r.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_accumulate_into_reallocated_buffer():
    """rt_render_range(accumulate=1) on a buffer whose address the context has sums for,
    but whose contents changed (freed and handed out again for another frame, or written
    by the caller): the context must continue from the buffer's float values -- exactly
    what a context with no state for that address does -- not from its stale sums."""
    import torch
    W, spp = 64, 4
    cam = native_camera(W, spp)
    S, M = arrays_for("random")
    lay = N.shard_layout(W, cam.image_height, 0, 1)
    n = lay.max_shard_tiles * 64 * 3
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    fresh = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        r.upload_scene(S, M)
        fresh.upload_scene(S, M)
        buf = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render_range(cam, 0, spp, 50, 0, 1, 0, buf.data_ptr(), None)   # state for this address
        torch.cuda.synchronize()
        other = torch.rand(n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        other[5] = float("nan")
        other[7] = float("inf")
        buf.copy_(other)                                                  # "another frame" at the same address
        ref = other.clone()
        torch.cuda.synchronize()
        r.render_range(cam, spp, spp, 50, 0, 1, 1, buf.data_ptr(), None)
        fresh.render_range(cam, spp, spp, 50, 0, 1, 1, ref.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(buf.isnan(), ref.isnan())
        assert torch.equal(torch.nan_to_num(buf), torch.nan_to_num(ref))
        # and an untouched buffer still continues exactly (one launch == two ranges)
        one = torch.zeros(n, dtype=torch.float32, device="cuda")
        two = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render_range(cam, 0, 2 * spp, 50, 0, 1, 0, one.data_ptr(), None)
        r.render_range(cam, 0, spp, 50, 0, 1, 0, two.data_ptr(), None)
        r.render_range(cam, spp, spp, 50, 0, 1, 1, two.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(one, two)
    finally:
        r.close()
        fresh.close()


def test_split_launch_above_packed_limit():
    """spp > 8191 (the packed per-launch sums' limit) is rendered as consecutive
    sub-ranges: bit-identical to the same ranges requested explicitly, and
    rt_last_kernel_ms covers the whole call."""
    import torch
    cam = native_camera(8, 8200, depth=2, aspect=1.0)   # one 8x8 tile
    S, M = arrays_for("four")
    r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        r.upload_scene(S, M)
        lay = N.shard_layout(8, cam.image_height, 0, 1)
        n = lay.max_shard_tiles * 64 * 3
        a = torch.zeros(n, dtype=torch.float32, device="cuda")
        b = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render_range(cam, 0, 8200, 2, 0, 1, 0, a.data_ptr(), None)
        whole_ms = r.last_kernel_ms()
        r.render_range(cam, 0, 8191, 2, 0, 1, 0, b.data_ptr(), None)
        first_ms = r.last_kernel_ms()
        r.render_range(cam, 8191, 9, 2, 0, 1, 1, b.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert whole_ms >= 0.9 * first_ms, (whole_ms, first_ms)
    finally:
        r.close()


def test_albedo_above_one():
    """rt_upload_scene accepts albedo > 1 (the reference does: lambertian(color)): radiance
    can then exceed 1, so a chunk sum may leave the exact packed range and go through the
    64-bit atomics (both kinds can meet in one pixel).  The frame must stay finite and
    deterministic, a split into sample ranges must agree with one launch to fp32 rounding
    (sums of values above 1 are no longer exact, so no longer order-free), and the frame
    must agree with the fp64 path.  (fp32 pixel sums saturate to +inf above 2^34.)"""
    import torch
    S, M = arrays_for("four")
    M = M.copy()
    M["albedo"][:] = np.minimum(M["albedo"] * 2.0 + 0.3, 1.5)
    W, spp = 64, 16
    cam = native_camera(W, spp)
    out = {}
    for prec in (N.RT_PREC_F32, N.RT_PREC_F64):
        r = N.Renderer(0, SEED, prec)
        r.upload_scene(S, M)
        out[prec] = [r.render_frame(cam, spp, 50) for _ in range(2)]
        if prec == N.RT_PREC_F32:
            lay = N.shard_layout(W, cam.image_height, 0, 1)
            buf = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(W * cam.image_height * 3, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.render_range(cam, 0, 5, 50, 0, 1, 0, buf.data_ptr())
            r.render_range(cam, 5, spp - 5, 50, 0, 1, 1, buf.data_ptr())
            r.unshard(buf.data_ptr(), W, cam.image_height, 1, frame.data_ptr())
            torch.cuda.synchronize()
            split = frame.cpu().numpy().reshape(cam.image_height, W, 3)
        r.close()
    (s0, q0, _), (s1, q1, _) = out[N.RT_PREC_F32]
    assert np.isfinite(s0).all() and np.array_equal(s0, s1)
    assert s0.max() > spp, "test scene must push radiance above 1"
    assert np.allclose(split, s0, rtol=1e-5, atol=0)
    ref = out[N.RT_PREC_F64][0][0]
    rel = np.abs(s0.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    assert np.quantile(rel, 0.9) < 1e-4, float(np.quantile(rel, 0.9))


@pytest.mark.parametrize("front", [-1, 1, 3, 16])
def test_front_spheres_fp64_bit_exact(front):
    """Spheres taken out of the BVH into the front list (tested first by every ray) leave
    the fp64 frame and the world.hit counts bit-identical: the closest hit does not depend
    on the order in which spheres are tested."""
    arrays = arrays_for("random")
    cam = native_camera(96, 3)
    out = []
    for f in (0, front):
        with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
            r.set_tuning(front_spheres=f)
            r.upload_scene(*arrays)
            out.append(r.render_frame(cam, 3, 50))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])


# ---- negative radii (hollow spheres) and material parameters at their edges ---------------
# One frame for all of it: main.cpp's camera at 96 x 54, 16 spp, depth 50.  (The oracle's own
# sensitivity to fp32-level input error, scene coordinates rounded to fp32 against unrounded:
# plain, NEG and SHELL stay at max 1 LSB and >= 99.98 % exact at this frame; at 160 x 90 x 8 spp
# single diverged paths reach 6 LSB on SHELL -- hence this frame and no other.)
EDGE_W, EDGE_SPP = 96, 16
_EDGE = {}
_EDGE_ORACLE = {}


def material_edge_arrays(fuzz3: float = 3.0):
    """A ground and nine R = 0.5 spheres on x, z in {-1.2, 0, 1.2}, every centre coordinate
    moved by 0.013 (none exact in fp32), with raw material records -- not through api.metal,
    which clamps fuzz: lambertian 0 and 1; metal fuzz 0, 1, `fuzz3` (3: the upload's clamp)
    and -0.5 (the reference passes it through); dielectric ir 1, 1 / 1.5 and 2.4."""
    L, Mt, D = N.RT_LAMBERTIAN, N.RT_METAL, N.RT_DIELECTRIC
    mats = [(L, (0.5, 0.5, 0.5), 0.0, 0.0),
            (L, (0.0, 0.0, 0.0), 0.0, 0.0), (L, (1.0, 1.0, 1.0), 0.0, 0.0),
            (Mt, (0.7, 0.6, 0.5), 0.0, 0.0), (Mt, (0.7, 0.6, 0.5), 1.0, 0.0), (Mt, (0.7, 0.6, 0.5), fuzz3, 0.0),
            (Mt, (0.9, 0.9, 0.9), -0.5, 0.0),
            (D, (0.0, 0.0, 0.0), 0.0, 1.0), (D, (0.0, 0.0, 0.0), 0.0, 1.0 / 1.5), (D, (0.0, 0.0, 0.0), 0.0, 2.4)]
    M = np.zeros(len(mats), dtype=N.MATERIAL_DTYPE)
    for k, (ty, alb, fuzz, ir) in enumerate(mats):
        M[k]["type"], M[k]["albedo"], M[k]["fuzz"], M[k]["ir"] = ty, alb, fuzz, ir
    S = np.zeros(10, dtype=N.SPHERE_DTYPE)
    S[0]["center"], S[0]["radius"], S[0]["mat"] = (0.0, -1000.0, 0.0), 1000.0, 0
    k = 1
    for x in (-1.2, 0.0, 1.2):
        for z in (-1.2, 0.0, 1.2):
            S[k]["center"], S[k]["radius"], S[k]["mat"] = (x, 0.5, z), 0.5, k
            k += 1
    S["center"] += 0.013
    return S, M


def edge_arrays(name: str):
    if name not in _EDGE:
        from test_trace_rays import neg_field, shell_field
        S, M = arrays_for("random")
        _EDGE[name] = {"PLAIN": lambda: (S, M), "NEG": lambda: (neg_field(S), M),
                       "SHELL": lambda: (shell_field(S, M), M), "HOLLOW": lambda: arrays_for("hollow"),
                       "MATERIALS": material_edge_arrays,
                       "MATERIALS_FUZZ1": lambda: material_edge_arrays(fuzz3=1.0)}[name]()
    return _EDGE[name]


def edge_oracle(name: str):
    """The oracle's frame of the scene (sums, 8-bit, segments), rendered once."""
    if name not in _EDGE_ORACLE:
        _EDGE_ORACLE[name] = O.render_counter_full(O.OracleScene.from_arrays(*edge_arrays(name)),
                                                   O.camera(EDGE_W, EDGE_SPP), SEED)
    return _EDGE_ORACLE[name]


def edge_frame(prec, name, **tuning):
    """-> ((sums, rgb, segs), scene_info) of the scene's frame under a tuning."""
    r = N.Renderer(0, SEED, prec)
    try:
        if tuning:
            r.set_tuning(**tuning)
        r.upload_scene(*edge_arrays(name))
        info = r.scene_info()
        return r.render_frame(native_camera(EDGE_W, EDGE_SPP), EDGE_SPP, 50), info
    finally:
        r.close()


F32_EDGE_TUNINGS = [{}, dict(traversal=N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID), dict(block=512, traversal=8),
                    dict(front_spheres=0)]


_OTHER_PATH = {}


def f32_other_path_share(name, frame=None) -> float:
    """The share of the frame's pixels whose fp32 world.hit count differs from the oracle's:
    some sample of them took another path (default tuning)."""
    if name not in _OTHER_PATH:
        segs = (frame or edge_frame(N.RT_PREC_F32, name)[0])[2]
        _OTHER_PATH[name] = float((segs.astype(np.int64) != edge_oracle(name)[2].astype(np.int64)).mean())
    return _OTHER_PATH[name]


# Scenes on which single samples that fp32 sends down another path (a ray on the other side
# of a glass shell 0.04 thick) move a pixel past F32_MAX_LSB; there the bound holds for the
# pixels on the oracle's path, and the share of the others is bounded by the plain field's.
F32_DIVERGED_PATHS = {"SHELL"}


def assert_f32_edge_frame(name):
    """The four tunings -- default, grid off, one path per lane, no front list -- render one
    frame, sums and segments; the default frame within the F32_* constants of the oracle's.

    Every pixel whose world.hit count equals the oracle's (all of its samples on the oracle's
    path) is within F32_MAX_LSB, and the share of the other pixels is at most twice the share
    the same kernel shows on the plain random field at this frame (the oracle alone, fed
    coordinates rounded to fp32, puts 0.17 % of SHELL's pixels on another path against 0.10 %
    of the plain field's: a ratio of 1.7).  Measured on MI355X, pixels on another path: plain
    0.50 %, NEG 0.48 %, SHELL 0.69 %, HOLLOW 0.02 %, MATERIALS 0.10 %; max LSB over all pixels 1
    everywhere but SHELL, where one diverged sample of 16 moves a pixel by 4 (F32_DIVERGED_PATHS;
    its same-path pixels: 1)."""
    frames = [edge_frame(N.RT_PREC_F32, name, **t)[0] for t in F32_EDGE_TUNINGS]
    for k, f in enumerate(frames[1:], 1):
        assert np.array_equal(f[2], frames[0][2]), (name, F32_EDGE_TUNINGS[k])
        assert np.array_equal(f[0], frames[0][0]), (name, F32_EDGE_TUNINGS[k])
    sums, rgb, segs = frames[0]
    _, rgb_o, segs_o = edge_oracle(name)
    st = f32_stats(rgb, rgb_o)
    same = segs.astype(np.int64) == segs_o.astype(np.int64)
    d = np.abs(rgb.astype(np.int64) - rgb_o.astype(np.int64)).max(axis=2)
    other, plain = f32_other_path_share(name, frames[0]), f32_other_path_share("PLAIN")
    print(name, json.dumps(st), "pixels on another path", other, "on the plain field", plain,
          "max LSB on the same path", int(d[same].max()))
    assert np.isfinite(sums).all()
    assert d[same].max() <= F32_MAX_LSB
    assert other <= 2 * plain
    if name not in F32_DIVERGED_PATHS:
        assert st["max"] <= F32_MAX_LSB
    assert st["exact"] >= F32_EXACT_FRAC
    assert st["mean_abs"] <= F32_MEAN_LSB
    assert abs(st["bias"]) <= F32_BIAS_LSB


@pytest.mark.parametrize("kernel", [0, 3, 4, 5, "5-3d"])
@pytest.mark.parametrize("scene", ["NEG", "SHELL", "HOLLOW"])
def test_f64_negative_radius_frames_bit_exact(scene, kernel):
    """fp64 frames of the scenes with negative radii -- the field with a third of its radii
    negated, the field with a shell of -0.8 r inside every glass sphere, the ten spheres of the
    reference-made hollow golden -- equal the oracle's bit for bit, sums, 8-bit values and
    world.hit counts, under every fp64 kernel; on the two fields the default and kernel 5
    walk the sphere grid, kernels 3 and 4 the tree (whose boxes must hold |r|)."""
    tuning = dict(f64_kernel=5, traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D) if kernel == "5-3d" else \
        dict(f64_kernel=kernel) if kernel else {}
    (sums, rgb, segs), info = edge_frame(N.RT_PREC_F64, scene, **tuning)
    if scene != "HOLLOW":
        assert bool(info.render_traversal & N.RT_TRAV_GRID) == (kernel not in (3, 4)), (scene, kernel)
    sums_o, rgb_o, segs_o = edge_oracle(scene)
    assert np.isfinite(sums_o).all()
    assert np.array_equal(segs, segs_o.astype(np.uint32)), "path structure differs"
    assert np.array_equal(sums, sums_o)
    assert np.array_equal(rgb, rgb_o)


@pytest.mark.parametrize("scene", ["NEG", "SHELL", "HOLLOW"])
def test_f32_negative_radius_frames(scene):
    """fp32 frames of the same scenes: one frame whatever walks them (grid, tree, one path per
    lane, no front list), within the F32_* constants of the oracle's."""
    assert_f32_edge_frame(scene)


def test_material_edges_f64_bit_exact():
    """Material parameters at their edges (material_edge_arrays) in fp64: the oracle's frame
    bit for bit, and fuzz 3 uploads as fuzz 1 (material.h:33's clamp, applied by
    rt_upload_scene to the raw record)."""
    (sums, rgb, segs), _ = edge_frame(N.RT_PREC_F64, "MATERIALS")
    sums_o, rgb_o, segs_o = edge_oracle("MATERIALS")
    assert np.isfinite(sums_o).all()
    assert np.array_equal(segs, segs_o.astype(np.uint32)), "path structure differs"
    assert np.array_equal(sums, sums_o) and np.array_equal(rgb, rgb_o)
    (sums1, _, segs1), _ = edge_frame(N.RT_PREC_F64, "MATERIALS_FUZZ1")
    assert np.array_equal(segs1, segs) and np.array_equal(sums1, sums)


def test_material_edges_f32():
    """The same scene in fp32: one frame under the four tunings, within the F32_* constants,
    and fuzz 3 renders the fuzz-1 frame bit for bit."""
    assert_f32_edge_frame("MATERIALS")
    a, _ = edge_frame(N.RT_PREC_F32, "MATERIALS")
    b, _ = edge_frame(N.RT_PREC_F32, "MATERIALS_FUZZ1")
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0])


def test_material_edges_trace_tape():
    """64 rays into the material-edge scene on explicit tapes against orc_trace_tape; about a
    tenth of the tape entries are exactly 0.0 or 1 - 2^-53, the ends of random_double()'s
    range (not constant tapes: random_in_unit_sphere's rejection loop would never accept)."""
    rng = np.random.default_rng(5)
    S, M = edge_arrays("MATERIALS")
    sc = O.OracleScene.from_arrays(S, M)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
        r.upload_scene(S, M)
        bounced = 0
        for _ in range(64):
            o = rng.uniform(-3, 3, 3) + [0, 2.5, 0]
            target = rng.uniform([-1.5, 0.2, -1.5], [1.5, 0.8, 1.5])
            ray = [*o, *(target - o), rng.uniform()]
            tape = rng.uniform(size=2000)   # (long enough: 50 bounces never exhaust it)
            edge = rng.uniform(size=2000)
            tape[edge < 0.05] = 0.0
            tape[edge > 0.95] = 1.0 - 2.0 ** -53
            col, used = r.trace_tape(ray, 50, tape)
            out, used_o = O.trace_tape(sc, ray, 50, tape)
            assert used == used_o and used <= 2000 and list(col) == out
            bounced += used > 0
    assert bounced >= 48   # (the rays do meet the spheres)
