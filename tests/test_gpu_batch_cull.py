"""Per-item candidate lists (r09, RT_BATCH_CULL): tracing a tile's camera-ray batches against
the spheres its beam can reach (csrc/rt_batch_cull.h) instead of walking the sphere grid never
changes a bit of the frame.  Needs an MI355X.

Float sums and per-pixel world.hit counts of RT_BATCH_CULL=0 (every batch walks, the kernel of
before), of the default (lists of up to 24 spheres) and of RT_BATCH_CULL=2 (most items overflow
their list and walk) must be equal bit for bit, in every case below."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SETTINGS = ["0", None, "2"]   # (None: the variable unset, the default)
W, H, SPP = 104, 52, 40       # 13 x 7 tiles, the bottom row half outside; items of 32 and fewer samples


@contextmanager
def environment(**kv):
    """Variables as rt_create reads them (None: unset)."""
    old = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_ARRAYS = {}


def arrays(name):
    if name not in _ARRAYS:
        rtweekend.reset_stream()
        _ARRAYS[name] = api.flatten({"random": scenes.random_spheres, "hollow": scenes.hollow_glass}[name]())
    return _ARRAYS[name]


def camera(**fields):
    cam = scenes.main_camera()
    cam.image_width, cam.aspect_ratio, cam.samples_per_pixel = W, W / H, SPP
    for k, v in fields.items():
        setattr(cam, k, v)
    c = cam.native
    assert (c.image_width, c.image_height) == (W, H)
    return c


def renderer(setting, suspend=None, **tuning):
    with environment(RT_BATCH_CULL=setting, RT_GRID_SUSPEND=suspend):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    if tuning:
        r.set_tuning(**tuning)
    return r


def frames(cam, scene="random", depth=50, suspend=None, want_grid=True, **tuning):
    """[(sums, segments, plan)] per setting."""
    out = []
    for setting in SETTINGS:
        r = renderer(setting, suspend, **tuning)
        try:
            r.upload_scene(*arrays(scene))
            sums, _, segs = r.render_frame(cam, SPP, depth)
            i = r.scene_info()
            assert bool(i.render_traversal & N.RT_TRAV_GRID) == want_grid
            out.append((sums, segs, (i.render_block, i.render_traversal, i.render_waves_per_eu, i.lds_bytes)))
        finally:
            r.close()
    return out


def assert_equal(fr):
    (s0, g0, p0) = fr[0]
    assert g0.sum() > 0
    for setting, (s, g, p) in zip(SETTINGS[1:], fr[1:]):
        assert p == p0, (setting, p, p0)
        assert np.array_equal(g, g0), setting
        assert np.array_equal(s, s0), setting


CAMERAS = {
    "main": {},
    "defocus0": {"defocus_angle": 0.0},
    "inside120": {"vfov": 120.0, "lookfrom": (0.5, 0.4, 0.6), "lookat": (4.0, 0.3, -2.0), "focus_dist": 3.0},
}


@pytest.mark.parametrize("cam", list(CAMERAS))
def test_lists_never_change_the_frame(cam):
    assert_equal(frames(camera(**CAMERAS[cam])))


def test_depth_one():
    """Batches, pops and one shade pass: nothing but camera rays is traced."""
    assert_equal(frames(camera(), depth=1))


def test_hollow_glass():
    """Negative radii, a moving shell, spheres inside spheres."""
    assert_equal(frames(camera(), scene="hollow"))


@pytest.mark.parametrize("how", ["one_workgroup", "no_suspension", "walk_3d"])
def test_other_launch_shapes(how):
    kw = {"one_workgroup": dict(grid_workgroups=1), "no_suspension": dict(suspend="0"),
          "walk_3d": dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D)}[how]
    fr = frames(camera(), **kw)
    assert_equal(fr)
    assert bool(fr[0][2][1] & N.RT_TRAV_GFLAT) == (how != "walk_3d")


def test_tree_kernel_is_untouched():
    """The sphere tree's kernel has no lists: the same frame under every setting, and its plan
    (block, kernel, register budget, LDS bytes) does not move."""
    fr = frames(camera(), want_grid=False, traversal=600)
    assert_equal(fr)
    assert fr[0][2][:3] == (1024, 600, 8)
    grid = frames(camera())
    # (the lists cost the grid kernels 128 B per wave, whatever the setting)
    assert all(p[2][3] == grid[0][2][3] for p in grid)
    assert np.array_equal(grid[1][0], fr[0][0]) and np.array_equal(grid[1][1], fr[0][1])


def test_lists_are_used():
    """DIAG: the batches' sphere tests and cell steps per frame (slot 13: the batch trace's
    iterations) drop with the lists on; with a cap of 2 no more than with them off (at this
    image size every tile's beam reaches more than two spheres: every item walks)."""
    its = []
    for setting in SETTINGS:
        r = renderer(setting)
        try:
            r.upload_scene(*arrays("random"))
            its.append(r.render_diag(camera(), SPP, 50)["k_it2"])
        finally:
            r.close()
    print("batch trace iterations (off, default, cap 2):", its)
    assert its[1] < its[2] <= its[0]


def _device_frames(setting, body):
    import torch
    r = renderer(setting)
    try:
        r.upload_scene(*arrays("random"))
        out = body(r, torch)
        r.last_kernel_ms()   # (waits for the renderer's stream)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]
    finally:
        r.close()


def test_shard_one_of_three():
    cam = camera()
    lay = N.shard_layout(W, H, 1, 3)

    def body(r, torch):
        sums = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
        segs = torch.zeros(lay.max_shard_tiles * 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render(cam, SPP, 50, 1, 3, sums.data_ptr(), segs.data_ptr())
        return sums, segs

    ref = _device_frames("0", body)
    assert ref[1].sum() > 0
    for setting in SETTINGS[1:]:
        got = _device_frames(setting, body)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), setting


def test_two_sample_ranges_equal_one_launch():
    cam = camera()
    lay = N.shard_layout(W, H, 0, 1)

    def launch(ranges):
        def body(r, torch):
            sums = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
            segs = torch.zeros(lay.max_shard_tiles * 64, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for k, (b, n) in enumerate(ranges):
                r.render_range(cam, b, n, 50, 0, 1, k > 0, sums.data_ptr(), segs.data_ptr())
            return sums, segs
        return body

    ref = _device_frames("0", launch([(0, SPP)]))
    for setting in SETTINGS:
        got = _device_frames(setting, launch([(0, 13), (13, SPP - 13)]))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), setting
