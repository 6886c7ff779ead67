"""Resumable flat grid walks (r07, RT_GRID_SUSPEND): suspending and resuming a lane's walk
through the sphere grid never changes a bit of the frame.  Needs an MI355X.

The fp32 sphere-only kernel over the flat grid walk may stop the walks of a wave's last few
lanes between blocks of iterations and resume them in the next trace (rt_device.h closest_hit,
SUSP).  Float sums and per-pixel world.hit counts must be those of every other setting and of
the sphere tree (traversal 600), bit for bit; DIAG slot 31 counts the suspensions."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
TREE = 600                       # the sphere tree's coherent kernel
SETTINGS = ["0", None, "16,8", "64,1"]   # (None: the variable unset, the default)
IMAGES = {"64x64": (64, 64), "13x5": (13, 5)}
SPP, DEPTH = 4, 50


@contextmanager
def grid_suspend(value):
    """RT_GRID_SUSPEND as rt_create reads it (None: unset)."""
    old = os.environ.pop("RT_GRID_SUSPEND", None)
    if value is not None:
        os.environ["RT_GRID_SUSPEND"] = value
    try:
        yield
    finally:
        os.environ.pop("RT_GRID_SUSPEND", None)
        if old is not None:
            os.environ["RT_GRID_SUSPEND"] = old


_ARRAYS = {}


def random_arrays(ground=True):
    if "random" not in _ARRAYS:
        rtweekend.reset_stream()
        _ARRAYS["random"] = api.flatten(scenes.random_spheres())
    S, M = _ARRAYS["random"]
    return (S, M) if ground else (S[S["radius"] < 64].copy(), M)


def camera(image):
    W, H = IMAGES[image]
    cam = scenes.main_camera()
    cam.image_width, cam.samples_per_pixel, cam.max_depth = W, SPP, DEPTH
    c = cam.native
    c.image_height = H
    return c


def render(setting, cam, arrays=None, diag=False, **tuning):
    """(sums, segments[, suspensions]) of one fresh context created under `setting`."""
    with grid_suspend(setting):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        if tuning:
            r.set_tuning(**tuning)
        r.upload_scene(*(arrays or random_arrays()))
        sums, _, segs = r.render_frame(cam, SPP, DEPTH)
        if not diag:
            return sums, segs
        return sums, segs, r.render_diag(cam, SPP, DEPTH)["grid_suspensions"], r.scene_info()
    finally:
        r.close()


_TREE = {}


def tree_frame(image):
    """The sphere tree's frame of `image`, rendered once."""
    if image not in _TREE:
        _TREE[image] = render("0", camera(image), traversal=TREE)
    return _TREE[image]


@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("setting", SETTINGS)
def test_suspension_never_changes_the_frame(setting, image):
    """Every setting renders the tree's frame (and so each other's), sums and segment counts
    bit for bit; the walks are suspended where the setting says so."""
    sums, segs, n_susp, info = render(setting, camera(image), diag=True)
    assert info.render_traversal & N.RT_TRAV_GFLAT
    ref_sums, ref_segs = tree_frame(image)
    assert np.array_equal(segs, ref_segs)
    assert np.array_equal(sums, ref_sums)
    print(setting, image, "suspensions", n_susp)
    if setting == "0":
        assert n_susp == 0
    elif image == "64x64" and setting is not None:
        assert n_susp > 0


def test_drain_with_suspended_lanes():
    """One workgroup renders the whole frame, so its waves drain the queue while lanes are
    suspended: the same frame."""
    sums, segs, n_susp, _ = render("64,1", camera("64x64"), diag=True, grid_workgroups=1)
    ref_sums, ref_segs = tree_frame("64x64")
    assert n_susp > 0
    assert np.array_equal(segs, ref_segs) and np.array_equal(sums, ref_sums)


def test_other_kernels_never_suspend():
    """A grid taller than one cell (the 3-D walk) and a scene with a mesh (the mixed-scene
    kernel) count no suspension, whatever the setting."""
    from test_mesh import mesh_arrays
    S, M = random_arrays()
    tall = S.copy()
    tall["center"][:, 1] *= 20.0
    tall["center_vec"][:, 1] *= 20.0
    _, _, n_tall, info = render("64,1", camera("64x64"), arrays=(tall, M), diag=True)
    assert info.render_traversal & N.RT_TRAV_GRID and not info.render_traversal & N.RT_TRAV_GFLAT
    assert n_tall == 0
    _, _, n_mixed, info = render("64,1", camera("64x64"), arrays=mesh_arrays("mixed"), diag=True)
    assert info.num_triangles > 0 and info.render_traversal & N.RT_TRAV_GFLAT
    assert n_mixed == 0


def test_far_camera_within_reach():
    """The field without its ground seen from 150 units away (within the grid's reach): rays
    enter the grid far from their origin; the tree's frame."""
    look = np.array((13.0, 2.0, 3.0))
    cam = scenes.main_camera()
    cam.image_width, cam.samples_per_pixel, cam.max_depth = 64, SPP, DEPTH
    cam.lookfrom = tuple(look / np.linalg.norm(look) * 150.0)
    cam.vfov, cam.defocus_angle, cam.focus_dist = float(np.degrees(2 * np.arctan(3.0 / 150.0))), 0.0, 150.0
    arrays = random_arrays(ground=False)
    sums, segs, n_susp, info = render("64,1", cam.native, arrays=arrays, diag=True)
    assert info.render_traversal & N.RT_TRAV_GFLAT and n_susp > 0
    ref_sums, ref_segs = render("0", cam.native, arrays=arrays, traversal=TREE)
    assert np.array_equal(segs, ref_segs) and np.array_equal(sums, ref_sums)


def test_shard_equals_its_tiles_of_the_frame():
    """Shard 3 of 8 holds the whole frame's tiles 3, 11, 19, ...: the same values."""
    import torch
    cam = camera("64x64")
    W, H = IMAGES["64x64"]
    with grid_suspend("64,1"):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        r.upload_scene(*random_arrays())
        whole_l, part_l = N.shard_layout(W, H, 0, 1), N.shard_layout(W, H, 3, 8)
        whole = torch.zeros(whole_l.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
        part = torch.zeros(part_l.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render(cam, SPP, DEPTH, 0, 1, whole.data_ptr())
        r.render(cam, SPP, DEPTH, 3, 8, part.data_ptr())
        r.last_kernel_ms()   # (waits for the renderer's stream)
        torch.cuda.synchronize()
        n = part_l.shard_tiles
        assert n == len(range(3, whole_l.shard_tiles, 8)) and n > 0
        w = whole.cpu().numpy().reshape(-1, 64 * 3)[3:whole_l.shard_tiles:8]
        assert np.array_equal(part.cpu().numpy().reshape(-1, 64 * 3)[:n], w)
    finally:
        r.close()
