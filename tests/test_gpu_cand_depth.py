"""The depth-ordered candidate loop (r21, rt_device.h RT_CAND_DEPTH): a tile's candidate list
sorted by a near bound of each sphere's roots (csrc/rt_batch_cull.h cull_near), the loop stopping
at the first candidate no lane's closest hit reaches, and ties between equal roots kept with the
lower record -- none of it changes a bit of the frame.  Needs an MI355X.

Float sums and per-pixel segment counts of the default context, of RT_BATCH_CULL=0 (every item
walks the grid: the loop is not run), of a tree context (the kernel without lists) and of
RT_BATCH_CULL=2 (lists longer than the cap: the fallback) must be equal bit for bit, at depth 1
and 50, in every scene below.  64 x 48 pixels at 4 spp: 8 x 6 tiles, one item each."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes
from raytracingproject_amd.api import dielectric, lambertian, metal, sphere

pytestmark = pytest.mark.gpu

SEED = 0x5EED
W, H, SPP = 64, 48, 4
# (name, RT_BATCH_CULL, tuning)
SETTINGS = [("default", None, {}), ("walk", "0", {}), ("tree", None, {"traversal": 600}), ("cap2", "2", {})]


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


def base():
    """scenes.hollow_glass(): the ground and nine spheres, a scene the grid kernels take."""
    return scenes.hollow_glass()


def coincident(order):
    """Two spheres of one centre and radius and different albedo: every root is a tie, and the
    lower record has to win it whichever the sorted list puts first."""
    w = base()
    pair = [sphere((1.5, 0.5, -1.5), 0.5, lambertian((0.9, 0.1, 0.1))), sphere((1.5, 0.5, -1.5), 0.5, lambertian((0.1, 0.1, 0.9)))]
    for s in pair[::order]:
        w.add(s)
    return w


def inside_glass():
    """The camera (13, 2, 3), lens radius 0.05, inside a glass sphere: its near bound is 0."""
    w = base()
    w.add(sphere((13, 2, 3), 0.6, dielectric(1.5)))
    return w


def crossing():
    """A moving sphere passing through a static one over the shutter."""
    w = base()
    w.add(sphere((1.0, 0.4, -2.0), 0.4, metal((0.8, 0.7, 0.3), 0.1)))
    w.add(sphere((1.0, 0.4, -2.9), (1.0, 0.4, -1.1), 0.3, lambertian((0.2, 0.8, 0.3))))
    return w


SCENES = {
    "random_spheres": scenes.random_spheres,
    "four_spheres": scenes.four_spheres,
    "coincident_ab": lambda: coincident(1),
    "coincident_ba": lambda: coincident(-1),
    "inside_glass": inside_glass,
    "crossing": crossing,
    "defocus_off": lambda: coincident(1),
}
CAMERA = {"defocus_off": {"defocus_angle": 0.0}}
# scenes whose default context is known to run a grid kernel (the kernels with lists)
GRID = {"random_spheres", "coincident_ab", "coincident_ba", "inside_glass", "crossing", "defocus_off"}

_ARRAYS = {}


def arrays(name):
    if name not in _ARRAYS:
        rtweekend.reset_stream()
        _ARRAYS[name] = api.flatten(SCENES[name]())
    return _ARRAYS[name]


def camera(**fields):
    cam = scenes.main_camera()
    cam.image_width, cam.aspect_ratio, cam.samples_per_pixel = W, W / H, SPP
    for k, v in fields.items():
        setattr(cam, k, v)
    c = cam.native
    assert (c.image_width, c.image_height) == (W, H)
    return c


def frame(scene, depth, cull, tuning):
    with environment(RT_BATCH_CULL=cull):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    try:
        if tuning:
            r.set_tuning(**tuning)
        r.upload_scene(*arrays(scene))
        sums, _, segs = r.render_frame(camera(**CAMERA.get(scene, {})), SPP, depth)
        return sums, segs, r.scene_info().render_traversal
    finally:
        r.close()


@pytest.mark.parametrize("depth", [1, 50])
@pytest.mark.parametrize("scene", list(SCENES))
def test_frame_is_bit_identical(scene, depth):
    got = {name: frame(scene, depth, cull, tuning) for name, cull, tuning in SETTINGS}
    print(scene, depth, {k: v[2] for k, v in got.items()})
    s0, g0, t0 = got["default"]
    assert g0.sum() > 0
    if scene in GRID:
        assert t0 & N.RT_TRAV_GRID, t0
    assert not got["tree"][2] & N.RT_TRAV_GRID, got["tree"][2]
    for name in ("walk", "tree", "cap2"):
        s, g, _ = got[name]
        assert np.array_equal(g, g0), name
        assert np.array_equal(s, s0), name


def test_coincident_spheres_show_the_lower_record():
    """The two input orders of the coincident pair give different frames (the pair's first sphere
    is the one seen), so the tie is met in this view and decided by the record order."""
    a = frame("coincident_ab", 50, None, {})
    b = frame("coincident_ba", 50, None, {})
    assert np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], b[0])
