"""The frame kernels' tables (csrc/rt_launch.h RenderKernel; rt_render_f32.hip, rt_render_f64.hip):
every fp32 sphere key of the table is accepted by rt_set_tuning, is what the plan resolves to and
renders; the fp64 kernels render one frame; keys outside the tables are refused on the host,
before any launch.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
G3D = 262144   # RT_TRAV_G3D: keep the 3-D walk on a grid one cell tall in y (tuning only, in no key)
# (block, waves_per_eu, the traversal asked for, the key the plan resolves to) on the four-sphere
# scene, whose grid is one cell tall in y: the flat walk's keys are what 66136 / 66264 become
# there, and the 3-D walk's need G3D.
F32_SPHERE_KEYS = [(1024, 8, 600, 600), (1024, 8, 728, 728), (1024, 8, 88, 88), (1024, 8, 216, 216), (512, 8, 8, 8),
                   (1024, 8, 66136 | G3D, 66136), (1024, 8, 66264 | G3D, 66264),
                   (1024, 8, 197208, 197208), (1024, 8, 197336, 197336),
                   (1024, 8, 66136, 197208), (1024, 8, 66264, 197336)]


@pytest.fixture(scope="module")
def four():
    return api.flatten(scenes.four_spheres())


def camera_64x48():
    cam = scenes.main_camera()
    cam.aspect_ratio, cam.image_width, cam.samples_per_pixel, cam.max_depth = 4.0 / 3.0, 64, 2, 4
    cam = cam.native
    assert (cam.image_width, cam.image_height) == (64, 48)
    return cam


def test_named_keys_are_the_numbers():
    """The numbers above, spelled with the public flags as the table spells them."""
    d = N.RT_TRAV_SELROOT | N.RT_TRAV_B128 | N.RT_TRAV_COH | N.RT_TRAV_CULL
    assert (d, d | N.RT_TRAV_NOSUM, d & ~N.RT_TRAV_CULL, (d | N.RT_TRAV_NOSUM) & ~N.RT_TRAV_CULL,
            N.RT_TRAV_SELROOT) == (600, 728, 88, 216, 8)
    g = d | N.RT_TRAV_GRID
    assert (g, g | N.RT_TRAV_NOSUM, g | N.RT_TRAV_GFLAT, g | N.RT_TRAV_NOSUM | N.RT_TRAV_GFLAT) == \
        (66136, 66264, 197208, 197336)
    assert N.RT_TRAV_G3D == G3D and N.RT_TRAV_DEFAULT == 66136


@pytest.mark.parametrize("block,wpe,ask,key", F32_SPHERE_KEYS)
def test_f32_sphere_key_is_planned_and_renders(four, block, wpe, ask, key):
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        t = r.tuning()
        assert t.sphere_grid_density > 0
        t.block, t.waves_per_eu, t.traversal = block, wpe, ask
        assert r._L.rt_set_tuning(r.ctx, C.byref(t)) == N.RT_OK
        r.upload_scene(*four)
        info = r.scene_info()
        if key & N.RT_TRAV_GRID:
            assert min(info.grid_res) >= 1 and info.grid_res[1] == 1
        assert (info.render_block, info.render_waves_per_eu, info.render_traversal) == (block, wpe, key)
        cam = camera_64x48()
        sums = np.empty((48, 64, 3), np.float32)
        rgb = np.empty((48, 64, 3), np.int32)
        assert r._L.rt_render_frame(r.ctx, C.byref(cam), 2, 4, N._ptr(sums), N._ptr(rgb), None) == N.RT_OK
        assert np.isfinite(sums).all() and sums.max() > 0
        assert r.scene_info().render_traversal == key


def test_f64_kernels_render_one_frame(four):
    """f64_kernel 3, 4 and 5 (on this grid the flat walk, kernel 6; with G3D kernel 5 itself): the
    same frame bit for bit."""
    frames = []
    for kernel, trav in ((3, N.RT_TRAV_DEFAULT), (4, N.RT_TRAV_DEFAULT), (5, N.RT_TRAV_DEFAULT),
                         (5, N.RT_TRAV_DEFAULT | G3D)):
        with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
            r.set_tuning(f64_kernel=kernel, traversal=trav)
            r.upload_scene(*four)
            assert r.scene_info().grid_res[1] == 1
            sums, _, segs = r.render_frame(camera_64x48(), 2, 4)
            assert np.isfinite(sums).all() and sums.max() > 0
            frames.append((sums, segs))
    for sums, segs in frames[1:]:
        assert np.array_equal(sums.view(np.uint64), frames[0][0].view(np.uint64))
        assert np.array_equal(segs, frames[0][1])


@pytest.mark.parametrize("bad", [dict(block=448), dict(waves_per_eu=4, traversal=600), dict(f64_kernel=6),
                                 dict(f64_kernel=7)])
@pytest.mark.parametrize("precision", [N.RT_PREC_F32, N.RT_PREC_F64])
def test_keys_outside_the_tables_are_refused(precision, bad):
    """Refused by rt_set_tuning with RT_ERR_INVALID -- nothing is uploaded or launched -- and the
    tuning stays what it was."""
    with N.Renderer(0, SEED, precision) as r:
        before = bytes(r.tuning())
        t = r.tuning()
        for k, v in bad.items():
            setattr(t, k, v)
        assert r._L.rt_set_tuning(r.ctx, C.byref(t)) == N.RT_ERR_INVALID
        assert bytes(r.tuning()) == before
