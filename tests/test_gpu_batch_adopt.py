"""Adopted batch hits (r10, RT_BATCH_ADOPT): in the fp32 sphere-grid kernels a lane that waits
for a path while its wave traces a batch of camera rays keeps the hit of its own ray instead of
queueing it for some lane to pop and regenerate.  Which lane shades a path never changes a bit
of the frame.  Needs an MI355X.

Float sums and per-pixel world.hit counts of RT_BATCH_ADOPT=0 (every primary hit goes through
the FIFO, the kernel of before) and of the default (adoption on) must be equal bit for bit, and
the launch plan the same, in every case below.

The launch shape matters: a resident launch has more waves than this small image has tiles, so
its items are single samples and each wave traces one batch with all 64 lanes waiting --
everything is adopted, nothing pushed or popped.  The cases therefore run on two workgroups
(32 waves for 91 tiles) with item_balance 0, which gives every tile one item of 32 samples and
one of 8: waves work through several multi-sample items, batches run while
other lanes hold live (or suspended) paths, adopters and pushed hits mix in one batch, leftovers
are popped after an adopting batch, and paths in flight cross item switches.
test_the_cases_run_the_mixed_state checks with the instrumented build that this is so."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SETTINGS = ["0", None]        # (None: the variable unset, the default: on)
W, H, SPP = 104, 52, 40       # 13 x 7 tiles, the bottom row half outside the image (waiting lanes that never hit)
FEW = dict(grid_workgroups=2, item_balance=0.0)   # (the module docstring)


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


def renderer(setting, suspend=None, cull=None, **tuning):
    """A context with the variables as given and the FEW launch shape unless tuning overrides it."""
    with environment(RT_BATCH_ADOPT=setting, RT_GRID_SUSPEND=suspend, RT_BATCH_CULL=cull):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    r.set_tuning(**{**FEW, **tuning})
    return r


def frames(cam, scene="random", depth=50, suspend=None, cull=None, want_grid=True, **tuning):
    """[(sums, segments, plan)] per setting."""
    out = []
    for setting in SETTINGS:
        r = renderer(setting, suspend, cull, **tuning)
        try:
            r.upload_scene(*arrays(scene))
            sums, _, segs = r.render_frame(cam, SPP, depth)
            i = r.scene_info()
            assert bool(i.render_traversal & N.RT_TRAV_GRID) == want_grid
            out.append((sums, segs, (i.render_block, i.render_traversal, i.render_waves_per_eu, i.lds_bytes)))
        finally:
            r.close()
    return out


def diags(cam, scene="random", depth=50, suspend=None, cull=None, **tuning):
    """The instrumented kernel's counters per setting."""
    out = []
    for setting in SETTINGS:
        r = renderer(setting, suspend, cull, **tuning)
        try:
            r.upload_scene(*arrays(scene))
            out.append(r.render_diag(cam, SPP, depth))
        finally:
            r.close()
    return out


def assert_equal(fr, traced=True):
    (s0, g0, p0), (s, g, p) = fr
    assert (g0.sum() > 0) == traced
    assert p == p0, (p, p0)
    assert np.array_equal(g, g0)
    assert np.array_equal(s, s0)


CAMERAS = {
    "main": {},
    "defocus0": {"defocus_angle": 0.0},
    # pitched up: the upper two thirds of the image see only sky (batches without a hit, several
    # batches inside one pop loop), the bottom rows the far field
    "sky": {"lookat": (0.0, 3.5, 0.0)},
    "inside120": {"vfov": 120.0, "lookfrom": (0.5, 0.4, 0.6), "lookat": (4.0, 0.3, -2.0), "focus_dist": 3.0},
}
# launch shapes and settings beside FEW.  one_workgroup: the drain, a dry queue with a non-empty
# FIFO.  Suspended lanes (64,1: every walk suspends after each iteration) hold a path and must
# not adopt.  RT_BATCH_CULL 0 and 2: the batch walks the grid.  walk_3d: the 66136 kernel.
# resident: the default launch (single-sample items, every hit adopted).
SHAPES = {
    "one_workgroup": dict(grid_workgroups=1), "no_suspension": dict(suspend="0"),
    "suspend_64_1": dict(suspend="64,1"), "cull_off": dict(cull="0"), "cull_2": dict(cull="2"),
    "walk_3d": dict(traversal=N.RT_TRAV_DEFAULT | N.RT_TRAV_G3D), "resident": dict(grid_workgroups=0),
}


def test_depth_one():
    """The smallest case: batches and one shade pass.  Every lane waits at the start of every
    round and adopts if its ray hit; lanes that missed make the wave batch again inside the same
    pop loop, where the adopters' next hits are pushed."""
    assert_equal(frames(camera(), depth=1))


@pytest.mark.parametrize("cam", list(CAMERAS))
def test_adoption_never_changes_the_frame(cam):
    assert_equal(frames(camera(**CAMERAS[cam])))


def test_depth_zero():
    """No camera ray is traced: nothing to adopt, every sample is 0."""
    assert_equal(frames(camera(), depth=0), traced=False)


def test_hollow_glass():
    """Negative radii, a moving shell, spheres inside spheres."""
    assert_equal(frames(camera(), scene="hollow"))


@pytest.mark.parametrize("how", list(SHAPES))
def test_other_launch_shapes(how):
    fr = frames(camera(), **SHAPES[how])
    assert_equal(fr)
    assert bool(fr[0][2][1] & N.RT_TRAV_GFLAT) == (how != "walk_3d")


def test_tree_kernel_is_untouched():
    """The sphere tree's kernel adopts nothing: the same frame under both settings, equal to
    the grid kernels', and its plan (block, kernel, register budget) does not move."""
    fr = frames(camera(), want_grid=False, traversal=600)
    assert_equal(fr)
    assert fr[0][2][:3] == (1024, 600, 8)
    grid = frames(camera())
    assert np.array_equal(grid[1][0], fr[0][0]) and np.array_equal(grid[1][1], fr[0][1])
    r = renderer(None, traversal=600)
    try:
        r.upload_scene(*arrays("random"))
        d = r.render_diag(camera(), SPP, 50)
    finally:
        r.close()
    assert d["pop_passes"] is None and d["hits_adopted"] is None   # (no such counters in this kernel)


def test_bad_setting_is_refused():
    for bad in ("2", "on", "01"):
        with pytest.raises(N.RtError):
            renderer(bad).close()


def check_mixed(off, on, what):
    """DIAG of one case, adoption off and on: hits are adopted AND hits are pushed and popped
    with adoption on (the mixed state), what is adopted is exactly what is no longer popped, and
    finished paths (slot 11) and traced segments (slot 10) stay what they were."""
    print(f"{what}: popped, adopted, pop passes, batches, bounce rounds, suspensions "
          f"off {off['x15']} {off['hits_adopted']} {off['pop_passes']} {off['k_it1']} {off['bounce_it']} "
          f"{off['grid_suspensions']} | on {on['x15']} {on['hits_adopted']} {on['pop_passes']} {on['k_it1']} "
          f"{on['bounce_it']} {on['grid_suspensions']}")
    assert off["hits_adopted"] == 0 and on["hits_adopted"] > 0
    assert 0 < on["x15"] < off["x15"]
    assert on["x15"] + on["hits_adopted"] == off["x15"]
    assert on["pop_passes"] > 0
    assert on["pop_lanes"] == on["x15"] and off["pop_lanes"] == off["x15"]
    assert on["flushes"] == off["flushes"] == W * H * SPP
    assert on["segments"] == off["segments"]
    # several batches per wave, and batches beside live paths: more batches than waves, fewer
    # adopted hits than 64 per batch would give
    assert on["k_it1"] > 4 * on["waves"] and on["hits_adopted"] < 64 * on["k_it1"]


def test_hits_are_adopted():
    """The field at depth 50 on the FEW shape."""
    check_mixed(*diags(camera()), "field")


@pytest.mark.parametrize("how", ["one_workgroup", "suspend_64_1", "cull_off", "cull_2", "walk_3d"])
def test_the_cases_run_the_mixed_state(how):
    """The launch shapes above, instrumented: each pushes, pops and adopts in one frame; with
    RT_GRID_SUSPEND=64,1 walks are suspended (lanes that hold a path, not ready, during batches)."""
    off, on = diags(camera(), **SHAPES[how])
    check_mixed(off, on, how)
    if how == "suspend_64_1":
        assert on["grid_suspensions"] > 0 and off["grid_suspensions"] > 0


@pytest.mark.parametrize("case", ["sky", "hollow"])
def test_camera_and_scene_cases_run_the_mixed_state(case):
    kw = dict(cam=camera(**CAMERAS["sky"])) if case == "sky" else dict(cam=camera(), scene="hollow")
    check_mixed(*diags(**kw), case)


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
    """(30 tiles for 32 waves: five items of 8 samples per tile)"""
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
    got = _device_frames(None, body)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


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
