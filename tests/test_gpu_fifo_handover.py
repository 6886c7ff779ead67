"""The FIFO hand-over of the fp32 sphere-grid kernels (r13): a queued primary hit is a 16-byte
entry {t, pix, sid, rng0} whose rng0 is the path's RNG state right after CounterRng::start as
the batch computed it; the lane that pops the entry sets that state instead of hashing pixel
and sample again, and rebuilds the batch's camera ray from it.  Needs an MI355X.

The reference has no FIFO at all: the one-path-per-lane kernel (render_lanes), i.e. the
traversal without RT_TRAV_COH -- instantiated as block 512, traversal 8, which every coherent
kernel is tested against (its frame is bit-identical to the coherent kernels').
Float sums and per-pixel segment counts of the default coherent grid kernel must equal it bit
for bit in every case below.

The launch shape is that of tests/test_gpu_batch_adopt.py and for the same reason: a resident
launch on this small image adopts every hit and never pushes or pops, so the cases run on two
workgroups (32 waves for 91 tiles) with item_balance 0 (items of 32 and 8 samples); the bottom
tile row lies half outside the image.  test_the_cases_use_the_fifo checks with the
instrumented build that entries are pushed, popped and wrapped around."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes

pytestmark = pytest.mark.gpu

SEED = 0x5EED
W, H, SPP = 104, 52, 40
FEW = dict(grid_workgroups=2, item_balance=0.0)
LANES = dict(block=512, traversal=8)   # the reference: render_lanes, no RT_TRAV_COH
FIFO_ENTRIES = 128                     # rt_device.h COH_FIFO
SWITCHES = ("RT_BATCH_ADOPT", "RT_GRID_SUSPEND", "RT_BATCH_CULL")


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


CAMERAS = {
    "main": {},
    "defocus0": {"defocus_angle": 0.0},
    # pitched up: most of the image sees only sky (batches without a hit, several batches inside
    # one pop loop), the bottom rows the far field
    "sky": {"lookat": (0.0, 3.5, 0.0)},
    "inside120": {"vfov": 120.0, "lookfrom": (0.5, 0.4, 0.6), "lookat": (4.0, 0.3, -2.0), "focus_dist": 3.0},
}


def camera(name="main"):
    cam = scenes.main_camera()
    cam.image_width, cam.aspect_ratio, cam.samples_per_pixel = W, W / H, SPP
    for k, v in CAMERAS[name].items():
        setattr(cam, k, v)
    c = cam.native
    assert (c.image_width, c.image_height) == (W, H)
    return c


def renderer(env=None, **tuning):
    """A context created with the switches as given (the others unset) and the tuning as given."""
    with environment(**{**dict.fromkeys(SWITCHES), **(env or {})}):
        r = N.Renderer(0, SEED, N.RT_PREC_F32)
    r.set_tuning(**tuning)
    return r


def check_plan(r):
    """The coherent grid kernel at two 1,024-thread workgroups per CU (<= 80 KB of LDS each)."""
    i = r.scene_info()
    assert i.render_block == 1024 and i.render_waves_per_eu == 8, (i.render_block, i.render_waves_per_eu)
    assert i.render_traversal & N.RT_TRAV_GRID and i.render_traversal & N.RT_TRAV_COH, i.render_traversal
    assert 0 < i.lds_bytes <= 81920, i.lds_bytes


def frame(cam, scene, depth, env=None, coherent=True, **tuning):
    """(sums, segments) of a whole frame: the coherent grid kernel on the FEW shape, or the reference."""
    r = renderer(env, **({**FEW, **tuning} if coherent else LANES))
    try:
        r.upload_scene(*arrays(scene))
        sums, _, segs = r.render_frame(camera(cam), SPP, depth)
        if coherent:
            check_plan(r)
        else:
            assert not r.scene_info().render_traversal & N.RT_TRAV_COH
        return sums, segs
    finally:
        r.close()


_REF = {}


def reference(cam="main", scene="random", depth=50):
    """The FIFO-less frame of a case, rendered once and never written to."""
    key = (cam, scene, depth)
    if key not in _REF:
        sums, segs = frame(cam, scene, depth, coherent=False)
        sums.setflags(write=False)
        segs.setflags(write=False)
        _REF[key] = (sums, segs)
    return _REF[key]


def assert_equal(got, ref, traced=True):
    assert (ref[1].sum() > 0) == traced
    assert np.array_equal(got[1], ref[1])
    assert got[0].dtype == ref[0].dtype and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


@pytest.mark.parametrize("depth", [50, 1, 0])
def test_main_camera(depth):
    """Depth 50; depth 1 (batches and one shade pass: the hand-over is the whole frame); depth 0
    (no camera ray is traced, every sample is 0)."""
    assert_equal(frame("main", "random", depth), reference(depth=depth), traced=depth > 0)


@pytest.mark.parametrize("cam", ["defocus0", "sky", "inside120"])
def test_other_cameras(cam):
    """No defocus disk (no rejected-candidate field in play), the sky-pitched camera, 120 degrees
    from inside the field."""
    assert_equal(frame(cam, "random", 50), reference(cam=cam))


def test_hollow_glass():
    assert_equal(frame("main", "hollow", 50), reference(scene="hollow"))


def test_one_workgroup():
    """16 waves for 182 items: the drain, a dry queue with a non-empty FIFO."""
    assert_equal(frame("main", "random", 50, grid_workgroups=1), reference())


@pytest.mark.parametrize("env", [{"RT_BATCH_ADOPT": "0"}, {"RT_GRID_SUSPEND": "64,1"}, {"RT_BATCH_CULL": "0"}],
                         ids=["adopt_off", "suspend_64_1", "cull_off"])
def test_switches(env):
    """RT_BATCH_ADOPT=0: every primary hit takes the 16-byte entry, the heaviest FIFO traffic,
    wrap-around of the 128 entries included.  RT_GRID_SUSPEND=64,1: suspended lanes beside
    popping lanes.  RT_BATCH_CULL=0: the walking batch feeds the same FIFO."""
    assert_equal(frame("main", "random", 50, env=env), reference())


def _device_frames(coherent, body):
    import torch
    r = renderer(**(FEW if coherent else LANES))
    try:
        r.upload_scene(*arrays("random"))
        out = body(r, torch)
        r.last_kernel_ms()   # (waits for the renderer's stream)
        torch.cuda.synchronize()
        if coherent:
            check_plan(r)
        return [t.cpu().numpy() for t in out]
    finally:
        r.close()


def _buffers(torch, lay):
    sums = torch.zeros(lay.max_shard_tiles * 64 * 3, dtype=torch.float32, device="cuda")
    segs = torch.zeros(lay.max_shard_tiles * 64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return sums, segs


def test_shard_one_of_three():
    """The pop's tile decode with nshards > 1."""
    cam = camera()
    lay = N.shard_layout(W, H, 1, 3)

    def body(r, torch):
        sums, segs = _buffers(torch, lay)
        r.render(cam, SPP, 50, 1, 3, sums.data_ptr(), segs.data_ptr())
        return sums, segs

    ref = _device_frames(False, body)
    got = _device_frames(True, body)
    assert ref[1].sum() > 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


def test_two_sample_ranges_equal_one_launch():
    """Samples 0-23 and 24-39 accumulated: sample_begin != 0 goes into rng0's sample word."""
    cam = camera()
    lay = N.shard_layout(W, H, 0, 1)

    def launch(ranges):
        def body(r, torch):
            sums, segs = _buffers(torch, lay)
            for k, (b, n) in enumerate(ranges):
                r.render_range(cam, b, n, 50, 0, 1, k > 0, sums.data_ptr(), segs.data_ptr())
            return sums, segs
        return body

    ref = _device_frames(False, launch([(0, SPP)]))
    got = _device_frames(True, launch([(0, 24), (24, SPP - 24)]))
    assert ref[1].sum() > 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


def _diag(cam, env=None):
    r = renderer(env, **FEW)
    try:
        r.upload_scene(*arrays("random"))
        d = r.render_diag(camera(cam), SPP, 50)
        check_plan(r)
        return d
    finally:
        r.close()


def test_the_cases_use_the_fifo():
    """Instrumented: the main case, RT_BATCH_ADOPT=0 and the sky camera push and pop entries;
    with adoption off a wave pops more hits than its FIFO has entries (the ring wrapped); the
    pop-pass histogram (slots 32-39) sums to the pop-pass counter (slot 27)."""
    for what, cam, env in (("main", "main", None), ("adopt_off", "main", {"RT_BATCH_ADOPT": "0"}),
                           ("sky", "sky", None)):
        d = _diag(cam, env)
        hist = d["pop_pass_hist"] + d["pop_pass_hist_after_adopt"]
        print(f"{what}: popped {d['x15']} adopted {d['hits_adopted']} pop passes {d['pop_passes']} waves {d['waves']} "
              f"histogram 1-2/3-6/7-16/17-64 other {d['pop_pass_hist']} after an adopting batch "
              f"{d['pop_pass_hist_after_adopt']}")
        assert d["x15"] > 0 and d["pop_passes"] > 0
        assert d["pop_lanes"] == d["x15"]
        assert sum(hist) == d["pop_passes"]
        assert d["flushes"] == W * H * SPP
        if what == "adopt_off":
            assert d["hits_adopted"] == 0 and sum(d["pop_pass_hist_after_adopt"]) == 0
            # (the mean over the waves: some wave popped more than the ring holds)
            assert d["x15"] > FIFO_ENTRIES * d["waves"]
        else:
            assert d["hits_adopted"] > 0
