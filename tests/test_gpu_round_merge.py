"""The pop loop of the fp32 sphere-grid kernels after r19: a batch is followed, inside the same
turn of the loop, by the loop's head tests and the pop of the lanes that adopted nothing, so the
path state (pix, RNG state, ray, hit, throughput, scatter count, origin sphere) has one merge
between batch, adoption and pop where it had one per turn.  Needs an MI355X.

The cases are the places where such a merge can go wrong: adopters, pushed hits and sky misses
in one batch with pops right behind it; no adoption at all; every lane or no lane in need of a
path; batches with invalid lanes; paths and FIFO entries that cross item switches; a shard; and
samples that leave [0, 1] beside samples from every finish site.  Reference, launch shape and comparison are those
of tests/test_gpu_round_paths.py (whose reference frames are shared, rendered once): the
one-path-per-lane kernel (block 512, traversal 8), two workgroups with item_balance 0, per-pixel
sums and segment counts equal bit for bit, and in every case the default plan -- block 1024,
8 waves, the coherent grid kernel, at most 80 KB of LDS."""
import pytest

import test_gpu_round_paths as RP
from raytracingproject_amd import _native as N

pytestmark = pytest.mark.gpu

W, H, SPP = RP.W, RP.H, RP.SPP   # 104 x 52 @ 40 spp


def frame(scene="random", depth=50, shape=(W, H, SPP), env=None, **tuning):
    """(sums, segments) of a whole frame of the coherent grid kernel on RP.FEW plus `tuning`."""
    r = RP.renderer(env, **{**RP.FEW, **tuning})
    try:
        r.upload_scene(*RP.arrays(scene))
        sums, _, segs = r.render_frame(RP.camera(*shape), shape[2], depth)
        RP.check_plan(r)
        return sums, segs
    finally:
        r.close()


def test_field_scene():
    """Depth 50: adopters, pushed hits and sky misses mix in one batch, pops follow adopting batches."""
    RP.assert_equal(frame(), RP.reference())


def test_field_scene_without_adoption():
    """RT_BATCH_ADOPT=0: every hit is pushed and every path starts from a pop behind its batch."""
    RP.assert_equal(frame(env={"RT_BATCH_ADOPT": "0"}), RP.reference())


@pytest.mark.parametrize("depth", [1, 0])
def test_every_lane_or_no_lane_needs_a_path(depth):
    """Depth 1: every path ends in its batch or its first shade pass, so every lane needs a path in
    every batch.  Depth 0: no lane is valid, no path starts, the queue runs dry through batches alone."""
    RP.assert_equal(frame(depth=depth), RP.reference(depth=depth), traced=depth > 0)


def test_invalid_lanes_in_edge_tiles():
    """100 x 50 @ 8 spp: lanes of the right and bottom tiles lie outside the image; they neither
    adopt nor push, and stay in need of a path behind every batch of their tile."""
    shape = (100, 50, 8)
    RP.assert_equal(frame(shape=shape), RP.reference(shape=shape))


def test_items_of_eight_samples():
    """item_samples 8 at 40 spp: five items per tile, so paths and FIFO entries cross item switches
    and a popped path is not eligible for the item sums."""
    RP.assert_equal(frame(item_samples=8), RP.reference())


def test_shard_one_of_three():
    cam = RP.camera()
    lay = N.shard_layout(W, H, 1, 3)

    def body(r, torch):
        sums, segs = RP._buffers(torch, lay)
        r.render(cam, SPP, 50, 1, 3, sums.data_ptr(), segs.data_ptr())
        return sums, segs

    RP._assert_device_equal(RP._device_frames(True, body), RP._device_frames(False, body))


def test_out_of_range_samples_take_the_generic_tail():
    """The four-sphere scene with a lambertian albedo of (1.5, 1.0, -0.25) at 64 x 32 @ 8 spp, depth
    4: paths through that sphere carry a throughput above 1 and below 0 into the round's miss finish,
    whose samples take flush_sample's generic tail (64-bit sums, flags), beside in-range samples
    from the batch's sky finish and zeros from the absorbed / depth-limit finish."""
    shape = (64, 32, 8)
    ref = RP.reference("four_out_of_range", 4, shape)
    first = RP.reference("four_out_of_range", 4, (64, 32, 1))[0]
    assert (first[..., 0] > 1).any() and (first[..., 2] < 0).any()
    RP.assert_equal(frame("four_out_of_range", 4, shape), ref)
