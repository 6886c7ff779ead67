"""The candidates' near bound of csrc/rt_batch_cull.h (cull_near, the packed list word, the
order of the list: what closest_hit's depth-ordered candidate loop stops on) against brute
force: tests/cpp/cand_depth_driver.cpp under ASan + UBSan, over scenes x cameras written here
in test_batch_cull's case format.  No GPU, and the native library is not loaded.

Every root the kernel's fp32 sphere test can report for a camera ray of a tile must be at least
the sphere's bound for that tile, raw and as packed; every list that fits the cap must come out
of the rank sort as a permutation ordered by (near, index).  Four mutated copies of the bound
(no rounding margins, no lens radius, no motion half-length, the packed bound rounded up) must
each make the driver fail.
"""
from __future__ import annotations

import math
import subprocess

import numpy as np
import pytest

from raytracingproject_amd import build, rtweekend, scenes
from test_batch_cull import camera_words, case, records, synthetic_scenes, world_records


def moved(recs, scale, shift):
    """SphereF records scaled about the origin, then moved."""
    out = np.array(recs, np.float32, copy=True)
    out[:, 0:3] = (recs[:, 0:3].astype(np.float64) * scale + shift).astype(np.float32)
    out[:, 3] = recs[:, 3] * np.float32(scale)
    out[:, 4:7] = recs[:, 4:7] * np.float32(scale)
    return out


def moved_camera(scale, shift, lookfrom=(13, 2, 3), lookat=(0, 0, 0), focus_dist=10.0, **kw):
    lf = tuple(np.asarray(lookfrom, float) * scale + shift)
    la = tuple(np.asarray(lookat, float) * scale + shift)
    return camera_words(lookfrom=lf, lookat=la, focus_dist=focus_dist * scale, **kw)


def axis_case(rng, name, radius):
    """A camera whose pixels have no size and no lens: every ray of the tile is the axis.  Small
    spheres centred on it: the root is (s - r) / L to rounding, so the bound's margins and the
    downward truncation of the packed word are all that keeps it below the root."""
    c = rng.uniform(-2, 2, 3)
    a = rng.normal(size=3)
    a *= 10.0 / np.linalg.norm(a)
    words = np.concatenate([c, c + a, np.zeros(12)]).astype(np.float32)
    c32 = words[0:3].astype(np.float64)
    a32 = words[3:6].astype(np.float64) - c32
    ax = a32 / np.linalg.norm(a32)
    sp = [(tuple(c32 + math.exp(rng.uniform(math.log(0.5), math.log(300.0))) * ax), float(radius), (0, 0, 0))
          for _ in range(400)]
    return case(name, (8, 8, 0, words), records(sp))


def near_scene(rng):
    """Around the main camera at (13, 2, 3): spheres a few radii in front of the lens and beside
    the view, static and moving towards the camera -- where the lens radius and the motion's
    half-length decide the bound."""
    c = np.array([13.0, 2.0, 3.0])
    fwd = -c / np.linalg.norm(c)
    side = np.cross(fwd, [0, 1, 0])
    side /= np.linalg.norm(side)
    up = np.cross(side, fwd)
    sp = []
    for _ in range(60):
        dist = rng.uniform(0.3, 4.0)
        off = rng.uniform(-0.35, 0.35, 2) * dist
        p = c + dist * fwd + off[0] * side + off[1] * up
        r = rng.uniform(0.02, 0.25) * dist
        cv = (0, 0, 0) if rng.random() < 0.5 else tuple(-fwd * rng.uniform(0.2, 1.5) * dist + rng.normal(size=3) * 0.1)
        sp.append((tuple(p), float(r), cv))
    return records(sp)


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    rng = np.random.default_rng(21)
    rtweekend.reset_stream()
    field = world_records(scenes.random_spheres())
    assert len(field) == 484
    scene_set = {
        "hollow": world_records(scenes.hollow_glass()),
        "four": world_records(scenes.four_spheres()),
        "edges": synthetic_scenes(rng),
        "near": near_scene(rng),
    }
    small = dict(width=44, aspect=44 / 20)   # 6 x 3 tiles, partial at the right and bottom edges
    cams = {
        "main": camera_words(**small),
        "nodefocus": camera_words(defocus_angle=0.0, **small),
        "defocus10": camera_words(defocus_angle=10.0, **small),
        "vfov5": camera_words(vfov=5.0, **small),
        "vfov120": camera_words(width=72, aspect=2.0, vfov=120.0),
        "vfov120defocus10": camera_words(width=72, aspect=2.0, vfov=120.0, defocus_angle=10.0),
        "inside": camera_words(lookfrom=(0.5, 0.4, 0.6), lookat=(4, 0.3, -2), focus_dist=3.0, **small),
        "inside120": camera_words(width=72, aspect=2.0, vfov=120.0, lookfrom=(0.5, 0.4, 0.6), lookat=(4, 0.3, -2),
                                  focus_dist=3.0),
        "far200": camera_words(lookfrom=(200 * 13 / 13.5, 200 * 2 / 13.5, 200 * 3 / 13.5), focus_dist=200.0, vfov=4.0,
                               **small),
    }
    for _ in range(4):   # random cameras around the field, looking into it
        lf = rng.uniform(-12, 12, 3) * [1, 0.15, 1] + [0, 1.2, 0]
        cams[f"random{len(cams)}"] = camera_words(lookfrom=tuple(lf), lookat=tuple(rng.uniform(-3, 3, 3) * [1, 0.1, 1]),
                                                  vfov=float(rng.uniform(10, 90)), focus_dist=float(rng.uniform(1, 12)),
                                                  defocus_angle=float(rng.choice([0.0, 0.6, 4.0])), **small)
    nan_cam = camera_words(**small)
    nan_cam[3][4] = np.float32("nan")
    blob = small_blob = b""
    for sn, recs in scene_set.items():
        for cn, cam in cams.items():
            small_blob += case(f"{sn}/{cn}", cam, recs)
    # scaled by 1e-3, and scaled and moved 1e4 off the origin (fp32 spacing there: 1e-3, a sphere's size)
    for sn in ("four", "edges", "near"):
        for tag, shift in (("milli", 0.0), ("milli1e4", np.array([1e4, -1e4, 1e4]))):
            for cn, kw in (("main", {}), ("nodefocus", dict(defocus_angle=0.0)), ("defocus10", dict(defocus_angle=10.0))):
                small_blob += case(f"{sn}/{tag}/{cn}", moved_camera(1e-3, shift, **kw, **small),
                                   moved(scene_set[sn], 1e-3, shift))
    small_blob += axis_case(rng, "axis/r1e-4", 1e-4) + axis_case(rng, "axis/r0.05", 0.05)
    blob = small_blob
    for cn in ("main", "defocus10", "inside", "random9"):
        blob += case(f"field/{cn}", cams[cn], field)
    blob += case("field/nan", nan_cam, field)
    d = tmp_path_factory.mktemp("cand_depth")
    (d / "cases.bin").write_bytes(blob)
    # the mutated bounds run the cases without the 484-sphere field
    (d / "cases_small.bin").write_bytes(small_blob)
    return d


@pytest.fixture(scope="module")
def drivers():
    return build.build_cand_depth()


def run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)


def test_no_root_lies_below_the_bound(drivers, cases_file):
    p = run(drivers[0], cases_file / "cases.bin")
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    lines = {ln.split()[0]: ln for ln in p.stdout.splitlines() if ln and not ln.startswith(" ")}
    # the NaN camera bounds nothing; the main view bounds spheres and meets their roots
    assert " bounded 0 " in lines["field/nan"], lines["field/nan"]
    assert " bounded 0 " not in lines["field/main"] and " roots 0 " not in lines["field/main"], lines["field/main"]
    assert " lists 0 " not in lines["four/main"], lines["four/main"]


@pytest.mark.parametrize("mutant", [1, 2, 3, 4])
def test_mutated_bound_is_caught(drivers, cases_file, mutant):
    p = run(drivers[mutant], cases_file / "cases_small.bin")
    print(p.stdout)
    assert p.returncode == 1 and "BELOW" in p.stdout, (mutant, p.stdout[-2000:], p.stderr[-2000:])
