"""The sphere tree and the sphere grid over scenes with negative radii (the reference's hollow
spheres: its roots use radius * radius, its aabb orders the corners) under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/cpp/bvh_boxes_driver.cpp, a stand-alone program built by
raytracingproject_amd.build.build_bvh_boxes and run directly.

For max_leaf in {1, 4} x front in {0, -1, 3} it checks that every sphere outside the big and
front lists occurs exactly once in the tree, that every child box has lo <= hi and contains
the swept box (from |r|) of every sphere beneath it, that the tree is byte-identical to the
trees of the same scene with every radius positive and every radius negative, and that the
grid builder returns the same header and bytes for the three sign patterns.

(Before exact_box took |r|, a negative radius gave an inverted box: every scene here failed.)"""
import os
import subprocess

import numpy as np
import pytest

from raytracingproject_amd import api, rtweekend, scenes


def _random_field():
    rtweekend.reset_stream()
    return api.flatten(scenes.random_spheres())[0]


def _neg(ground: bool) -> np.ndarray:
    """The random field with the radius negated on indices 1::3 (and on the ground, index 0)."""
    S = _random_field().copy()
    S["radius"][1::3] *= -1
    if ground:
        S["radius"][0] *= -1
    return S


def _spheres(*rows) -> np.ndarray:
    S = np.zeros(len(rows), dtype=_random_field().dtype)
    for k, (c, r) in enumerate(rows):
        S[k]["center"], S[k]["radius"] = c, r
    return S


CASES = {
    "neg": lambda: _neg(False),
    "neg_ground": lambda: _neg(True),
    "hollow": lambda: api.flatten(scenes.hollow_glass())[0],
    "single_negative": lambda: _spheres(((0, 1, 0), -0.4)),                       # a single-leaf tree
    "concentric": lambda: _spheres(((0, 0, 0), 0.5), ((0, 0, 0), -0.4)),
}
# negative radii in each input (so that no case goes vacuous)
EXPECT_NEGATIVE = {"neg": 162, "neg_ground": 163, "hollow": 4, "single_negative": 1, "concentric": 1}


@pytest.mark.parametrize("case", sorted(CASES))
def test_tree_and_grid_depend_on_abs_radius_only(case, tmp_path):
    from raytracingproject_amd.build import build_bvh_boxes
    exe = build_bvh_boxes()
    S = CASES[case]()
    assert int((S["radius"] < 0).sum()) == EXPECT_NEGATIVE[case]
    rec = np.concatenate([S["center"], S["center_vec"], S["radius"][:, None],
                          (S["moving"] != 0).astype(np.float64)[:, None]], axis=1).astype(np.float64)
    assert rec.shape == (len(S), 8)
    f = tmp_path / "spheres.f64"
    f.write_bytes(np.ascontiguousarray(rec).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=env)
    report = "AddressSanitizer" in r.stderr or "runtime error" in r.stderr or "LeakSanitizer" in r.stderr
    assert r.returncode == 0 and not report, r.stdout[-3000:] + r.stderr[-5000:]
    print(r.stdout)
    w = r.stdout.split()
    assert w[0] == "bvh_boxes" and int(w[w.index("spheres") + 1]) == len(S)
    assert int(w[w.index("negative") + 1]) == EXPECT_NEGATIVE[case]
    assert int(w[w.index("trees") + 1]) == 6                         # every parameter set built
    if case.startswith("neg"):
        # (with its R = 1 spheres in the front list, -1 and 3, the field suits a grid at both densities)
        assert int(w[w.index("grids") + 1]) >= 8
    assert "checks failed 0" in r.stdout
