"""The host-side scene packing (csrc/rt_pack.cpp: pack_scene, everything rt_upload_scene_ex
computes before it touches the device) and the sphere grid's reach test (grid_reach_ok) under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/pack_driver.cpp, a stand-alone program
built by raytracingproject_amd.build.build_pack and run directly.

For both precisions and both mesh-builder settings the driver checks the sphere, big-sphere,
material and triangle records against the inputs, the id map, the grid's entry count, the reach
box and box_extent; then the rejections with their status codes; then grid_reach_ok for the
cameras below against the verdicts test_grid_reach and FAR_CASES (tests/test_gpu_parity.py)
assert on the GPU."""
import os
import subprocess

import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, meshgen, rtweekend, scenes


def _field(ground: bool = True):
    rtweekend.reset_stream()
    S, M = api.flatten(scenes.random_spheres())
    return (S, M) if ground else (S[S["radius"] < 64].copy(), M)


def _neg():
    """The negated field of test_bvh_boxes: radius negated on indices 1::3 and on the ground."""
    S, M = _field()
    S = S.copy()
    S["radius"][1::3] *= -1
    S["radius"][0] *= -1
    return S, M


def _radius0():
    """four_spheres with a sphere of radius 0 between them."""
    S, M = api.flatten(scenes.four_spheres())
    S = np.concatenate([S, S[1:2]])
    S[-1]["center"], S[-1]["radius"] = (2.0, 0.5, 1.0), 0.0
    return S, M


def _blob(mixed: bool):
    V, F = meshgen.blob(0, radius=meshgen.MESH_RADIUS, center=meshgen.MESH_CENTER)
    if not mixed:
        M = np.zeros(1, dtype=N.MATERIAL_DTYPE)
        M[0]["type"], M[0]["albedo"] = N.RT_METAL, (0.7, 0.6, 0.5)
        return np.zeros(0, dtype=N.SPHERE_DTYPE), M, N.triangles(V, F, 0)
    S, M = _field()
    return S, M, N.triangles(V, F, 3)


def _far(dist):
    """tests/test_gpu_parity.py far_cameras: main.cpp's view of the field from `dist` units away."""
    look = np.array((13.0, 2.0, 3.0))
    cam = scenes.main_camera()
    cam.image_width = 160
    cam.lookfrom = tuple(look / np.linalg.norm(look) * dist)
    cam.vfov, cam.defocus_angle, cam.focus_dist = float(np.degrees(2 * np.arctan(3.0 / dist))), 0.0, float(dist)
    return cam.native


def _nan_camera():
    cam = scenes.main_camera().native
    cam.center[1] = float("nan")
    return cam


# (camera, walks) per input
def _cams_ground():
    return [(scenes.main_camera().native, 1), (_far(150.0), 0), (_far(2.0e4), 0), (_far(2.0e7), 0), (_nan_camera(), 0)]


def _cams_no_ground():
    return [(scenes.main_camera().native, 1), (_far(150.0), 1), (_far(2.0e4), 0), (_nan_camera(), 0)]


def _cams_main():
    return [(scenes.main_camera().native, 1), (_nan_camera(), 0)]


def _cams_no_grid():
    return [(scenes.main_camera().native, 0)]   # (no spheres, no grid: nothing to walk)


CASES = {
    "field": (lambda: _field(True), _cams_ground),
    "field_no_ground": (lambda: _field(False), _cams_no_ground),
    "hollow": (lambda: api.flatten(scenes.hollow_glass()), _cams_main),
    "four": (lambda: api.flatten(scenes.four_spheres()), _cams_main),
    "neg": (_neg, _cams_ground),
    "radius0": (_radius0, _cams_main),
    "blob": (lambda: _blob(False), _cams_no_grid),
    "blob_mixed": (lambda: _blob(True), _cams_ground),
}
# per input: spheres, big spheres, triangles, grids built over the four packs, cameras that walk
# (so that no case goes vacuous)
EXPECT = {
    "field": (485, 1, 0, 4, 1), "field_no_ground": (484, 0, 0, 4, 2), "hollow": (10, 1, 0, 4, 1),
    "four": (4, 1, 0, 4, 1), "neg": (485, 1, 0, 4, 1), "radius0": (5, 1, 0, 4, 1), "blob": (0, 0, 20, 0, 0),
    "blob_mixed": (485, 1, 20, 4, 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_pack_scene_and_grid_reach(case, tmp_path):
    from raytracingproject_amd.build import build_pack
    exe = build_pack()
    make, cams = CASES[case]
    arrays = make()
    S, M = arrays[0], arrays[1]
    T = arrays[2] if len(arrays) > 2 else np.zeros(0, dtype=N.TRIANGLE_DTYPE)
    cams = cams()
    n_s, n_big, n_t, n_grids, n_walks = EXPECT[case]
    assert (len(S), len(T)) == (n_s, n_t) and sum(w for _, w in cams) == n_walks
    blob = np.array([len(S), len(M), len(T), len(cams)], dtype="<i4").tobytes()
    blob += np.ascontiguousarray(S, dtype=N.SPHERE_DTYPE).tobytes()
    blob += np.ascontiguousarray(M, dtype=N.MATERIAL_DTYPE).tobytes()
    blob += np.ascontiguousarray(T, dtype=N.TRIANGLE_DTYPE).tobytes()
    for cam, walks in cams:
        assert len(bytes(cam)) == 160
        blob += bytes(cam) + np.array([walks, 0], dtype="<i4").tobytes()
    f = tmp_path / "scene.bin"
    f.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=env)
    report = "AddressSanitizer" in r.stderr or "runtime error" in r.stderr or "LeakSanitizer" in r.stderr
    assert r.returncode == 0 and not report, r.stdout[-3000:] + r.stderr[-5000:]
    print(r.stdout)
    w = r.stdout.split()
    got = {k: int(w[w.index(k) + 1]) for k in ("spheres", "big", "triangles", "packs", "grids", "reach", "walks")}
    assert w[0] == "pack" and got == dict(spheres=n_s, big=n_big, triangles=n_t, packs=4, grids=n_grids,
                                          reach=len(cams), walks=n_walks), got
    assert "checks failed 0" in r.stdout
