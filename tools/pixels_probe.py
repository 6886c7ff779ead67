#!/usr/bin/env python3
"""rt_render_pixels against rt_radiance_rays and rt_render on the same paths (not a test; bench.py
is unchanged).

On the C3 scene (random spheres) at `--width` x 9/16 `--width`, max_depth `--depth`, per precision:
  (a) pixels     rt_render_pixels over a full-frame job list {p, 0, spp}, with segment counts;
      radiance   rt_radiance_rays over exactly those samples' rays and keys, pre-built once with
                 rt_camera_rays (that kernel is the previous commit's: the baseline);
      render     rt_render of the same frame with the one-path-per-lane tree kernel (block 512,
                 traversal 8; fp64: f64_kernel 3), as tools/radiance_probe.py;
  (b) sparse     rt_render_pixels over the pixels of every eighth 8x8 tile at 8 x spp samples:
                 the same T as (a) in an eighth of the jobs;
  (c) scan       rt_camera_rays with max_rays = 0 over the full-frame job list: the scan of the
                 jobs' counts, the 8-byte read-back and nothing else (it answers RT_ERR_INVALID
                 for T > 0 before any ray is written).  Wall-clock, since the call ends before the
                 closing timing event is recorded.
  --traversals   instead of (a)-(c): rt_render_pixels over the full-frame list and over the sparse
                 list of (b), and rt_render_pixels_moments over the full-frame list, each on a
                 context with RT_TRAV_DEFAULT (the queries walk the sphere grid: rt_pixels_plan) and
                 on one with RT_TRAV_DEFAULT & ~RT_TRAV_GRID (the tree, the path before the grid
                 walk), for each spp of `--spp` (a comma list); alternating, medians of `--reps`.
                 grid_wins: the tree's median exceeds the grid's by more than the two spreads.
All in one process, alternating, `--reps` times each after one warm-up of each; (a) and (b) are
timed by rt_last_kernel_ms, which for rt_render_pixels spans the whole call, scan and read-back
included.  One JSON line per precision with medians, spreads (max - min) and ratios.  There is no
pass threshold: what the in-kernel camera saves (44 or 72 bytes of ray and key per path) against
what the job search and the per-sample atomics or stores cost is the finding.

python tools/pixels_probe.py [--width 1920 --spp 2 --depth 50 --reps 5 --out profiles/pixels_probe.jsonl]
python tools/pixels_probe.py --traversals [--spp 2,16 --reps 10 --out profiles/pixels_traversals.jsonl]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from raytracingproject_amd import _native as N  # noqa: E402
from raytracingproject_amd import api, rtweekend, scenes  # noqa: E402

TREE_TRAVERSAL = N.RT_TRAV_SELROOT   # the one-path-per-lane tree kernel instantiated at block 512


def jobs_of(pixel, count):
    j = np.zeros(len(pixel), N.RtPixelJob)
    j["pixel"], j["sample_count"] = pixel, count
    return j


def measure(prec, S, M, cam, spp, reps, depth):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    W, H = cam.image_width, cam.image_height
    si = N.shard_layout(W, H, 0, 1)
    full = jobs_of(np.arange(W * H), spp)
    jj, ii = np.mgrid[0:H, 0:W]
    tile = (jj // 8) * si.tiles_x + ii // 8
    sparse = jobs_of((jj * W + ii)[tile % 8 == 0], 8 * spp)
    up = lambda a: torch.from_numpy(a.view(np.uint8)).to("cuda")   # noqa: E731
    d_full, d_sparse = up(full), up(sparse)
    n = W * H * spp
    with N.Renderer(0, 0x5EED, prec) as q, N.Renderer(0, 0x5EED, prec) as r:
        q.upload_scene(S, M)
        if f64:
            r.set_tuning(f64_kernel=3)
        else:
            r.set_tuning(traversal=TREE_TRAVERSAL, block=512)
        r.upload_scene(S, M)
        d_rays = torch.empty((n, 7), dtype=tdt, device="cuda")
        d_keys = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_rad = torch.empty((n, 3), dtype=tdt, device="cuda")
        d_seg = torch.empty(n, dtype=torch.int32, device="cuda")
        d_out = torch.empty((len(full), 3), dtype=tdt, device="cuda")
        d_oseg = torch.empty(len(full), dtype=torch.int32, device="cuda")
        d_sums = torch.empty((si.shard_tiles * 64, 3), dtype=tdt, device="cuda")
        d_rseg = torch.empty(si.shard_tiles * 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert q.camera_rays(cam, d_full.data_ptr(), len(full), d_rays.data_ptr(), d_keys.data_ptr(), None, n) == n
        camera_ms = q.last_kernel_ms()
        ms = {k: [] for k in ("pixels", "radiance", "render", "sparse", "scan")}
        seg = {}
        for rep in range(reps + 1):   # (the first round warms up)
            t = {}
            q.render_pixels(cam, d_full.data_ptr(), len(full), depth, d_out.data_ptr(), d_oseg.data_ptr())
            t["pixels"] = q.last_kernel_ms()
            seg["pixels"] = int(d_oseg.sum(dtype=torch.int64).item())
            q.radiance_rays(d_rays.data_ptr(), n, d_keys.data_ptr(), depth, d_rad.data_ptr(), d_seg.data_ptr())
            t["radiance"] = q.last_kernel_ms()
            r.render(cam, spp, depth, 0, 1, d_sums.data_ptr(), d_rseg.data_ptr())
            t["render"] = r.last_kernel_ms()
            q.render_pixels(cam, d_sparse.data_ptr(), len(sparse), depth, d_out.data_ptr(), d_oseg.data_ptr())
            t["sparse"] = q.last_kernel_ms()
            seg["sparse"] = int(d_oseg[: len(sparse)].sum(dtype=torch.int64).item())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            total = q.camera_rays_count(cam, d_full.data_ptr(), len(full))
            t["scan"] = (time.perf_counter() - t0) * 1e3
            assert total == n
            if rep:
                for k, v in t.items():
                    ms[k].append(v)
        torch.cuda.synchronize()
        seg["radiance"] = int(d_seg.sum(dtype=torch.int64).item())
        seg["render"] = int(d_rseg.sum(dtype=torch.int64).item())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"scene": "c3", "precision": "fp64" if f64 else "fp32", "width": W, "height": H, "spp": spp,
            "max_depth": depth, "samples": n, "jobs": len(full), "sparse_jobs": len(sparse),
            "sparse_samples": int(sparse["sample_count"].sum()), "reps": reps, "camera_rays_ms": round(camera_ms, 4)}
    for k in ms:
        line[f"{k}_ms_median"] = round(med[k], 4)
        line[f"{k}_ms_spread"] = round(float(max(ms[k]) - min(ms[k])), 4)
    line.update({f"{k}_segments": v for k, v in seg.items()})
    line["pixels_over_radiance_ms"] = round(med["pixels"] / med["radiance"], 4)
    line["pixels_over_render_ms"] = round(med["pixels"] / med["render"], 4)
    line["sparse_over_pixels_ms"] = round(med["sparse"] / med["pixels"], 4)
    return line


TRAVERSALS = {"grid": N.RT_TRAV_DEFAULT, "tree": N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID}


def traversal_contexts(prec, S, M, cam):
    """One context per traversal, the scene uploaded, and what rt_pixels_plan says each walks."""
    ctxs, plans = {}, {}
    for name, trav in TRAVERSALS.items():
        r = N.Renderer(0, 0x5EED, prec)
        r.set_tuning(traversal=trav)
        r.upload_scene(S, M)
        p = r.pixels_plan(cam)
        assert p.walks_grid == (1 if name == "grid" else 0), (name, p.walks_grid)
        ctxs[name], plans[name] = r, {"traversal": p.traversal, "block": p.block, "lds_bytes": p.lds_bytes,
                                  "walks_grid": {n: r.pixels_plan(cam, c).walks_grid for n, c in
                                                 (("pixels", N.RT_QUERY_PIXELS), ("moments", N.RT_QUERY_MOMENTS),
                                                  ("aov", N.RT_QUERY_AOV))}}
    return ctxs, plans


def compare(line, call, ms):
    """Medians and spreads of one call on both contexts into line; the verdict by the two spreads."""
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    for k in ms:
        line[f"{call}_{k}_ms_median"] = round(med[k], 4)
        line[f"{call}_{k}_ms_spread"] = round(spread[k], 4)
    line[f"{call}_grid_over_tree"] = round(med["grid"] / med["tree"], 4)
    line[f"{call}_grid_wins"] = bool(med["tree"] - med["grid"] > spread["grid"] + spread["tree"])


def measure_traversals(prec, S, M, cam, spp, reps, depth):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    W, H = cam.image_width, cam.image_height
    si = N.shard_layout(W, H, 0, 1)
    full = jobs_of(np.arange(W * H), spp)
    jj, ii = np.mgrid[0:H, 0:W]
    tile = (jj // 8) * si.tiles_x + ii // 8
    sparse = jobs_of((jj * W + ii)[tile % 8 == 0], 8 * spp)
    up = lambda a: torch.from_numpy(a.view(np.uint8)).to("cuda")   # noqa: E731
    d_full, d_sparse = up(full), up(sparse)
    d_out = torch.empty((len(full), 3), dtype=tdt, device="cuda")
    d_sq = torch.empty((len(full), 3), dtype=tdt, device="cuda")
    d_seg = torch.empty(len(full), dtype=torch.int32, device="cuda")
    ctxs, plans = traversal_contexts(prec, S, M, cam)
    calls = ("pixels", "moments", "sparse")
    ms = {c: {k: [] for k in ctxs} for c in calls}
    segs = {}
    torch.cuda.synchronize()
    for rep in range(reps + 1):   # (the first round warms up)
        for k, r in ctxs.items():
            r.render_pixels(cam, d_full.data_ptr(), len(full), depth, d_out.data_ptr(), d_seg.data_ptr())
            t = {"pixels": r.last_kernel_ms()}
            segs[k] = int(d_seg.sum(dtype=torch.int64).item())
            r.render_pixels_moments(cam, d_full.data_ptr(), len(full), depth, d_out.data_ptr(), d_sq.data_ptr(),
                                    d_seg.data_ptr())
            t["moments"] = r.last_kernel_ms()
            r.render_pixels(cam, d_sparse.data_ptr(), len(sparse), depth, d_out.data_ptr(), d_seg.data_ptr())
            t["sparse"] = r.last_kernel_ms()
            torch.cuda.synchronize()
            if rep:
                for c in calls:
                    ms[c][k].append(t[c])
    for r in ctxs.values():
        r.close()
    assert segs["grid"] == segs["tree"], segs
    line = {"probe": "pixels-traversals", "scene": "c3", "precision": "fp64" if f64 else "fp32", "width": W, "height": H,
            "spp": spp, "max_depth": depth, "samples": W * H * spp, "sparse_jobs": len(sparse), "reps": reps,
            "segments": segs["grid"], "plans": plans}
    for c in calls:
        compare(line, c, ms[c])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", default="2", help="samples per pixel (--traversals: a comma list)")
    ap.add_argument("--traversals", action="store_true", help="the grid against the tree instead of (a)-(c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rtweekend.reset_stream()
    S, M = api.flatten(scenes.random_spheres())
    cam_api = scenes.main_camera()
    cam_api.image_width = a.width
    cam = cam_api.native
    lines = []
    for pname in a.precisions.split(","):
        prec = N.RT_PREC_F64 if pname == "fp64" else N.RT_PREC_F32
        for spp in (int(x) for x in a.spp.split(",")):
            line = (measure_traversals if a.traversals else measure)(prec, S, M, cam, spp, a.reps, a.depth)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
