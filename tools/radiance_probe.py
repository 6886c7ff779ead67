#!/usr/bin/env python3
"""rt_radiance_rays against rt_render on the same frame's worth of paths (not a test; bench.py
is unchanged).

On the C3 scene (random spheres), camera rays for `--width` x 9/16 `--width` pixels x `--spp`
samples, built on the device with torch from the fp32 camera vectors (pixel-square jitter, a
uniform point of the defocus disk, a uniform time; keys {pixel, sample, 5}), max_depth `--depth`:
  radiance   rt_radiance_rays over those rays, with segment counts;
  render     rt_render of the same frame with the tuning that selects the one-path-per-lane tree
             kernel (block 512, traversal 8: no sphere grid, no coherent primaries; fp64:
             f64_kernel 3) -- the same tree and the same path population.  (The query's fp32
             traversal adds whole-record LDS reads and pop culling, 8 | 16 | 512, as
             rt_trace_rays does; at block 512 the library instantiates the render kernel with
             traversal 8 only, so that is what the comparison runs.)
Both run in the same process, alternating, `--reps` times each after one warm-up of each, timed
by rt_last_kernel_ms.  One JSON line per precision: both medians and spreads (max - min of the
repeats), segments, Msegments/s and the ratio of the medians, and for scale rt_trace_rays'
median on the same rays (their first segments alone).  There is no pass threshold: the
render kernel has its camera inlined and its sums in registers, the query reads 28 B (fp32) and
writes 12-16 B per ray, so the ratio is the finding.

python tools/radiance_probe.py [--width 1920 --spp 2 --depth 50 --reps 5 --out profiles/radiance_probe.jsonl]
"""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from raytracingproject_amd import _native as N  # noqa: E402
from raytracingproject_amd import api, rtweekend, scenes  # noqa: E402

TREE_TRAVERSAL = N.RT_TRAV_SELROOT   # the one-path-per-lane tree kernel instantiated at block 512


def camera_rays_device(cam, spp, seed=7):
    """-> (rays float32[n, 7], keys uint32[n, 4]) on the device, pixel-major, sample-minor."""
    import torch
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    W, H = cam.image_width, cam.image_height
    n = W * H * spp
    vec = lambda v: torch.tensor(list(v), dtype=torch.float32, device=dev)   # noqa: E731
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    pix, k = idx // spp, idx % spp
    i, j = (pix % W).float()[:, None], (pix // W).float()[:, None]
    u = torch.rand((n, 5), generator=g, device=dev, dtype=torch.float32)
    ps = vec(cam.pixel00_loc) + (i + u[:, 0:1] - 0.5) * vec(cam.pixel_delta_u) + (j + u[:, 1:2] - 0.5) * vec(cam.pixel_delta_v)
    o = vec(cam.center).expand(n, 3)
    if cam.defocus_angle > 0:
        rad, th = torch.sqrt(u[:, 2:3]), 2 * math.pi * u[:, 3:4]
        o = o + rad * torch.cos(th) * vec(cam.defocus_disk_u) + rad * torch.sin(th) * vec(cam.defocus_disk_v)
    rays = torch.cat([o, ps - o, u[:, 4:5]], dim=1).contiguous()
    keys = torch.stack([pix, k, torch.full_like(pix, 5), torch.zeros_like(pix)], dim=1).to(torch.int32).contiguous()
    return rays, keys


def measure(prec, S, M, cam, spp, reps, DEPTH):
    import torch
    f64 = prec == N.RT_PREC_F64
    rays, keys = camera_rays_device(cam, spp)
    if f64:
        rays = rays.double()
    n = len(rays)
    tdt = torch.float64 if f64 else torch.float32
    si = N.shard_layout(cam.image_width, cam.image_height, 0, 1)
    with N.Renderer(0, 0x5EED, prec) as q, N.Renderer(0, 0x5EED, prec) as r:
        q.upload_scene(S, M)
        if f64:
            r.set_tuning(f64_kernel=3)
        else:
            r.set_tuning(traversal=TREE_TRAVERSAL, block=512)
        r.upload_scene(S, M)
        d_rad = torch.empty((n, 3), dtype=tdt, device="cuda")
        d_seg = torch.empty(n, dtype=torch.int32, device="cuda")
        d_sums = torch.empty((si.shard_tiles * 64, 3), dtype=tdt, device="cuda")
        d_rseg = torch.empty(si.shard_tiles * 64, dtype=torch.int32, device="cuda")
        d_hits = torch.empty(n * N.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms = {"radiance": [], "render": [], "trace": []}
        for rep in range(reps + 1):   # (the first round warms up)
            q.trace_rays(rays.data_ptr(), n, d_hits.data_ptr())   # the rays' first segments alone, for scale
            t_t = q.last_kernel_ms()
            if rep:
                ms["trace"].append(t_t)
            q.radiance_rays(rays.data_ptr(), n, keys.data_ptr(), DEPTH, d_rad.data_ptr(), d_seg.data_ptr())
            t_q = q.last_kernel_ms()
            r.render(cam, spp, DEPTH, 0, 1, d_sums.data_ptr(), d_rseg.data_ptr())
            t_r = r.last_kernel_ms()
            if rep:
                ms["radiance"].append(t_q)
                ms["render"].append(t_r)
        torch.cuda.synchronize()
        seg_q, seg_r = int(d_seg.sum(dtype=torch.int64).item()), int(d_rseg.sum(dtype=torch.int64).item())
        finite = bool(torch.isfinite(d_rad).all().item())
        info = r.scene_info()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    return {"scene": "c3", "precision": "fp64" if f64 else "fp32", "width": cam.image_width, "height": cam.image_height,
            "spp": spp, "max_depth": DEPTH, "rays": n, "reps": reps,
            "render_kernel": {"block": info.render_block, "traversal": info.render_traversal},
            "radiance_ms_median": round(med["radiance"], 4), "radiance_ms_spread": round(spread["radiance"], 4),
            "radiance_segments": seg_q, "radiance_msegments_per_s": round(seg_q / med["radiance"] / 1e3, 1),
            "render_ms_median": round(med["render"], 4), "render_ms_spread": round(spread["render"], 4),
            "render_segments": seg_r, "render_msegments_per_s": round(seg_r / med["render"] / 1e3, 1),
            "radiance_over_render_ms": round(med["radiance"] / med["render"], 4),
            "trace_first_segments_ms_median": round(med["trace"], 4), "radiance_finite": finite}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=2)
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
        line = measure(N.RT_PREC_F64 if pname == "fp64" else N.RT_PREC_F32, S, M, cam, a.spp, a.reps, a.depth)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
