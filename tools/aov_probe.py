#!/usr/bin/env python3
"""rt_render_pixels_aov against the composed route it replaces (not a test; bench.py is unchanged).

On the C3 scene (random spheres) at `--width` x 9/16 `--width`, a full-frame job list {p, 0, spp}
for each spp of `--spp`, per precision, all in one process, alternating, `--reps` times each after
one warm-up round:
  fused     rt_render_pixels_aov with all five outputs (rt_last_kernel_ms: the whole call, the scan
            and its read-back, the seed and finalize launches included);
  plain     fp32 only: the same call on a context created under RT_AOV_COMBINE=0 -- one set of
            atomics per sample instead of the wave combine;
  composed  rt_camera_rays + rt_trace_rays over the same list, the two calls' rt_last_kernel_ms
            added.  The caller's reduction of the hit records is NOT counted, which favours this
            route.  Its buffers are 44 or 72 B of ray and key plus 72 B of rt_hit per sample:
            `--composed-spp` (default: the same spp) measures it at fewer samples where they do not
            fit, and the line says so (composed_spp, and the per-sample figures).
  --traversals  instead of those: the fused call (the wave combine) on a context with
            RT_TRAV_DEFAULT (the call walks the sphere grid: rt_pixels_plan) and on one with
            RT_TRAV_DEFAULT & ~RT_TRAV_GRID (the tree), alternating.  grid_wins: the tree's median
            exceeds the grid's by more than the two spreads.
One JSON line per precision and spp with medians, spreads (max - min) and ratios.  There is no pass
threshold: whether fused is below composed, and whether the combine pays, is the finding.

python tools/aov_probe.py [--width 1920 --spp 2,16 --reps 5 --out profiles/aov_probe.jsonl]
python tools/aov_probe.py --traversals [--spp 2,16 --reps 10 --out profiles/aov_traversals.jsonl]
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from raytracingproject_amd import _native as N  # noqa: E402
from raytracingproject_amd import api, rtweekend, scenes  # noqa: E402


def jobs_of(pixel, count):
    j = np.zeros(len(pixel), N.RtPixelJob)
    j["pixel"], j["sample_count"] = pixel, count
    return j


def renderer(prec, S, M, combine, traversal=None):
    old = os.environ.get("RT_AOV_COMBINE")
    os.environ["RT_AOV_COMBINE"] = "1" if combine else "0"   # (read at rt_create)
    try:
        r = N.Renderer(0, 0x5EED, prec)
    finally:
        if old is None:
            del os.environ["RT_AOV_COMBINE"]
        else:
            os.environ["RT_AOV_COMBINE"] = old
    if traversal is not None:
        r.set_tuning(traversal=traversal)
    r.upload_scene(S, M)
    return r


def measure_traversals(prec, S, M, cam, spp, reps):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    npx = cam.image_width * cam.image_height
    d_jobs = torch.from_numpy(jobs_of(np.arange(npx), spp).view(np.uint8)).to("cuda")
    ctxs = {"grid": renderer(prec, S, M, True, N.RT_TRAV_DEFAULT),
            "tree": renderer(prec, S, M, True, N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID)}
    plans = {}
    for k, r in ctxs.items():
        p = r.pixels_plan(cam)
        assert p.walks_grid == (1 if k == "grid" else 0), (k, p.walks_grid)
        plans[k] = {"traversal": p.traversal, "block": p.block, "lds_bytes": p.lds_bytes,
                                  "walks_grid": {n: r.pixels_plan(cam, c).walks_grid for n, c in
                                                 (("pixels", N.RT_QUERY_PIXELS), ("moments", N.RT_QUERY_MOMENTS),
                                                  ("aov", N.RT_QUERY_AOV))}}
    d_alb = torch.empty((npx, 3), dtype=tdt, device="cuda")
    d_nrm = torch.empty((npx, 3), dtype=tdt, device="cuda")
    d_dep = torch.empty(npx, dtype=tdt, device="cuda")
    d_id = torch.empty(npx, dtype=torch.int32, device="cuda")
    d_hits = torch.empty(npx, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ms, hits = {k: [] for k in ctxs}, {}
    for rep in range(reps + 1):   # (the first round warms up)
        for k, r in ctxs.items():
            r.render_pixels_aov(cam, d_jobs.data_ptr(), npx, d_alb.data_ptr(), d_nrm.data_ptr(), d_dep.data_ptr(),
                                d_id.data_ptr(), d_hits.data_ptr())
            t = r.last_kernel_ms()
            hits[k] = int(d_hits.sum(dtype=torch.int64).item())
            if rep:
                ms[k].append(t)
    for r in ctxs.values():
        r.close()
    assert hits["grid"] == hits["tree"], hits
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    line = {"probe": "aov-traversals", "scene": "c3", "precision": "fp64" if f64 else "fp32", "width": cam.image_width,
            "height": cam.image_height, "spp": spp, "samples": npx * spp, "reps": reps, "hits": hits["grid"],
            "plans": plans}
    for k in ms:
        line[f"aov_{k}_ms_median"] = round(med[k], 4)
        line[f"aov_{k}_ms_spread"] = round(spread[k], 4)
    line["aov_grid_over_tree"] = round(med["grid"] / med["tree"], 4)
    line["aov_grid_wins"] = bool(med["tree"] - med["grid"] > spread["grid"] + spread["tree"])
    return line


def measure(prec, S, M, cam, spp, cspp, reps):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    npx = cam.image_width * cam.image_height
    d_jobs = torch.from_numpy(jobs_of(np.arange(npx), spp).view(np.uint8)).to("cuda")
    d_cjobs = torch.from_numpy(jobs_of(np.arange(npx), cspp).view(np.uint8)).to("cuda")
    n, cn = npx * spp, npx * cspp
    ctxs = {"fused": renderer(prec, S, M, True)}
    if not f64:
        ctxs["plain"] = renderer(prec, S, M, False)
    q = ctxs["fused"]
    d_alb = torch.empty((npx, 3), dtype=tdt, device="cuda")
    d_nrm = torch.empty((npx, 3), dtype=tdt, device="cuda")
    d_dep = torch.empty(npx, dtype=tdt, device="cuda")
    d_id = torch.empty(npx, dtype=torch.int32, device="cuda")
    d_hits = torch.empty(npx, dtype=torch.int32, device="cuda")
    d_rays = torch.empty((cn, 7), dtype=tdt, device="cuda")
    d_keys = torch.empty(cn * 16, dtype=torch.uint8, device="cuda")
    d_rec = torch.empty(cn * N.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {k: [] for k in (*ctxs, "camera_rays", "trace_rays")}
    hits = {}
    for rep in range(reps + 1):   # (the first round warms up)
        t = {}
        for k, r in ctxs.items():
            r.render_pixels_aov(cam, d_jobs.data_ptr(), npx, d_alb.data_ptr(), d_nrm.data_ptr(), d_dep.data_ptr(),
                                d_id.data_ptr(), d_hits.data_ptr())
            t[k] = r.last_kernel_ms()
            hits[k] = int(d_hits.sum(dtype=torch.int64).item())
        assert q.camera_rays(cam, d_cjobs.data_ptr(), npx, d_rays.data_ptr(), d_keys.data_ptr(), None, cn) == cn
        t["camera_rays"] = q.last_kernel_ms()
        q.trace_rays(d_rays.data_ptr(), cn, d_rec.data_ptr())
        t["trace_rays"] = q.last_kernel_ms()
        torch.cuda.synchronize()
        if rep:
            for k, v in t.items():
                ms[k].append(v)
    for r in ctxs.values():
        r.close()
    assert len(set(hits.values())) == 1, hits
    med = {k: float(np.median(v)) for k, v in ms.items()}
    composed = [a + b for a, b in zip(ms["camera_rays"], ms["trace_rays"])]
    line = {"scene": "c3", "precision": "fp64" if f64 else "fp32", "width": cam.image_width,
            "height": cam.image_height, "spp": spp, "samples": n, "jobs": npx, "composed_spp": cspp,
            "composed_samples": cn, "composed_buffer_gb": round(cn * ((56 if f64 else 28) + 16 + 72) / 1e9, 3),
            "reps": reps, "hits": hits["fused"]}
    for k in ms:
        line[f"{k}_ms_median"] = round(med[k], 4)
        line[f"{k}_ms_spread"] = round(float(max(ms[k]) - min(ms[k])), 4)
    line["composed_ms_median"] = round(float(np.median(composed)), 4)
    line["composed_ms_spread"] = round(float(max(composed) - min(composed)), 4)
    line["fused_ns_per_sample"] = round(med["fused"] * 1e6 / n, 4)
    line["composed_ns_per_sample"] = round(float(np.median(composed)) * 1e6 / cn, 4)
    line["fused_over_composed_per_sample"] = round(line["fused_ns_per_sample"] / line["composed_ns_per_sample"], 4)
    if "plain" in med:
        line["combine_over_plain_ms"] = round(med["fused"] / med["plain"], 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", default="2,16")
    ap.add_argument("--composed-spp", type=int, default=0, help="cap on the composed route's spp (0: none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--traversals", action="store_true", help="the grid against the tree instead of the routes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rtweekend.reset_stream()
    S, M = api.flatten(scenes.random_spheres())
    cam_api = scenes.main_camera()
    cam_api.image_width = a.width
    cam = cam_api.native
    lines = []
    for pname in a.precisions.split(","):
        for spp in (int(s) for s in a.spp.split(",")):
            cspp = min(spp, a.composed_spp) if a.composed_spp > 0 else spp
            prec = N.RT_PREC_F64 if pname == "fp64" else N.RT_PREC_F32
            line = (measure_traversals(prec, S, M, cam, spp, a.reps) if a.traversals
                    else measure(prec, S, M, cam, spp, cspp, a.reps))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
