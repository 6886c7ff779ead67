#!/usr/bin/env python3
"""What the second moments and the adaptive loop cost (not a test; bench.py is unchanged).

On the C3 scene (random spheres) at `--width` x 9/16 `--width`, max_depth `--depth`:
  (a) moments    rt_render_pixels_moments against rt_render_pixels over a full-frame job list
                 {p, 0, spp} for each spp of `--spps`, per precision; same library, same process,
                 alternating, `--reps` launches each after one warm-up of each; rt_last_kernel_ms
                 (the whole call: scan, read-back, seed or reduce, finalize); medians, spreads
                 (max - min) and the ratio.
  (b) refine     rt_refine_jobs over one slot per pixel (sums and second moments of an 8-sample
                 fp32 round), `--reps` launches; rt_last_kernel_ms.
  (c) adaptive   one frame by Renderer.render_adaptive (fp32; min `--min`, max `--max`, rel_error
                 `--rel-error`, abs_floor `--abs-floor`): wall clock from the first call to the last
                 stats read-back (median of `--frames` frames after a warm-up frame), rounds, mean
                 samples per pixel, and the RMSE of its mean image against the uniform `--max`-spp
                 rt_render frame (the default kernel), whose own rt_last_kernel_ms is given for
                 comparison -- with, as the yardstick for that RMSE, the RMSE of a uniform rt_render
                 frame at the adaptive frame's mean spp (rounded up) against the same `--max`-spp frame.
  (t) traversals the adaptive frame of (c), and the denoised frame's total (rt_render_pixels_moments
                 + rt_render_pixels_aov + rt_denoise at `--denoise-spp`, the three calls'
                 rt_last_kernel_ms added, as tools/denoise_probe.py adds them), each on a context with
                 RT_TRAV_DEFAULT (the queries walk the sphere grid: rt_pixels_plan) and on one with
                 RT_TRAV_DEFAULT & ~RT_TRAV_GRID (the tree), alternating, `--reps` times after a
                 warm-up.  grid_wins: the tree's median exceeds the grid's by more than the two
                 spreads.  (tools/pixels_probe.py --traversals has the single calls.)
One JSON line per measurement.  There is no pass threshold.

python tools/adaptive_probe.py [--parts a,b,c --width 1920 --spps 2,16 --reps 10 --out profiles/adaptive_probe.jsonl]
python tools/adaptive_probe.py --parts t [--reps 10 --out profiles/adaptive_traversals.jsonl]
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


def jobs_of(pixel, count):
    j = np.zeros(len(pixel), N.RtPixelJob)
    j["pixel"], j["sample_count"] = pixel, count
    return j


def stats(v):
    return round(float(np.median(v)), 4), round(float(max(v) - min(v)), 4)


def part_a(prec, S, M, cam, spps, reps, depth):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    npx = cam.image_width * cam.image_height
    lines = []
    with N.Renderer(0, 0x5EED, prec) as r:
        r.upload_scene(S, M)
        d_s = torch.empty((npx, 3), dtype=tdt, device="cuda")
        d_q = torch.empty((npx, 3), dtype=tdt, device="cuda")
        d_g = torch.empty(npx, dtype=torch.int32, device="cuda")
        for spp in spps:
            d_j = torch.from_numpy(jobs_of(np.arange(npx), spp).view(np.uint8)).to("cuda")
            torch.cuda.synchronize()
            ms = {"pixels": [], "moments": []}
            for rep in range(reps + 1):   # (the first round warms up)
                r.render_pixels(cam, d_j.data_ptr(), npx, depth, d_s.data_ptr(), d_g.data_ptr())
                a = r.last_kernel_ms()
                segs = int(d_g.sum(dtype=torch.int64).item())
                r.render_pixels_moments(cam, d_j.data_ptr(), npx, depth, d_s.data_ptr(), d_q.data_ptr(), d_g.data_ptr())
                b = r.last_kernel_ms()
                assert int(d_g.sum(dtype=torch.int64).item()) == segs
                if rep:
                    ms["pixels"].append(a)
                    ms["moments"].append(b)
            line = {"part": "a", "scene": "c3", "precision": "fp64" if f64 else "fp32", "width": cam.image_width,
                    "height": cam.image_height, "spp": spp, "max_depth": depth, "samples": npx * spp, "reps": reps,
                    "segments": segs}
            for k, v in ms.items():
                line[f"{k}_ms_median"], line[f"{k}_ms_spread"] = stats(v)
            line["moments_over_pixels_ms"] = round(line["moments_ms_median"] / line["pixels_ms_median"], 4)
            lines.append(line)
    return lines


def part_b(S, M, cam, reps, depth):
    import torch
    npx = cam.image_width * cam.image_height
    with N.Renderer(0, 0x5EED, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        jobs = torch.from_numpy(jobs_of(np.arange(npx), 8).view(np.uint8)).to("cuda")
        d_s = torch.empty((npx, 3), dtype=torch.float32, device="cuda")
        d_q = torch.empty((npx, 3), dtype=torch.float32, device="cuda")
        d_st = torch.zeros(2, dtype=torch.int64, device="cuda")
        r.render_pixels_moments(cam, jobs.data_ptr(), npx, depth, d_s.data_ptr(), d_q.data_ptr())
        p = N.RtAdaptiveParams(0.05, 0.01, 8, 256, 256, 0)
        ms = []
        for rep in range(reps + 1):
            d_j = jobs.clone()
            torch.cuda.synchronize()
            r.refine_jobs(d_j.data_ptr(), npx, d_s.data_ptr(), d_q.data_ptr(), p, d_st.data_ptr())
            torch.cuda.synchronize()
            if rep:
                ms.append(r.last_kernel_ms())
        st = d_st.cpu().numpy()
    med, spread = stats(ms)
    return [{"part": "b", "slots": npx, "reps": reps, "refine_ms_median": med, "refine_ms_spread": spread,
             "jobs_continuing": int(st[0]), "samples_asked": int(st[1])}]


def part_c(S, M, cam, a):
    import torch
    W, H = cam.image_width, cam.image_height
    with N.Renderer(0, 0x5EED, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        ref, _, _ = r.render_frame(cam, a.max, a.depth, want_segments=False)
        render_ms = []
        for _ in range(3):
            r.render_frame(cam, a.max, a.depth, want_segments=False)
            render_ms.append(r.last_kernel_ms())
        ref = ref.astype(np.float64) / a.max
        wall = []
        for f in range(a.frames + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_s, _, d_n, rounds = r.render_adaptive(cam, a.depth, a.rel_error, a.abs_floor, a.min, a.max, a.max)
            torch.cuda.synchronize()
            if f:
                wall.append((time.perf_counter() - t0) * 1e3)
        n = d_n.cpu().numpy().astype(np.float64)
        mean = d_s.cpu().numpy().astype(np.float64) / n[..., None]
        spp_eq = int(np.ceil(n.mean()))
        uni, _, _ = r.render_frame(cam, spp_eq, a.depth, want_segments=False)
        uni_ms = r.last_kernel_ms()
        uni = uni.astype(np.float64) / spp_eq
    med, spread = stats(wall)
    hist = {int(k): int(v) for k, v in zip(*np.unique(n, return_counts=True))}
    return [{"part": "c", "scene": "c3", "precision": "fp32", "width": W, "height": H, "max_depth": a.depth,
             "min_samples": a.min, "max_samples": a.max, "rel_error": a.rel_error, "abs_floor": a.abs_floor,
             "frames": a.frames, "adaptive_wall_ms_median": med, "adaptive_wall_ms_spread": spread, "rounds": rounds,
             "mean_spp": round(float(n.mean()), 3), "n_histogram": hist,
             "rmse_vs_uniform_max": round(float(np.sqrt(np.mean((mean - ref) ** 2))), 6),
             "uniform_max_render_ms_median": stats(render_ms)[0],
             "uniform_equal_spp": spp_eq, "uniform_equal_render_ms": round(uni_ms, 4),
             "uniform_equal_rmse_vs_uniform_max": round(float(np.sqrt(np.mean((uni - ref) ** 2))), 6)}]


def part_t(prec, S, M, cam, a):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    W, H = cam.image_width, cam.image_height
    npx = W * H
    spp = a.denoise_spp
    ctxs, plans = {}, {}
    for name, trav in (("grid", N.RT_TRAV_DEFAULT), ("tree", N.RT_TRAV_DEFAULT & ~N.RT_TRAV_GRID)):
        r = N.Renderer(0, 0x5EED, prec)
        r.set_tuning(traversal=trav)
        r.upload_scene(S, M)
        p = r.pixels_plan(cam)
        assert p.walks_grid == (1 if name == "grid" else 0), (name, p.walks_grid)
        ctxs[name], plans[name] = r, {"traversal": p.traversal, "block": p.block, "lds_bytes": p.lds_bytes,
                                  "walks_grid": {n: r.pixels_plan(cam, c).walks_grid for n, c in
                                                 (("pixels", N.RT_QUERY_PIXELS), ("moments", N.RT_QUERY_MOMENTS),
                                                  ("aov", N.RT_QUERY_AOV))}}
    d_j = torch.from_numpy(jobs_of(np.arange(npx), spp).view(np.uint8)).to("cuda")
    d_s, d_q, d_alb, d_nrm, d_out = (torch.empty((npx, 3), dtype=tdt, device="cuda") for _ in range(5))
    d_z = torch.empty(npx, dtype=tdt, device="cuda")
    d_hits = torch.empty(npx, dtype=torch.int32, device="cuda")
    params = N.Renderer.denoise_params()
    names = ("adaptive_wall", "denoised_total", "denoised_moments", "denoised_aov", "denoised_filter")
    ms = {n: {k: [] for k in ctxs} for n in names}
    shape = {}
    for rep in range(a.reps + 1):   # (the first round warms up)
        for k, r in ctxs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_as, _, d_n, rounds = r.render_adaptive(cam, a.depth, a.rel_error, a.abs_floor, a.min, a.max, a.max)
            torch.cuda.synchronize()
            t = {"adaptive_wall": (time.perf_counter() - t0) * 1e3}
            shape[k] = (rounds, int(d_n.sum(dtype=torch.int64).item()))
            r.render_pixels_moments(cam, d_j.data_ptr(), npx, a.depth, d_s.data_ptr(), d_q.data_ptr())
            t["denoised_moments"] = r.last_kernel_ms()
            r.render_pixels_aov(cam, d_j.data_ptr(), npx, d_alb.data_ptr(), d_nrm.data_ptr(), d_z.data_ptr(), None,
                                d_hits.data_ptr())
            t["denoised_aov"] = r.last_kernel_ms()
            r.denoise(W, H, d_s.data_ptr(), d_out.data_ptr(), d_q.data_ptr(), None, spp, d_alb.data_ptr(),
                      d_nrm.data_ptr(), d_z.data_ptr(), d_hits.data_ptr(), spp, params, None)
            t["denoised_filter"] = r.last_kernel_ms()
            t["denoised_total"] = t["denoised_moments"] + t["denoised_aov"] + t["denoised_filter"]
            torch.cuda.synchronize()
            if rep:
                for n in names:
                    ms[n][k].append(t[n])
    for r in ctxs.values():
        r.close()
    assert shape["grid"] == shape["tree"], shape
    line = {"part": "t", "scene": "c3", "precision": "fp64" if f64 else "fp32", "width": W, "height": H,
            "max_depth": a.depth, "min_samples": a.min, "max_samples": a.max, "rel_error": a.rel_error,
            "abs_floor": a.abs_floor, "denoise_spp": spp, "reps": a.reps, "rounds": shape["grid"][0],
            "mean_spp": round(shape["grid"][1] / npx, 3), "plans": plans}
    for n in names:
        med = {k: float(np.median(v)) for k, v in ms[n].items()}
        spread = {k: float(max(v) - min(v)) for k, v in ms[n].items()}
        for k in med:
            line[f"{n}_{k}_ms_median"], line[f"{n}_{k}_ms_spread"] = round(med[k], 4), round(spread[k], 4)
        line[f"{n}_grid_over_tree"] = round(med["grid"] / med["tree"], 4)
        line[f"{n}_grid_wins"] = bool(med["tree"] - med["grid"] > spread["grid"] + spread["tree"])
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spps", default="2,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--max", type=int, default=256)
    ap.add_argument("--rel-error", type=float, default=0.05)
    ap.add_argument("--abs-floor", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--denoise-spp", type=int, default=16, help="(t) samples per pixel of the denoised frame")
    ap.add_argument("--t-precisions", default="fp32", help="(t) precisions")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rtweekend.reset_stream()
    S, M = api.flatten(scenes.random_spheres())
    cam_api = scenes.main_camera()
    cam_api.image_width = a.width
    cam = cam_api.native
    lines = []

    def emit(new):
        for line in new:
            print(json.dumps(line), flush=True)
        lines.extend(new)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))

    parts = a.parts.split(",")
    if "a" in parts:
        for pname in a.precisions.split(","):
            emit(part_a(N.RT_PREC_F64 if pname == "fp64" else N.RT_PREC_F32, S, M, cam,
                        [int(s) for s in a.spps.split(",")], a.reps, a.depth))
    if "b" in parts:
        emit(part_b(S, M, cam, a.reps, a.depth))
    if "c" in parts:
        emit(part_c(S, M, cam, a))
    if "t" in parts:
        for pname in a.t_precisions.split(","):
            emit(part_t(N.RT_PREC_F64 if pname == "fp64" else N.RT_PREC_F32, S, M, cam, a))


if __name__ == "__main__":
    main()
