#!/usr/bin/env python3
"""rt_denoise on a real frame: what it costs and what it buys (not a test; bench.py is unchanged).

On the C3 scene (random spheres) at `--width` x 9/16 `--width`, per precision, all in one process:
a full-frame job list {p, 0, spp} goes through rt_render_pixels_moments and rt_render_pixels_aov,
then rt_denoise runs on their device outputs.  Launches alternate, `--reps` times each after one
warm-up round; times are rt_last_kernel_ms (the whole call), reported as medians with spreads
(max - min):
  moments, aov      the two renders the filter consumes;
  denoise_k         rt_denoise with iterations = k, k = 0 .. the default's: denoise_0 is prepare +
                    finish, and pass_k = denoise_k - denoise_(k-1) is the pass of step 2^(k-1) (the
                    passes are one kernel; its cost depends on the step through the caches).  A
                    kernel trace (rocprofv3 --kernel-trace --stats on this script) splits prepare
                    from finish;
  floor_copy        a device-to-device copy whose traffic is what one pass must move at least -- one
                    read of both record images and one write, 3 x 4 values per pixel: a copy of 1.5
                    record images (1.5 read, 1.5 written), timed with events.
RMSE against the uniform `--ref-spp` rt_render frame (fp32, a seed of its own, rendered once) of: the noisy mean; the
denoised frame at the default parameters; a uniform rt_render frame whose spp is chosen so that it
takes the time of moments + aov + denoise (its own time is reported beside it).
`--sweep` (fp32) adds the RMSE over a grid of sigma_lum x sigma_depth and over iterations: the
figures the defaults were chosen from.
One JSON line per precision.  There is no pass threshold: the numbers are the finding.

python tools/denoise_probe.py [--width 1920 --spp 16 --reps 5 --sweep --out profiles/denoise_probe.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from raytracingproject_amd import _native as N  # noqa: E402
from raytracingproject_amd import api, rtweekend, scenes  # noqa: E402


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(ref.shape) - ref) ** 2)))


def stats(line, name, v):
    line[f"{name}_ms_median"] = round(float(np.median(v)), 4)
    line[f"{name}_ms_spread"] = round(float(max(v) - min(v)), 4)


def measure(prec, S, M, cam, spp, reps, ref, sweep):
    import torch
    f64 = prec == N.RT_PREC_F64
    tdt = torch.float64 if f64 else torch.float32
    W, H = cam.image_width, cam.image_height
    npx = W * H
    jobs = np.zeros(npx, N.RtPixelJob)
    jobs["pixel"], jobs["sample_count"] = np.arange(npx), spp
    d_jobs = torch.from_numpy(jobs.view(np.uint8)).to("cuda")
    d_s, d_q, d_alb, d_nrm, d_out = (torch.empty((npx, 3), dtype=tdt, device="cuda") for _ in range(5))
    d_z, d_var = (torch.empty(npx, dtype=tdt, device="cuda") for _ in range(2))
    d_hits = torch.empty(npx, dtype=torch.int32, device="cuda")
    # 1.5 record images: 6 values per pixel
    d_src, d_dst = (torch.empty(npx * 6, dtype=tdt, device="cuda") for _ in range(2))
    default = N.Renderer.denoise_params()
    iters = default.iterations
    r = N.Renderer(0, 0x5EED, prec)
    r.upload_scene(S, M)

    def denoise(p):
        r.denoise(W, H, d_s.data_ptr(), d_out.data_ptr(), d_q.data_ptr(), None, spp, d_alb.data_ptr(),
                  d_nrm.data_ptr(), d_z.data_ptr(), d_hits.data_ptr(), spp, p, d_var.data_ptr())

    torch.cuda.synchronize()
    names = ["moments", "aov", "floor_copy"] + [f"denoise_{k}" for k in range(iters + 1)]
    ms = {k: [] for k in names}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps + 1):   # (the first round warms up)
        t = {}
        r.render_pixels_moments(cam, d_jobs.data_ptr(), npx, 50, d_s.data_ptr(), d_q.data_ptr())
        t["moments"] = r.last_kernel_ms()
        r.render_pixels_aov(cam, d_jobs.data_ptr(), npx, d_alb.data_ptr(), d_nrm.data_ptr(), d_z.data_ptr(), None,
                            d_hits.data_ptr())
        t["aov"] = r.last_kernel_ms()
        for k in range(iters + 1):
            denoise(N.Renderer.denoise_params(iterations=k))
            t[f"denoise_{k}"] = r.last_kernel_ms()
        torch.cuda.synchronize()
        e0.record()
        d_dst.copy_(d_src)
        e1.record()
        torch.cuda.synchronize()
        t["floor_copy"] = e0.elapsed_time(e1)
        if rep:
            for k, v in t.items():
                ms[k].append(v)
    line = {"scene": "c3", "precision": "fp64" if f64 else "fp32", "width": W, "height": H, "spp": spp, "reps": reps,
            "params": {f: getattr(default, f) for f, _ in N.RtDenoiseParams._fields_},
            "record_image_mb": round(npx * 4 * (8 if f64 else 4) / 1e6, 3)}
    for k in names:
        stats(line, k, ms[k])
    for k in range(1, iters + 1):
        stats(line, f"pass_{k}", [a - b for a, b in zip(ms[f"denoise_{k}"], ms[f"denoise_{k - 1}"])])
    total = [a + b + c for a, b, c in zip(ms["moments"], ms["aov"], ms[f"denoise_{iters}"])]
    stats(line, "render_aov_denoise", total)
    line["denoise_over_moments"] = round(line[f"denoise_{iters}_ms_median"] / line["moments_ms_median"], 4)
    passes = (line[f"denoise_{iters}_ms_median"] - line["denoise_0_ms_median"]) / max(iters, 1)
    line["pass_over_floor_copy"] = round(passes / line["floor_copy_ms_median"], 3)

    # what it buys: the frames the loop left in the buffers are the default parameters' (k = iters)
    torch.cuda.synchronize()
    s = d_s.cpu().numpy()
    line["rmse_noisy"] = round(rmse(s / s.dtype.type(spp), ref), 6)
    line["rmse_denoised"] = round(rmse(d_out.cpu().numpy(), ref), 6)
    # a uniform frame for the same time: scale spp by the measured time of a uniform spp-sample frame
    r.render_frame(cam, spp, 50, want_segments=False)
    r.render_frame(cam, spp, 50, want_segments=False)
    t_uniform = r.last_kernel_ms()
    eq = max(1, int(spp * line["render_aov_denoise_ms_median"] / t_uniform))
    sums, _, _ = r.render_frame(cam, eq, 50, want_segments=False)
    line.update(uniform_ms_at_spp=round(t_uniform, 4), equal_time_spp=eq, equal_time_ms=round(r.last_kernel_ms(), 4),
                rmse_equal_time_uniform=round(rmse(sums / sums.dtype.type(eq), ref), 6))
    if sweep:
        grid = []
        for sl in (1.0, 2.0, 4.0, 8.0, 16.0):
            for sd in (0.01, 0.05, 0.25):
                denoise(N.Renderer.denoise_params(sigma_lum=sl, sigma_depth=sd))
                torch.cuda.synchronize()
                grid.append({"sigma_lum": sl, "sigma_depth": sd, "rmse": round(rmse(d_out.cpu().numpy(), ref), 6)})
        line["sweep_sigma"] = grid
        its = []
        for k in range(0, 9):
            denoise(N.Renderer.denoise_params(iterations=k))
            torch.cuda.synchronize()
            its.append({"iterations": k, "rmse": round(rmse(d_out.cpu().numpy(), ref), 6)})
        line["sweep_iterations"] = its
        pw = []
        for k in (0, 3, 5, 7, 10):
            denoise(N.Renderer.denoise_params(normal_log2_power=k))
            torch.cuda.synchronize()
            pw.append({"normal_log2_power": k, "rmse": round(rmse(d_out.cpu().numpy(), ref), 6)})
        line["sweep_normal_power"] = pw
    r.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--sweep", action="store_true", help="fp32: RMSE over sigma_lum x sigma_depth, iterations, normal power")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rtweekend.reset_stream()
    S, M = api.flatten(scenes.random_spheres())
    cam_api = scenes.main_camera()
    cam_api.image_width = a.width
    cam = cam_api.native
    # (a seed of its own: the reference shares no sample with the frames it judges)
    with N.Renderer(0, 0x5EED + 1, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        sums, _, _ = r.render_frame(cam, a.ref_spp, 50, want_segments=False)
    ref = sums.reshape(-1, 3).astype(np.float64) / a.ref_spp
    lines = []
    for pname in a.precisions.split(","):
        f64 = pname == "fp64"
        line = measure(N.RT_PREC_F64 if f64 else N.RT_PREC_F32, S, M, cam, a.spp, a.reps, ref, a.sweep and not f64)
        line["ref_spp"] = a.ref_spp
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
