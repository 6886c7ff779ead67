#!/usr/bin/env python3
"""CPU count of the candidate tests a depth-ordered candidate loop would skip (round 21,
DESIGN.md §5 and §8).

The fp32 sphere-grid kernels trace a tile's camera rays against the item's candidate list
(rt_batch_cull.h: the spheres of the LDS array the tile's beam can reach), every lane testing
every candidate in ascending record order.  With a conservative near bound per candidate --
no root of any of the tile's rays lies below it -- a wave could leave out every candidate whose
bound is not below the largest closest hit any of its 64 lanes holds so far.  This tool takes
the C3 scene and camera (main.cpp's field at 1920x1080), and for a grid of tiles and a few
samples per tile reproduces the item's list (cull_keep's geometry), the 64 camera rays of a
batch and their hits, and counts per batch:

  tests     the list's length (what the loop runs today)
  sorted    tests left when the list is ordered by the near bound and the loop breaks at the
            first candidate whose bound no lane's tmax exceeds
  unsorted  tests left in ascending record order, each such candidate skipped on its own

The near bound is the header's: a hit at ray parameter lam needs |s - lam L| <= W + lam L k,
so lam >= (s - W) / (L (1 + k)), clamped to >= 0 and truncated to the 20 bits a packed list
word keeps.  A lane whose ray hits nothing (sky) holds tmax = +inf and keeps every candidate
alive for its wave.  Arithmetic is fp64: the margins of the fp32 predicate (2^-17 relative)
move no count here.

python tools/cand_depth_bound.py [--stride 4] [--samples 4] [--json out.json]
"""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from raytracingproject_amd import rtweekend, scenes  # noqa: E402

BIG_RADIUS = 64.0      # rt_scene.h
CAND_CAP = 24          # rt_batch_cull.h BATCH_CAND_CAP
VALU_PER_TEST = 40.0   # miss path + root path of one sphere test (ISSUE / isa_blocks_r19)
VALU_PER_CHECK = 1.0   # the v_cmp against the candidate's bound
BATCHES_PER_LAUNCH = 8.29e6
VALU_PER_LAUNCH = 19.83e9


def field():
    rtweekend.reset_stream()
    w = scenes.random_spheres()
    C = np.array([o.center1 for o in w.objects], float)
    V = np.array([o.center_vec for o in w.objects], float)
    R = np.array([o.radius for o in w.objects], float)
    return C, V, R


def camera(W, H):
    """camera::initialize (camera.h) for main.cpp's camera at W x H."""
    lf, la, vup = np.array([13, 2, 3.0]), np.zeros(3), np.array([0, 1, 0.0])
    fd = 10.0
    vh = 2 * math.tan(math.radians(20) / 2) * fd
    vw = vh * W / H
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(vup, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    du, dv = vw * u / W, -vh * v / H
    p00 = lf - fd * w - vw * u / 2 + vh * v / 2 + 0.5 * (du + dv)
    rad = fd * math.tan(math.radians(0.6 / 2))
    return lf, p00, du, dv, u * rad, v * rad


def trunc20(x):
    """An fp32 value >= 0 with its low 12 mantissa bits cleared (the packed list word)."""
    b = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xfffff000)
    return b.view(np.float32).astype(float)


def roots(o, d, tm, c, cv, r):
    """Nearest root in (0.001, inf) of rays [n, 3] against one sphere; inf: none."""
    f = o - (c + tm[:, None] * cv)
    a = (d * d).sum(1)
    hb = (f * d).sum(1)
    disc = hb * hb - a * ((f * f).sum(1) - r * r)
    sq = np.sqrt(np.maximum(disc, 0))
    t0, t1 = (-hb - sq) / a, (-hb + sq) / a
    return np.where(disc >= 0, np.where(t0 > 1e-3, t0, np.where(t1 > 1e-3, t1, np.inf)), np.inf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stride", type=int, default=4, help="every stride-th tile in x and in y")
    ap.add_argument("--samples", type=int, default=4, help="batches per tile")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = a.width, a.height
    C, V, R = field()
    big = np.abs(R) >= BIG_RADIUS
    Cs, Vs, Rs = C[~big], V[~big], R[~big]
    c, p00, du, dv, ddu, ddv = camera(W, H)
    nrm = np.linalg.norm
    rho = 4 * (nrm(du) + nrm(dv))
    rl = nrm(ddu) + nrm(ddv)
    rb = np.abs(Rs) + nrm(0.5 * Vs, axis=1)
    Cb = Cs + 0.5 * Vs
    rng = np.random.default_rng(1)
    S = a.samples
    n_batch = n_walk = 0
    tests = left_sorted = left_unsorted = 0
    hist = np.zeros(CAND_CAP + 1, int)
    for ty0 in range(0, H, 8 * a.stride):
        for tx0 in range(0, W, 8 * a.stride):
            ax = p00 + (tx0 + 3.5) * du + (ty0 + 3.5) * dv - c
            L = nrm(ax)
            ax /= L
            k = (rl + rho) / L
            q = Cb - c
            sa = q @ ax
            perp = nrm(q - sa[:, None] * ax, axis=1)
            Wd = rb + rl
            keep = ~((sa < -Wd) | (perp > Wd + k / (1 - k) * np.maximum(sa + Wd, 0)))
            lst = np.where(keep)[0]
            if len(lst) > CAND_CAP:
                n_walk += S
                continue
            near = trunc20(np.maximum((sa[lst] - Wd[lst]) / (L * (1 + k)), 0))
            # S batches of 64 rays: pixel (lane & 7, lane >> 3), jitter, disc, time
            n = S * 64
            lane = np.tile(np.arange(64), S)
            px, py = tx0 + (lane & 7), ty0 + (lane >> 3)
            valid = (px < W) & (py < H)
            smp = p00 + (px + rng.random(n) - 0.5)[:, None] * du + (py + rng.random(n) - 0.5)[:, None] * dv
            rr, ang = np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
            o = c + (rr * np.cos(ang))[:, None] * ddu + (rr * np.sin(ang))[:, None] * ddv
            d = smp - o
            tm = rng.random(n)
            tmax0 = np.full(n, np.inf)
            for kb in np.where(big)[0]:
                tmax0 = np.minimum(tmax0, roots(o, d, tm, C[kb], V[kb], R[kb]))
            T = np.stack([roots(o, d, tm, Cs[j], Vs[j], Rs[j]) for j in lst], 0) if len(lst) else np.zeros((0, n))
            for order, srt in ((np.argsort(near, kind="stable"), True), (np.arange(len(lst)), False)):
                tmax = tmax0.copy()
                done = np.zeros(S, bool)   # sorted: the batch's loop has broken
                ran = np.zeros(S, int)
                for i in order:
                    alive = ((tmax > near[i]) & valid).reshape(S, 64).any(1) & ~done
                    if srt:
                        done |= ~alive
                    ran += alive
                    run = np.repeat(alive, 64)
                    tmax = np.where(run, np.minimum(tmax, T[i]), tmax)
                if srt:
                    left_sorted += ran.sum()
                    final = tmax
                else:
                    left_unsorted += ran.sum()
                    # both orders find the closest hit of every lane
                    assert np.array_equal(tmax, final) and np.array_equal(tmax, np.minimum(tmax0, T.min(0, initial=np.inf)))
            tests += S * len(lst)
            hist[len(lst)] += S
            n_batch += S
    per = lambda x: x / n_batch
    out = {
        "width": W, "height": H, "tile_stride": a.stride, "samples_per_tile": S,
        "batches": n_batch, "batches_of_walking_items": n_walk,
        "tests_per_batch": per(tests),
        "sorted_tests_per_batch": per(left_sorted), "sorted_skipped_per_batch": per(tests - left_sorted),
        "unsorted_tests_per_batch": per(left_unsorted), "unsorted_skipped_per_batch": per(tests - left_unsorted),
        "list_length_histogram": hist.tolist(),
    }
    for form in ("sorted", "unsorted"):
        sk, left = out[f"{form}_skipped_per_batch"], out[f"{form}_tests_per_batch"]
        # every candidate reached pays the check; a sorted loop stops paying at its break
        net = sk * VALU_PER_TEST - (left + (1 if form == "sorted" else sk)) * VALU_PER_CHECK
        out[f"{form}_net_valu_per_batch"] = net
        out[f"{form}_share_of_launch"] = net * BATCHES_PER_LAUNCH / VALU_PER_LAUNCH
    out["go_threshold_skipped_per_batch"] = 0.7
    print(json.dumps(out, indent=1))
    if a.json:
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
