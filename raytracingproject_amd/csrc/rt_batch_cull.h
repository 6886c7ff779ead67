// rt_batch_cull.h -- which spheres can the camera rays of one 8x8 tile hit?  One predicate,
// shared by the fp32 sphere-grid kernels (render_coherent's per-item candidate list) and the
// CPU driver that checks it against brute force (tests/cpp/batch_cull_driver.cpp).
//
// Geometry.  c: camera centre; m = pixel00 + (tx0 + 3.5) du + (ty0 + 3.5) dv: the tile's
// middle on the focus plane; a = m - c, L = |a|.  A camera ray of the tile starts at
// o = c + x ddu + y ddv (x^2 + y^2 < 1, so |o - c| <= R_l = |ddu| + |ddv|; 0 without defocus)
// and runs through s = m + e du + f dv with |e|, |f| <= 3.5 + 0.5 (pixel centres, jitter), so
// |s - m| <= rho = 4 (|du| + |dv|).  Its point at parameter lam >= 0 is (1 - lam) o + lam s,
// within D(lam) = |1 - lam| R_l + lam rho <= R_l + lam (R_l + rho) of the axis point c + lam a.
// A sphere moving from C to C + cv over the shutter (ray times lie in [0, 1)) stays inside the
// ball Cb = C + cv / 2, rb = |r| + |cv| / 2.  With q = Cb - c split along the axis, s = q.a / L
// and perp = |q - s a / L|, W = rb + R_l and k = (R_l + rho) / L, a hit at lam means
//   |s - lam L| <= rb + D(lam)  and  perp <= rb + D(lam) <= W + lam L k,
// the first of which gives lam L (1 - k) <= s + W, so (k < 1)
//   s >= -W   and   perp <= W + k / (1 - k) max(s + W, 0).
// A sphere is dropped only when one of the two fails.
//
// Rounding (u = 2^-24; everything below is fp32, with or without FMA contraction, and with
// the device's approximate rcp / sqrt, a few u each).  Every bound is widened so that it
// holds for the rays the kernel really traces and for the kernel's own fp32 sphere test:
//  * scale = |c|_1 + |pixel00|_1 + (tx0 + 8) |du|_1 + (ty0 + 8) |dv|_1 + |ddu|_1 + |ddv|_1
//    bounds every intermediate of camera_ray_lds and of m above.  m (two FMAs per component)
//    is off by < 4 u scale; the kernel's pixel sample (five operations), origin (two) and
//    direction s - o (one) by < 9, 4 and 2 u scale as vectors' lengths.  Taking the rounded m
//    as the axis point, all of it is a displacement of s and o: rho and R_l each grow by
//    E = CULL_EPS_CAM scale = 32 u scale.
//  * per sphere: Cb, q, s, the projection q - s ax (ax = a / L is a unit vector to 4 u) and
//    the two norms are each good to a few u |q|: together < 16 u |q| on s and on perp --
//    perp comes from the projected vector, not from |q|^2 - s^2, whose cancellation would
//    cost sqrt(u) |q|, so the bound is relative at any distance: |q| up to GridHdr::far_o
//    and beyond, until |q|^2 overflows to +inf, which keeps the sphere.
//  * the kernel's test (sphere_root, fp32) takes disc = r^2 - |l|^2 >= 0 for a hit, l the
//    closest-approach vector, known to |dl| < 16 u (|o| + |C|): it can report a ray that
//    passes the sphere at up to r + 2 |dl| + 4 u r.  |o| <= |c| + R_l and |C| <= |q| + |c| +
//    rb: < 64 u (|q| + scale + rb).
//    Together mg = CULL_EPS (|q| + scale + rb) = 128 u (...) is added to W.
//  * k, 1 - k (k <= 7/8: its difference from 1 is good to 8 u), their quotient and the final
//    sum each carry a factor CULL_UP = 1 + 2^-19; k > 7/8 (or L = 0, or a NaN anywhere in the
//    camera words) keeps every sphere.
// Both comparisons are written so that a NaN keeps the sphere.
//
// The near bound (r21, cull_near).  A ray's parameter lam is the kernel's t: it traces
// o + t (sample - o).  The first condition above also bounds a hit from below:
//   lam L >= s - rb - D(lam) >= s - W - lam L k,   so   lam >= (s - W) / (L (1 + k)):
// no camera ray of the tile reaches the sphere before that parameter, at any time in [0, 1).
// A candidate list ordered by this bound can stop at the first candidate whose bound lies
// beyond every lane's closest hit (rt_device.h closest_hit CAND).
// Rounding: the bound has to hold for the root the kernel's sphere_root reports, not for the
// exact one, so the point the kernel takes for the hit may lie off the sphere by eps, and the
// condition reads |s - lam L| <= rb + D(lam) + eps.  eps has two parts:
//  * what the margin mg above already covers: the displaced ray (E), s and q (16 u |q|), and
//    the root's own relative error -- the pair c / q, q / a and the approximate rcp are good
//    to a few u of the root, a distance of a few u (|q| + rb) along the ray; c = |f|^2 - r^2
//    cancels where the origin lies near the surface, to 4 u |f|^2 / (2 |f|), the same order;
//  * the discriminant.  disc = r^2 - |l|^2 carries |d disc| < 32 u r (|o| + |C|) + 4 u r^2
//    (dl above), and the half chord sqrt(disc) it yields is off by at most sqrt(|d disc|)
//    -- all of it near grazing, where disc is small and the error passes through the square
//    root.  The far root moves by that distance, and the near root c / q by the same relative
//    amount, less in distance.  sqrt(|d disc|) < sqrt(64 u rb (|q| + scale + rb))
//    = 2^-9 sqrt(rb (...)); G = CULL_SQ sqrt(rb (|q| + scale + rb)) with CULL_SQ = 2^-8 is
//    taken off as well.  (A ray that misses the exact sphere and is reported as a hit has
//    disc within d disc of zero: the same bound on the point it reports.)
//  * nd = 1 / (L (1 + k)) is rounded down by CULL_UP^2 (iL, the sum, the quotient: a few u
//    each), the product by CULL_DN = 1 - 2^-19; the result is clamped to >= 0, and is 0 for a
//    NaN anywhere and for a beam that drops nothing (!ok).
//  * packing (cand_pack) clears the low 12 bits of the fp32 pattern: for a value >= 0 that
//    is truncation toward zero, downward.
// So cull_near, before and after packing, is at most every root sphere_root reports.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_scene.h"

namespace rtx {

// candidates one item's list holds (byte offsets of sphere records); more: the item walks
constexpr int BATCH_CAND_CAP = 24;
// LDS per wave: the list, then its count (word BATCH_CAND_CAP), padded
constexpr size_t BATCH_CAND_BYTES = 128;
static_assert((BATCH_CAND_CAP + 1) * 4 <= BATCH_CAND_BYTES, "candidate list");

// tests/cpp/batch_cull_driver.cpp only: 1 shrinks the rounding margins to nothing, 2 drops
// the lens radius, 3 drops the motion's half-length -- each must make the driver fail
// (tests/cpp/cand_depth_driver.cpp: the same three, and 4: the packed bound rounded up)
#ifndef RT_CULL_MUTATE
#define RT_CULL_MUTATE 0
#endif
#if RT_CULL_MUTATE == 1
constexpr float CULL_EPS = 0x1p-29f, CULL_EPS_CAM = 0x1p-31f, CULL_UP = 1.f;
constexpr float CULL_SQ = 0x1p-20f, CULL_DN = 1.f;
#else
constexpr float CULL_EPS = 0x1p-17f, CULL_EPS_CAM = 0x1p-19f, CULL_UP = 1.f + 0x1p-19f;
constexpr float CULL_SQ = 0x1p-8f, CULL_DN = 1.f - 0x1p-19f;
#endif
// a packed list word (r21): the near bound's upper 20 bits over the record's index in the LDS
// sphere array (< 4096: rt_scene.h's limits, asserted where the list is built)
constexpr uint32_t CAND_IDX_BITS = 12, CAND_IDX_MASK = (1u << CAND_IDX_BITS) - 1u;

// what the tile's rays share: the axis (from c along the unit vector ax), the widened lens
// radius, k / (1 - k), the scale of the camera words; ok: a sphere may be dropped at all;
// nd: 1 / (L (1 + k)) rounded down (cull_near)
struct CullBeam {
    float c[3], ax[3];
    float rl, g, scale;
    bool ok;
    float nd;
};

// cam: CohConst::cam (f_center, f_p00, f_du, f_dv, f_ddu, f_ddv); (tx0, ty0): the tile's
// top-left pixel
RT_HD inline CullBeam cull_beam(const float* cam, int defocus, int tx0, int ty0) {
    auto nrm = [](const float* v) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto l1 = [](const float* v) { return fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]); };
    const float* c = cam;
    const float *p00 = cam + 3, *du = cam + 6, *dv = cam + 9, *ddu = cam + 12, *ddv = cam + 15;
    const float fx = (float)tx0 + 3.5f, fy = (float)ty0 + 3.5f;
    CullBeam b;
    float a[3];
    for (int k = 0; k < 3; ++k) {
        b.c[k] = c[k];
        a[k] = (p00[k] + fx * du[k] + fy * dv[k]) - c[k];
    }
    const float L = nrm(a);
    const float iL = 1.f / L;
    for (int k = 0; k < 3; ++k) b.ax[k] = a[k] * iL;
    b.scale = l1(c) + l1(p00) + (fx + 4.5f) * l1(du) + (fy + 4.5f) * l1(dv) + l1(ddu) + l1(ddv);
    const float E = CULL_EPS_CAM * b.scale;
    const float rho = 4.f * (nrm(du) + nrm(dv)) * CULL_UP + E;
#if RT_CULL_MUTATE == 2
    b.rl = E;
#else
    b.rl = (defocus ? nrm(ddu) + nrm(ddv) : 0.f) * CULL_UP + E;
#endif
    const float k = (b.rl + rho) * iL * CULL_UP;
    b.ok = k <= 0.875f;   // (false for NaN and for L = 0)
    b.g = k / (1.f - k) * CULL_UP * CULL_UP;
    b.nd = iL / ((1.f + k) * CULL_UP * CULL_UP);
    return b;
}

// false only where no camera ray of the beam's tile can hit the sphere, at any time in [0, 1)
RT_HD inline bool cull_keep(const CullBeam& b, const SphereF& s) {
    const float hx = 0.5f * s.cv[0], hy = 0.5f * s.cv[1], hz = 0.5f * s.cv[2];
#if RT_CULL_MUTATE == 3
    const float rb = fabsf(s.r);
#else
    const float rb = fabsf(s.r) + sqrtf(hx * hx + hy * hy + hz * hz) * CULL_UP;
#endif
    const float qx = (s.c[0] + hx) - b.c[0], qy = (s.c[1] + hy) - b.c[1], qz = (s.c[2] + hz) - b.c[2];
    const float qn = sqrtf(qx * qx + qy * qy + qz * qz);
    const float sa = qx * b.ax[0] + qy * b.ax[1] + qz * b.ax[2];
    const float px = qx - sa * b.ax[0], py = qy - sa * b.ax[1], pz = qz - sa * b.ax[2];
    const float perp = sqrtf(px * px + py * py + pz * pz);
    const float W = (rb + b.rl) + CULL_EPS * (qn + b.scale + rb);
    const float bound = (W + b.g * fmaxf(sa + W, 0.f)) * CULL_UP;
    const bool behind = sa < -W, outside = perp > bound;   // (false for NaN)
    return !b.ok || !(behind || outside);
}

// at most every root the kernel's fp32 sphere test reports for a camera ray of the beam's tile
// against the sphere, at any time in [0, 1); >= 0, and 0 where nothing is known (the text above)
RT_HD inline float cull_near(const CullBeam& b, const SphereF& s) {
    const float hx = 0.5f * s.cv[0], hy = 0.5f * s.cv[1], hz = 0.5f * s.cv[2];
#if RT_CULL_MUTATE == 3
    const float rb = fabsf(s.r);
#else
    const float rb = fabsf(s.r) + sqrtf(hx * hx + hy * hy + hz * hz) * CULL_UP;
#endif
    const float qx = (s.c[0] + hx) - b.c[0], qy = (s.c[1] + hy) - b.c[1], qz = (s.c[2] + hz) - b.c[2];
    const float qn = sqrtf(qx * qx + qy * qy + qz * qz);
    const float sa = qx * b.ax[0] + qy * b.ax[1] + qz * b.ax[2];
    const float W = (rb + b.rl) + CULL_EPS * (qn + b.scale + rb);
    const float G = CULL_SQ * sqrtf(rb * (qn + b.scale + rb));
    const float near = ((sa - W) - G) * b.nd * CULL_DN;
    return b.ok && near > 0.f ? near : 0.f;   // (0 for NaN)
}

// the list word of record k with near bound `near` (>= 0), and its two halves
RT_HD inline uint32_t cand_pack(float near, uint32_t k) {
    uint32_t u;
    memcpy(&u, &near, 4);
#if RT_CULL_MUTATE == 4
    u += CAND_IDX_MASK;
#endif
    return (u & ~CAND_IDX_MASK) | k;
}
RT_HD inline float cand_near(uint32_t w) {
    w &= ~CAND_IDX_MASK;
    float f;
    memcpy(&f, &w, 4);
    return f;
}
RT_HD inline uint32_t cand_index(uint32_t w) { return w & CAND_IDX_MASK; }
// a word's place in the ascending order of the n list words: how many are smaller.  The words
// differ in their index bits, so the places are a permutation, ordered by (near, index).
RT_HD inline uint32_t cand_rank(const uint32_t* words, uint32_t n, uint32_t w) {
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) r += words[j] < w;
    return r;
}

// the predicate as one call: cam words, tile, sphere record
RT_HD inline bool batch_cull_keep(const float* cam, int defocus, int tx0, int ty0, const SphereF& s) {
    return cull_keep(cull_beam(cam, defocus, tx0, ty0), s);
}

}  // namespace rtx
