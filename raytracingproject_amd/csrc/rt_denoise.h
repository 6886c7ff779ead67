// rt_denoise.h -- rt_denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; the
// spatial half of SVGF, Schied et al. 2017) over the per-pixel sums, second moments and first-hit
// guides the job calls write (rt_pixels.h, rt_moments.h, rt_aov.h).  The rule is in
// include/rt_hip.h: IEEE + - x / sqrt and comparisons only, every operation rounded once in the
// written order, so tests/denoise_ref.py restates it bit for bit in either precision.  This
// header is compiled without contraction, with IEEE division and square root and with denormals
// kept (rt_denoise.hip): the fp32 normal weight reaches 2^-128.
//
// Three kernels on T (float | double), over row-major width x height images, pixel p = y W + x:
//   * denoise_prepare_kernel, one thread per pixel: sums / n demodulated by the albedo into the
//     colour record {c0, c1, c2, V} (V: the variance of the mean of the channel average) and the
//     guides into the guide record {n^x, n^y, n^z, z}; records are 4 T, 16-byte (fp64: 32-byte)
//     aligned, so each arrives in one b128 load (fp64: two).  Without second moments V is the
//     variance of L over the 3x3 window: denoise_spatial_variance_kernel, a second launch, reads
//     the colours of the first and writes only V.
//   * denoise_atrous_kernel, one pass of step s: a 64 x 4 workgroup, one wave per 64 consecutive
//     pixels of a row, so that each of the 25 taps of a wave is one contiguous row segment of each
//     record image.  Reads src and the guide, writes dst (the two colour images ping-pong).  No
//     atomics, no LDS.
//   * denoise_finish_kernel, one thread per pixel: out = c a, out_variance = V; the albedo floor
//     a is recomputed from the guides as prepare did, so nothing is kept for it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rtx {

template <class T>
struct DnVec;
template <>
struct DnVec<float> {
    using type = float4;
};
template <>
struct DnVec<double> {
    using type = double4;
};
static_assert(sizeof(float4) == 16 && alignof(float4) == 16 && sizeof(double4) == 32, "denoise records");

// The inputs prepare and finish read.
template <class T>
struct DenoiseArgs {
    int W, H;
    int samples, guide_samples;
    const T* sums;
    const T* sumsq;           // may be null: the spatial variance
    const uint32_t* counts;   // may be null: n = samples
    const T* albedo;          // may be null (with hits)
    const uint32_t* hits;
    const T* normal;          // may be null
    const T* depth;           // may be null
};

constexpr int DN_BLOCK_X = 64, DN_BLOCK_Y = 4;

// a_c = max((albedo_c + (T)(guide_samples - hits)) / (T)guide_samples, 1/64); 1 without albedo
template <class T>
__device__ __forceinline__ void dn_albedo(const DenoiseArgs<T>& A, size_t p, T a[3]) {
#pragma clang fp contract(off)
    if (!A.albedo) {
        a[0] = a[1] = a[2] = (T)1;
        return;
    }
    const T sky = (T)((long long)A.guide_samples - (long long)A.hits[p]), gs = (T)A.guide_samples;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T v = (A.albedo[p * 3 + c] + sky) / gs;
        a[c] = v > (T)0.015625 ? v : (T)0.015625;
    }
}

__device__ __forceinline__ float dn_sqrt(float v) { return __builtin_sqrtf(v); }
__device__ __forceinline__ double dn_sqrt(double v) { return __builtin_sqrt(v); }

template <class T>
__device__ __forceinline__ T dn_lum(T c0, T c1, T c2) {
#pragma clang fp contract(off)
    return ((c0 + c1) + c2) / (T)3;
}

template <class T>
__global__ void denoise_prepare_kernel(DenoiseArgs<T> A, typename DnVec<T>::type* __restrict__ col,
                                       typename DnVec<T>::type* __restrict__ guide) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)A.W * (size_t)A.H) return;
    const uint32_t n = A.counts ? A.counts[p] : (uint32_t)A.samples;
    const T nT = (T)n;
    T a[3], s[3], m[3], c[3];
    dn_albedo(A, p, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = A.sums[p * 3 + k];
        m[k] = n > 0 ? s[k] / nT : (T)0;
        c[k] = m[k] / a[k];
    }
    T V = (T)0;
    if (A.sumsq && n >= 2) {
        const T n1 = (T)(n - 1u);
        T v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T d = A.sumsq[p * 3 + k] - s[k] * m[k];
            const T vk = d > (T)0 ? d / n1 : (T)0;
            v[k] = vk / (a[k] * a[k]);
        }
        V = ((v[0] + v[1]) + v[2]) / ((T)3 * nT);
    }
    typename DnVec<T>::type rc, rg;
    rc.x = c[0], rc.y = c[1], rc.z = c[2], rc.w = V;
    rg.x = rg.y = rg.z = (T)0;
    if (A.normal) {
        const T n0 = A.normal[p * 3], n1 = A.normal[p * 3 + 1], n2 = A.normal[p * 3 + 2];
        const T d = (n0 * n0 + n1 * n1) + n2 * n2;
        if (d > (T)0) {
            const T r = dn_sqrt(d);
            rg.x = n0 / r, rg.y = n1 / r, rg.z = n2 / r;
        }
    }
    rg.w = A.depth ? A.depth[p] : (T)0;
    col[p] = rc;
    guide[p] = rg;
}

// No second moments: V = max(0, mu2 - mu mu) of L over the in-image cells of the 3x3 window, in
// row-major order.  Reads the colours (x, y, z) of the records, writes only w.
template <class T>
__global__ void denoise_spatial_variance_kernel(int W, int H, T* __restrict__ col) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * (size_t)H) return;
    const long long x = (long long)(p % (size_t)W), y = (long long)(p / (size_t)W);
    T s1 = (T)0, s2 = (T)0;
    int k = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const long long qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const long long qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const T* r = col + ((size_t)qy * (size_t)W + (size_t)qx) * 4;
            const T L = dn_lum(r[0], r[1], r[2]);
            s1 = s1 + L;
            s2 = s2 + L * L;
            ++k;
        }
    }
    const T kT = (T)k, mu = s1 / kT, mu2 = s2 / kT, d = mu2 - mu * mu;
    col[p * 4 + 3] = d > (T)0 ? d : (T)0;
}

// One pass of step `step` (the rule: include/rt_hip.h).  A workgroup is DN_BLOCK_X x DN_BLOCK_Y
// pixels; workgroup b covers tile (b % tiles_x, b / tiles_x).
template <class T>
__global__ __launch_bounds__(DN_BLOCK_X* DN_BLOCK_Y) void denoise_atrous_kernel(
    int W, int H, int tiles_x, int step, int normal_log2_power, T sigma_depth, T sigma_lum, T lum_eps,
    const typename DnVec<T>::type* __restrict__ src, const typename DnVec<T>::type* __restrict__ guide,
    typename DnVec<T>::type* __restrict__ dst) {
#pragma clang fp contract(off)
    using V4 = typename DnVec<T>::type;
    const long long x = (long long)(blockIdx.x % (unsigned)tiles_x) * DN_BLOCK_X + (threadIdx.x & (DN_BLOCK_X - 1));
    const long long y = (long long)(blockIdx.x / (unsigned)tiles_x) * DN_BLOCK_Y + (threadIdx.x / DN_BLOCK_X);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    // the variance under the 3x3 Gaussian, normalised over the cells inside the image
    T vs = (T)0, gs = (T)0;
    for (int dy = -1; dy <= 1; ++dy) {
        const long long qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const long long qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const T g = (dx == 0 ? (T)0.5 : (T)0.25) * (dy == 0 ? (T)0.5 : (T)0.25);
            vs = vs + g * src[(size_t)qy * (size_t)W + (size_t)qx].w;
            gs = gs + g;
        }
    }
    const T den = sigma_lum * dn_sqrt(vs / gs) + lum_eps;
    const V4 cp = src[p], gp = guide[p];
    const T Lp = dn_lum(cp.x, cp.y, cp.z);
    const bool p_flat = gp.x == (T)0 && gp.y == (T)0 && gp.z == (T)0;
    const bool p_inf = __builtin_isinf(gp.w);
    T Sw = (T)0, S0 = (T)0, S1 = (T)0, S2 = (T)0, Sv = (T)0;
    for (int dy = -2; dy <= 2; ++dy) {
        const long long qy = y + (long long)dy * step;
        if (qy < 0 || qy >= H) continue;
        const T hy = dy == 0 ? (T)0.375 : (dy == 1 || dy == -1) ? (T)0.25 : (T)0.0625;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const long long qx = x + (long long)dx * step;
            if (qx < 0 || qx >= W) continue;
            const T hx = dx == 0 ? (T)0.375 : (dx == 1 || dx == -1) ? (T)0.25 : (T)0.0625;
            const T k = hx * hy;
            const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
            const V4 cq = src[q];
            T w = k;
            if (dx != 0 || dy != 0) {
                const V4 gq = guide[q];
                T wn = (T)1;
                if (!(p_flat && gq.x == (T)0 && gq.y == (T)0 && gq.z == (T)0)) {
                    const T d = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                    wn = d > (T)0 ? d : (T)0;
                    for (int i = 0; i < normal_log2_power; ++i) wn = wn * wn;
                }
                if (gp.w != gq.w && (p_inf || __builtin_isinf(gq.w))) {
                    w = (T)0;
                } else {
                    T xz = (T)0;
                    if (gp.w != gq.w) {
                        const T dz = gp.w - gq.w, zmin = gp.w < gq.w ? gp.w : gq.w;
                        xz = (dz < (T)0 ? -dz : dz) / (sigma_depth * zmin);
                    }
                    const T dl = Lp - dn_lum(cq.x, cq.y, cq.z);
                    const T xl = (dl < (T)0 ? -dl : dl) / den;
                    const T u1 = (T)1 - (xz + xl) * (T)0.125;
                    T u = u1 > (T)0 ? u1 : (T)0;
                    u = u * u;
                    u = u * u;
                    u = u * u;
                    w = (k * wn) * u;
                }
            }
            Sw = Sw + w;
            S0 = S0 + w * cq.x;
            S1 = S1 + w * cq.y;
            S2 = S2 + w * cq.z;
            Sv = Sv + (w * w) * cq.w;
        }
    }
    V4 o;
    o.x = S0 / Sw, o.y = S1 / Sw, o.z = S2 / Sw, o.w = Sv / (Sw * Sw);
    dst[p] = o;
}

template <class T>
__global__ void denoise_finish_kernel(DenoiseArgs<T> A, const typename DnVec<T>::type* __restrict__ col,
                                      T* __restrict__ out, T* __restrict__ out_variance) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)A.W * (size_t)A.H) return;
    T a[3];
    dn_albedo(A, p, a);
    const typename DnVec<T>::type c = col[p];
    out[p * 3] = c.x * a[0];
    out[p * 3 + 1] = c.y * a[1];
    out[p * 3 + 2] = c.z * a[2];
    if (out_variance) out_variance[p] = c.w;
}

}  // namespace rtx
