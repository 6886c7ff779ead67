// rt_moments.h -- per-job second moments (rt_render_pixels_moments) and the device side of an
// adaptive sampler's round (rt_refine_jobs).
//
// rt_render_pixels_moments is rt_render_pixels (rt_pixels.h: the same jobs, flat sample list,
// offsets and passes) with one more output per job and channel, the sum of squares of the
// job's per-sample radiance.  It shares that call's device code but for one kernel:
//   * fp32: pixels_moments_kernel is pixels_kernel<float, false, ...> -- the same path_loop
//     (rt_radiance.h), px_sample_start and fix_sample -- whose finished path also adds r^2,
//     r = rintf(L 2^19) the integer its sum already rounds to (fix_sample hands it back), to the job's second
//     moment: an exact integer below 2^64 in units of 2^-38, split into its low and high 32 bits
//     and added to two 64-bit words (sq[(job * 3 + c) * 2 + {0 low, 1 high}]) with plain integer
//     atomics -- order-free, no carry between the words, neither can overflow within 2^31
//     samples.  |r| >= 2^32 or a NaN sets the channel's bits in sqflags instead (SQ_NAN, SQ_INF:
//     two bits per channel).  The words are seeded and finalized by kernels in
//     rt_render_f64.hip (no contraction), as the sums' are.
//   * fp64: the stored 28-byte sample records already hold L, so the path kernel is
//     pixels_kernel's own, and the reduction is pixels_reduce_kernel<R, true>, which also adds
//     L L per channel in sample order, each product rounded on its own.
#pragma once
#include "rt_pixels.h"

namespace rtx {

constexpr uint32_t SQ_NAN = 1u, SQ_INF = 2u;   // per channel c: << (2 * c)

// (dmul_rn: rt_pixels.h) -- the difference, rounded, as the product is there
__device__ __forceinline__ double dsub_rn(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}

// pixels_kernel (rt_pixels.h), fp32, with the second moment.  acc, flags, segs_out as there; sq
// (num_jobs x 3 x 2 words) and sqflags (num_jobs) are added to.
template <int BLOCK, int MINW, int TRAV, bool MESH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(MINW))) void pixels_moments_kernel(
    RenderParams P, const PixelJob* __restrict__ jobs, const unsigned long long* __restrict__ offsets, int num_jobs,
    unsigned long long total, unsigned long long q_begin, int n, unsigned long long* __restrict__ acc,
    uint32_t* __restrict__ flags, uint32_t* __restrict__ segs_out, unsigned long long* __restrict__ sq,
    uint32_t* __restrict__ sqflags) {
    int job = 0;   // this lane's path is a sample of job `job`
    path_loop<float, false, BLOCK, TRAV, MESH>(
        P, n,
        [&](unsigned long long i, Ray<float>& ray, CounterRng& rng) {
            job = px_sample_start<float>(P, jobs, offsets, num_jobs, total, q_begin + i, rng, ray);
        },
        [&](const V3<float>& L, uint32_t segs) {
            // pixels_kernel's sum, then r^2 as two 32-bit halves (or a flag)
            uint32_t fl = 0, qf = 0;
            const float l[3] = {L.x, L.y, L.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float r;
                if (const long long s = fix_sample(l[c], c, fl, &r))
                    atomicAdd(acc + (size_t)job * 3 + c, (unsigned long long)s);
                const float ar = fabsf(r);
                if (ar < 0x1p32f) {
                    const unsigned long long a = (unsigned long long)ar, s = a * a;
                    unsigned long long* w = sq + ((size_t)job * 3 + c) * 2;
                    if (s & 0xffffffffull) atomicAdd(w, s & 0xffffffffull);
                    if (s >> 32) atomicAdd(w + 1, s >> 32);
                } else {   // NaN, inf, or a sample at or beyond 2^13
                    qf |= (r != r ? SQ_NAN : SQ_INF) << (2 * c);
                }
            }
            if (fl) atomicOr(flags + job, fl);
            if (qf) atomicOr(sqflags + job, qf);
            if (segs_out) atomicAdd(segs_out + job, segs);
        });
}

// rt_refine_jobs: one thread per job slot rewrites jobs[k] for the next round (the rule is in
// include/rt_hip.h); fp64 throughout, each operation rounded once in the written order.
// stats[0] += slots with next > 0, stats[1] += their next, one pair of atomics per workgroup
// (stats zeroed on the stream by the caller).
struct AdaptiveParams {   // = rt_adaptive_params (include/rt_hip.h)
    double rel_error, abs_floor;
    uint32_t min_samples, max_samples, max_step, pad;
};
static_assert(sizeof(AdaptiveParams) == 32, "rt_adaptive_params");

template <class R>
__global__ void refine_jobs_kernel(PixelJob* __restrict__ jobs, int num_jobs, const R* __restrict__ sums,
                                   const R* __restrict__ sumsq, AdaptiveParams A,
                                   unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_stat[2];
    if (threadIdx.x < 2) s_stat[threadIdx.x] = 0;
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < num_jobs) {
        const PixelJob jb = jobs[k];
        const unsigned long long n = (unsigned long long)jb.sample_begin + jb.sample_count;
        unsigned long long next;
        if (n >= A.max_samples) {
            next = 0;
        } else if (n < A.min_samples) {
            next = A.min_samples - n;
        } else {
            bool converged = true;
            double s[3], q[3];
            for (int c = 0; c < 3; ++c) {
                s[c] = (double)sums[(size_t)k * 3 + c];
                q[c] = (double)sumsq[(size_t)k * 3 + c];
                if (!__builtin_isfinite(s[c]) || !__builtin_isfinite(q[c])) converged = false;
            }
            if (converged) {
                const double nd = (double)n;
                double m[3], v[3];
                for (int c = 0; c < 3; ++c) {
                    m[c] = s[c] / nd;
                    const double d = dsub_rn(q[c], dmul_rn(s[c], m[c]));
                    v[c] = d > 0.0 ? d / dsub_rn(nd, 1.0) : 0.0;
                }
                const double e2 = ((v[0] + v[1]) + v[2]) / dmul_rn(3.0, nd);
                const double mean = ((m[0] + m[1]) + m[2]) / 3.0;
                const double am = fabs(mean), a = am > A.abs_floor ? am : A.abs_floor;
                const double t = dmul_rn(A.rel_error, a);
                converged = e2 <= dmul_rn(t, t);
            }
            if (converged) {
                next = 0;
            } else {
                const unsigned long long left = (unsigned long long)A.max_samples - n;
                next = n < left ? n : left;
                next = next < A.max_step ? next : A.max_step;
            }
        }
        PixelJob o;
        o.pixel = jb.pixel;
        o.sample_begin = (uint32_t)n;
        o.sample_count = (uint32_t)next;
        o.pad = 0;
        jobs[k] = o;
        if (next) {
            atomicAdd(&s_stat[0], 1ull);
            atomicAdd(&s_stat[1], next);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_stat[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_stat[threadIdx.x]);
}

}  // namespace rtx
