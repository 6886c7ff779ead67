// rt_moments.h -- per-job second moments (rt_render_pixels_moments) and the device side of an
// adaptive sampler's round (rt_refine_jobs).
//
// rt_render_pixels_moments is rt_render_pixels (rt_pixels.h: the same jobs, flat sample list,
// offsets and passes) with one more output per job and channel, the sum of squares of the
// job's per-sample radiance.  Everything here is a sibling of a kernel there, so that kernel's
// instantiations stay what they were:
//   * fp32: pixels_moments_kernel is pixels_kernel<float, false, ...> whose finished path also
//     adds r^2, r = rintf(L 2^19) the integer its sum already rounds to, to the job's second
//     moment: an exact integer below 2^64 in units of 2^-38, split into its low and high 32 bits
//     and added to two 64-bit words (sq[(job * 3 + c) * 2 + {0 low, 1 high}]) with plain integer
//     atomics -- order-free, no carry between the words, neither can overflow within 2^31
//     samples.  |r| >= 2^32 or a NaN sets the channel's bits in sqflags instead (SQ_NAN, SQ_INF:
//     two bits per channel).  The words are seeded and finalized by kernels in
//     rt_render_f64.hip (no contraction), as the sums' are.
//   * fp64: the stored 28-byte sample records already hold L, so the path kernel is
//     pixels_kernel's own; pixels_reduce_moments_kernel is pixels_reduce_kernel that also adds
//     L L per channel in sample order, each product rounded on its own.
#pragma once
#include "rt_pixels.h"

namespace rtx {

constexpr uint32_t SQ_NAN = 1u, SQ_INF = 2u;   // per channel c: << (2 * c)

// The product, rounded, whatever the translation unit's contraction setting: it cannot fuse
// into an addition that uses it.
__device__ __forceinline__ double dmul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
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
    using R = float;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* s_stack;
    uint32_t* s_mstack;
    const SceneView<R> sc = load_scene_lds<R, BLOCK, TRAV, MESH>(P, smem, s_stack, s_mstack);
    __syncthreads();
    uint16_t* stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;

    int job = 0;
    bool live = false, fin = false;   // holds a path; the list ran out for this lane
    uint32_t segs = 0;
    CounterRng rng;
    rng.st = 0;
    Ray<R> ray;
    ray.o = ray.d = mk((R)0, (R)0, (R)0);
    ray.time = (R)0;
    V3<R> thr = mk((R)1, (R)1, (R)1);
    int nsc = 0;
    int self_id = NO_SELF;
    DiagCounters dg;
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(6164) & 7u;   // hwreg(HW_REG_XCC_ID, 0, 4)
    uint32_t hdone = 0;
    for (;;) {
        bool need = !fin && !live;
        while (hdone < (uint32_t)QUEUE_HEADS) {
            const unsigned long long m = __ballot(need);
            if (m == 0) break;
            const uint32_t k = (uint32_t)__popcll(m);
            const uint32_t rank =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const uint32_t q = (xcc + hdone) & (uint32_t)(QUEUE_HEADS - 1);
            uint32_t base = 0;
            if (lane == __builtin_ctzll(__builtin_amdgcn_read_exec())) base = atomicAdd(P.queue + q * QUEUE_STRIDE, k);
            base = __builtin_amdgcn_readfirstlane(base);
            const unsigned long long c = (unsigned long long)base + rank;
            const unsigned long long i = ((c >> 6) * QUEUE_HEADS + q) * 64 + (c & 63);
            const bool got = need && i < (unsigned long long)n;
            if (got) {
                const unsigned long long fq = q_begin + i;
                job = px_job_of(offsets, num_jobs, total, fq);
                const PixelJob jb = jobs[job];
                const uint32_t sample = jb.sample_begin + (uint32_t)(fq - offsets[job]);
                rng.start(hash32(P.seed32 ^ jb.pixel), sample);
                ray = camera_ray<R>(P, (int)(jb.pixel % (uint32_t)P.W), (int)(jb.pixel / (uint32_t)P.W), rng);
                thr = mk((R)1, (R)1, (R)1);
                nsc = 0;
                self_id = NO_SELF;
                segs = 0;
                live = true;
                need = false;
            }
            if (__any(need)) ++hdone;   // this head ran out: the lanes still waiting ask the next
        }
        if (need) fin = true;   // every head is exhausted
        if (!__any(live)) break;
        if (live) {
            ++segs;
            const Hit<R> h = closest_hit<R, false, false, TRAV, MESH>(sc, ray, stack, BLOCK, self_id, &dg);
            bool done = true;
            V3<R> L = mk((R)0, (R)0, (R)0);
            if (h.id == -1) {
                L = mul_rn(thr, sky(ray.d));
            } else {
                const Shade<R> sh = shade<R, MESH>(sc, ray, h);
                V3<R> att, dir;
                if (scatter<R, false>(sc.mat[sh.meta & META_MAT_MASK], (sh.meta >> 24) & 3u, ray.d, sh, rng, att, dir)) {
                    thr = thr * att;
                    ++nsc;
                    ray.o = sh.p;
                    ray.d = dir;
                    self_id = h.id;
                    done = nsc >= P.max_depth;
                }
            }
            if (done) {
                // pixels_kernel's sum, then r^2 as two 32-bit halves (or a flag)
                constexpr float SC = (float)(1 << FIX_SAMPLE_SHIFT), ISC = 1.f / SC;
                uint32_t fl = 0, qf = 0;
                auto add = [&](float l, int c) {
                    const float r = __builtin_rintf(l * SC);
                    const float v = r * ISC;
                    if (v == 0.f) return;
                    const double q = (double)v * (double)(1ll << FIX_SHIFT);
                    if (fabs(q) < 0x1p62)
                        atomicAdd(acc + (size_t)job * 3 + c, (unsigned long long)(long long)q);
                    else   // NaN, inf or overflow
                        fl |= (q != q ? FIX_NAN : q > 0 ? FIX_POS : FIX_NEG) << (3 * c);
                    const float ar = fabsf(r);
                    if (ar < 0x1p32f) {
                        const unsigned long long a = (unsigned long long)ar, s = a * a;
                        unsigned long long* w = sq + ((size_t)job * 3 + c) * 2;
                        if (s & 0xffffffffull) atomicAdd(w, s & 0xffffffffull);
                        if (s >> 32) atomicAdd(w + 1, s >> 32);
                    } else {   // NaN, inf, or a sample at or beyond 2^13
                        qf |= (r != r ? SQ_NAN : SQ_INF) << (2 * c);
                    }
                };
                add(L.x, 0);
                add(L.y, 1);
                add(L.z, 2);
                if (fl) atomicOr(flags + job, fl);
                if (qf) atomicOr(sqflags + job, qf);
                if (segs_out) atomicAdd(segs_out + job, segs);
                live = false;
            }
        }
    }
}

// pixels_reduce_kernel (rt_pixels.h) with the second moment: out_sq continues as out does.
template <class R>
__global__ void pixels_reduce_moments_kernel(const unsigned long long* __restrict__ offsets, int num_jobs,
                                             unsigned long long q_begin, unsigned long long q_end,
                                             const R* __restrict__ samp, const uint32_t* __restrict__ sseg,
                                             int accumulate, R* __restrict__ out, R* __restrict__ out_sq,
                                             uint32_t* __restrict__ out_segs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    const unsigned long long j0 = offsets[k], j1 = offsets[k + 1];
    R* o = out + (size_t)k * 3;
    R* o2 = out_sq + (size_t)k * 3;
    if (j0 == j1) {
        if (q_begin == 0 && !accumulate) {
            o[0] = o[1] = o[2] = (R)0;
            o2[0] = o2[1] = o2[2] = (R)0;
            if (out_segs) out_segs[k] = 0;
        }
        return;
    }
    const unsigned long long a = j0 > q_begin ? j0 : q_begin, b = j1 < q_end ? j1 : q_end;
    if (a >= b) return;
    const bool fresh = j0 >= q_begin && !accumulate;
    R x = fresh ? (R)0 : o[0], y = fresh ? (R)0 : o[1], z = fresh ? (R)0 : o[2];
    R xx = fresh ? (R)0 : o2[0], yy = fresh ? (R)0 : o2[1], zz = fresh ? (R)0 : o2[2];
    uint32_t sg = (fresh || !out_segs) ? 0u : out_segs[k];
    for (unsigned long long q = a; q < b; ++q) {
        const R* s = samp + (size_t)(q - q_begin) * 3;
        x += s[0];
        y += s[1];
        z += s[2];
        xx += dmul_rn(s[0], s[0]);
        yy += dmul_rn(s[1], s[1]);
        zz += dmul_rn(s[2], s[2]);
        sg += sseg[q - q_begin];
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
    o2[0] = xx;
    o2[1] = yy;
    o2[2] = zz;
    if (out_segs) out_segs[k] = sg;
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
