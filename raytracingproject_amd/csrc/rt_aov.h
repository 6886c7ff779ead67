// rt_aov.h -- first-hit auxiliary outputs per job (rt_render_pixels_aov): for every sample of a
// job list (rt_pixels.h: jobs, offsets, the flat sample list) the camera ray rt_camera_rays
// writes and the record rt_trace_rays returns for it, reduced per job on the device:
//   albedo, normal  the per-sample value summed by rt_render_pixels' rule (fp32: rintf(v 2^19)
//                   as exact integers in units of 2^-FIX_SHIFT, or a flag; fp64: in sample order),
//   depth, id       the nearest hit of the job: the smallest (t, id),
//   hits            the number of samples that hit.
// One segment per sample, so nothing is persistent: a wave takes chunks of 64 consecutive flat
// samples, its lanes stay in lockstep, and no queue head is claimed.
//   * fp32: the lanes of one job are one contiguous run of the wave.  With COMBINE each run is
//     reduced across lanes first -- a segmented inclusive scan of the six 64-bit sums and of the
//     nearest-hit word by __shfl_up (no LDS memory, no barrier), the hit count from a ballot --
//     and the run's last lane issues the atomics: 8 per run instead of up to 8 per sample.
//     Integer sums and minima are order-free, so COMBINE changes no output bit.  A lane whose
//     value is a flag (non-finite, or beyond the exact range) issues its own atomicOr.  Lanes past
//     the list's end stay in the loop -- its bound is wave-uniform -- as a run of their own that
//     holds the neutral elements and issues nothing.
//   * fp64: a pass stores one record per sample (7 doubles: a, normal, t; one int32 id) at q -
//     q_begin; aov_reduce_kernel, one thread per job, adds them in sample order and keeps the
//     nearest (t, id), continuing across passes.
#pragma once
#include "rt_pixels.h"

namespace rtx {

// fp32: the nearest hit of a job as one word, (float bits of t) << 32 | (uint32_t)id, combined by
// unsigned minimum: t > 0.001, so bit order is numeric order, and equal t leaves the smaller id.
constexpr unsigned long long AOV_NONE = 0x7f800000ffffffffull;   // (+inf, -1)

// fp64: the nearest hit the reduction carries between passes (the caller may give only one of
// depth / id, or neither, so the outputs cannot carry it)
struct AovNear {
    double t;
    int32_t id, pad;
};
static_assert(sizeof(AovNear) == 16, "AovNear");

// (t, id) < (u, jd): the smaller t; among equal t the smaller id (as unsigned: -1, no hit, last)
__host__ __device__ __forceinline__ bool aov_nearer(double t, int32_t id, double u, int32_t jd) {
    return t < u || (t == u && (uint32_t)id < (uint32_t)jd);
}

// What the fp32 kernel adds to.  A null pointer: that output was not asked for.
struct AovAcc {
    unsigned long long* albedo;   // num_jobs x 3, units of 2^-FIX_SHIFT
    uint32_t* albedo_flags;       // num_jobs
    unsigned long long* normal;
    uint32_t* normal_flags;
    unsigned long long* nearest;  // num_jobs words as above
    uint32_t* hits;               // num_jobs
};

__device__ __forceinline__ unsigned long long aov_shfl_up(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return (unsigned long long)hi << 32 | lo;
}

// Flat samples [q_begin, q_begin + n) of the job list's `total`.  remap: rt_trace_rays' id map.
// fp32 (!EXACT): A's arrays are added to.  fp64 (EXACT): rec (n x 7) and rid (n) are written at
// q - q_begin.
template <class R, bool EXACT, int BLOCK, int MINW, int TRAV, bool MESH, bool COMBINE>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(MINW))) void aov_kernel(
    RenderParams P, const PixelJob* __restrict__ jobs, const unsigned long long* __restrict__ offsets, int num_jobs,
    unsigned long long total, unsigned long long q_begin, int n, const int* __restrict__ remap, AovAcc A,
    R* __restrict__ rec, int32_t* __restrict__ rid) {
    static_assert(!EXACT || sizeof(R) == 8, "EXACT needs fp64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* s_stack;
    uint32_t* s_mstack;
    const SceneView<R> sc = load_scene_lds<R, BLOCK, TRAV, MESH>(P, smem, s_stack, s_mstack);
    __syncthreads();
    uint16_t* stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;
    DiagCounters dg;
    // chunk c of the pass: samples [64 c, 64 c + 64); `base` is wave-uniform, so every lane of a
    // wave runs every iteration of its wave and takes part in the shuffles below
    const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
    for (unsigned long long base = (unsigned long long)blockIdx.x * BLOCK + (threadIdx.x & ~63u);
         base < (unsigned long long)n; base += step) {
        const unsigned long long i = base + (unsigned)lane;
        const bool valid = i < (unsigned long long)n;
        int job = -1;                                         // (past the end: a run of its own)
        V3<R> a = mk((R)0, (R)0, (R)0), nrm = a;             // a miss adds 0
        double t = __builtin_huge_val();
        int32_t id = -1;
        if (valid) {
            CounterRng rng;
            Ray<R> ray;
            job = px_sample_start<R>(P, jobs, offsets, num_jobs, total, q_begin + i, rng, ray);
            const Hit<R> h = closest_hit<R, EXACT, false, TRAV, MESH>(sc, ray, stack, BLOCK, NO_SELF, &dg);
            if (h.id != -1) {
                const Shade<R> sh = shade<R, MESH>(sc, ray, h);
                nrm = sh.normal;
                // material::scatter's attenuation: the albedo, or (1, 1, 1) for a dielectric
                if (((sh.meta >> 24) & 3u) == MAT_DIELECTRIC) {
                    a = mk((R)1, (R)1, (R)1);
                } else {
                    const auto& m = sc.mat[sh.meta & META_MAT_MASK];
                    a = mk((R)m.p[0], (R)m.p[1], (R)m.p[2]);
                }
                t = EXACT && h.id <= -2 ? h.td : (double)h.t;   // (trace_kernel's rt_hit.t)
                const int slot = h.id >= MESH_HIT_BASE ? P.n_spheres + P.n_big + (h.id & (MESH_HIT_BASE - 1))
                                 : h.id <= -2          ? P.n_spheres + (-2 - h.id)
                                                       : h.id;
                id = remap[slot];
            }
        }
        if constexpr (EXACT) {
            if (valid) {
                R* o = rec + (size_t)i * 7;
                o[0] = a.x, o[1] = a.y, o[2] = a.z;
                o[3] = nrm.x, o[4] = nrm.y, o[5] = nrm.z;
                o[6] = (R)t;
                rid[i] = id;
            }
        } else {
            const bool hit = id != -1;
            uint32_t fla = 0, fln = 0;
            unsigned long long s[6] = {0, 0, 0, 0, 0, 0};   // (two's complement: sums wrap as the atomics do)
            if (hit) {
                if (A.albedo) {
                    s[0] = (unsigned long long)fix_sample(a.x, 0, fla);
                    s[1] = (unsigned long long)fix_sample(a.y, 1, fla);
                    s[2] = (unsigned long long)fix_sample(a.z, 2, fla);
                }
                if (A.normal) {
                    s[3] = (unsigned long long)fix_sample(nrm.x, 0, fln);
                    s[4] = (unsigned long long)fix_sample(nrm.y, 1, fln);
                    s[5] = (unsigned long long)fix_sample(nrm.z, 2, fln);
                }
            }
            if (fla) atomicOr(A.albedo_flags + job, fla);
            if (fln) atomicOr(A.normal_flags + job, fln);
            unsigned long long w = hit ? (unsigned long long)__float_as_uint((float)t) << 32 | (uint32_t)id : AOV_NONE;
            uint32_t cnt = hit ? 1u : 0u;
            bool issue = valid;
            if constexpr (COMBINE) {
                // segmented inclusive scan over the run of `job`: runs are contiguous, so lane -
                // d in the run means every lane between is; the run's last lane ends with its total
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int jd = __shfl_up(job, d);
                    const bool same = jd == job && lane >= d;
                    if (A.albedo) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const unsigned long long o = aov_shfl_up(s[c], d);
                            if (same) s[c] += o;
                        }
                    }
                    if (A.normal) {
#pragma unroll
                        for (int c = 3; c < 6; ++c) {
                            const unsigned long long o = aov_shfl_up(s[c], d);
                            if (same) s[c] += o;
                        }
                    }
                    if (A.nearest) {
                        const unsigned long long o = aov_shfl_up(w, d);
                        if (same && o < w) w = o;
                    }
                }
                // the run's hits: the ballot's bits from the run's first lane to this one
                const unsigned long long hitm = __ballot(hit);
                // (the shuffles first, by every lane: under a short-circuit || lanes 0 and 63
                // would sit them out, and their neighbours would read an inactive lane)
                const int prev = __shfl_up(job, 1), next = __shfl_down(job, 1);
                const unsigned long long heads = __ballot(lane == 0 || prev != job);
                const bool tail = lane == 63 || next != job;
                const unsigned long long upto = ~0ull >> (63 - lane);   // lanes 0 .. lane
                const int first = 63 - __builtin_clzll(heads & upto);    // (lane 0 is a head)
                cnt = (uint32_t)__popcll(hitm & upto & (~0ull << first));
                issue = valid && tail;
            }
            if (issue && cnt) {   // (no hit in the run: sums 0, word AOV_NONE, nothing to add)
                if (A.albedo) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (s[c]) atomicAdd(A.albedo + (size_t)job * 3 + c, s[c]);
                }
                if (A.normal) {
#pragma unroll
                    for (int c = 3; c < 6; ++c)
                        if (s[c]) atomicAdd(A.normal + (size_t)job * 3 + (c - 3), s[c]);
                }
                if (A.nearest) atomicMin(A.nearest + job, w);
                if (A.hits) atomicAdd(A.hits + job, cnt);
            }
        }
    }
}

// fp32, one thread per job, before aov_kernel: the nearest-hit word starts at (+inf, -1), or
// (accumulate, a job that has samples) at what depth / id hold, a missing one counting as +inf
// / -1; hits is zeroed unless accumulate.
template <class R>
__global__ void aov_seed_kernel(const unsigned long long* __restrict__ offsets, int num_jobs, int accumulate,
                                const R* __restrict__ depth, const int32_t* __restrict__ id,
                                unsigned long long* __restrict__ nearest, uint32_t* __restrict__ hits) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    if (nearest) {
        unsigned long long w = AOV_NONE;
        if (accumulate && offsets[k] != offsets[k + 1]) {
            const uint32_t tb = depth ? __float_as_uint((float)depth[k]) : 0x7f800000u;
            w = (unsigned long long)tb << 32 | (id ? (uint32_t)id[k] : 0xffffffffu);
        }
        nearest[k] = w;
    }
    if (hits && !accumulate) hits[k] = 0;
}

// ... and after it: the word's halves; with accumulate a job without samples keeps what the
// buffers hold.
template <class R>
__global__ void aov_finalize_kernel(const unsigned long long* __restrict__ offsets, int num_jobs, int accumulate,
                                    const unsigned long long* __restrict__ nearest, R* __restrict__ depth,
                                    int32_t* __restrict__ id) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    if (accumulate && offsets[k] == offsets[k + 1]) return;
    const unsigned long long w = nearest[k];
    if (depth) depth[k] = (R)__uint_as_float((uint32_t)(w >> 32));
    if (id) id[k] = (int32_t)(uint32_t)w;
}

// fp64: the records of one pass, flat indices [q_begin, q_end), into their jobs' outputs: one
// thread per job adds that job's samples of the pass in sample order and keeps the nearest (t,
// id).  A job whose first sample lies in this pass starts from 0 and (+inf, -1) (accumulate:
// from the buffers, a missing depth / id counting as +inf / -1); one that began in an earlier
// pass continues the sums and counts in the buffers and the nearest hit in `carry`.  In the first
// pass (q_begin == 0) the jobs that count 0 get (0, 0, +inf, -1, 0) unless accumulate.  Any
// output may be null.
template <class R>
__global__ void aov_reduce_kernel(const unsigned long long* __restrict__ offsets, int num_jobs,
                                  unsigned long long q_begin, unsigned long long q_end, const R* __restrict__ rec,
                                  const int32_t* __restrict__ rid, int accumulate, AovNear* __restrict__ carry,
                                  R* __restrict__ albedo, R* __restrict__ normal, R* __restrict__ depth,
                                  int32_t* __restrict__ id, uint32_t* __restrict__ hits) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    const unsigned long long j0 = offsets[k], j1 = offsets[k + 1];
    R* oa = albedo ? albedo + (size_t)k * 3 : nullptr;
    R* on = normal ? normal + (size_t)k * 3 : nullptr;
    if (j0 == j1) {
        if (q_begin == 0 && !accumulate) {
            if (oa) oa[0] = oa[1] = oa[2] = (R)0;
            if (on) on[0] = on[1] = on[2] = (R)0;
            if (depth) depth[k] = (R)__builtin_huge_val();
            if (id) id[k] = -1;
            if (hits) hits[k] = 0;
        }
        return;
    }
    const unsigned long long b0 = j0 > q_begin ? j0 : q_begin, b1 = j1 < q_end ? j1 : q_end;
    if (b0 >= b1) return;
    const bool first = j0 >= q_begin;          // the job's first pass
    const bool fresh = first && !accumulate;
    R s[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s[c] = fresh || !oa ? (R)0 : oa[c];
        s[3 + c] = fresh || !on ? (R)0 : on[c];
    }
    uint32_t cnt = fresh || !hits ? 0u : hits[k];
    double t = __builtin_huge_val();
    int32_t nid = -1;
    if (!first) {
        t = carry[k].t;
        nid = carry[k].id;
    } else if (accumulate) {
        if (depth) t = (double)depth[k];
        if (id) nid = id[k];
    }
    for (unsigned long long q = b0; q < b1; ++q) {
        const R* r = rec + (size_t)(q - q_begin) * 7;
        const int32_t rj = rid[q - q_begin];
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] += r[c];
        if (rj != -1) {
            ++cnt;
            if (aov_nearer((double)r[6], rj, t, nid)) {
                t = (double)r[6];
                nid = rj;
            }
        }
    }
    if (oa) oa[0] = s[0], oa[1] = s[1], oa[2] = s[2];
    if (on) on[0] = s[3], on[1] = s[4], on[2] = s[5];
    if (hits) hits[k] = cnt;
    if (depth) depth[k] = (R)t;
    if (id) id[k] = nid;
    if (j1 > q_end) {
        carry[k].t = t;
        carry[k].id = nid;
    }
}

}  // namespace rtx
