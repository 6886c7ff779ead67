// rt_pixels.h -- sparse rendering (rt_render_pixels) and the device camera-ray generator
// (rt_camera_rays): a device list of jobs {pixel, sample_begin, sample_count}, each the sum of
// those samples of that pixel, bit for bit what rt_render / rt_render_range write for them.
//
// The flat sample list is job 0's samples in order, then job 1's, ...: offsets[k] (64-bit, an
// exclusive scan of the valid jobs' counts, offsets[num_jobs] = T) is job k's first flat index.
// A job with sample_count == 0 or pixel >= W * H counts 0, so no flat index maps to it and no
// kernel here reads or writes anything for it beyond its own output slots.
//
// pixels_kernel is radiance_kernel's (rt_radiance.h) persistent loop -- the per-XCD heads, the
// tree walk with rt_trace_rays' flags, the bounce loop in both arithmetics -- as a sibling, so
// that kernel's instantiations stay what they were.  A claimed index is a flat sample q, not a
// ray: the lane finds its job by a search in offsets, one per path (px_job_of: interpolation,
// then bisection -- one or two round trips to an L2-resident array where the counts are equal,
// at most ceil(log2(num_jobs + 1)) + 2 otherwise, against the 44 or 72 bytes of ray and key
// that radiance_kernel reads per path), starts CounterRng at
// key(seed, pixel, sample) and computes its ray with camera_ray<R>; no ray or key is read.
//   * fp32: a finished path adds rintf(L 2^19) per channel, scaled to units of 2^-FIX_SHIFT,
//     to the job's 64-bit sums with integer atomics (flush_sample's direct path: order-free),
//     flags by atomicOr, segments by a 32-bit atomicAdd into out_segments; px_finalize writes
//     out_sums.
//   * fp64: a finished path stores its three doubles and its count at q - pass_begin;
//     pixels_reduce_kernel, one thread per job, adds the job's samples of the pass in order,
//     continuing out_sums.
#pragma once
#include "rt_launch.h"
#include "rt_radiance.h"

namespace rtx {

struct PixelJob {   // = rt_pixel_job (include/rt_hip.h)
    uint32_t pixel, sample_begin, sample_count, pad;
};
static_assert(sizeof(PixelJob) == 16, "rt_pixel_job");

// The scan's input: job k's sample count where the job is valid, else 0; index num_jobs (the
// element whose exclusive sum is T) reads no job.
struct PixelJobCount {
    const PixelJob* jobs;
    int n;
    uint32_t npix;
    __host__ __device__ __forceinline__ unsigned long long operator()(int k) const {
        if (k >= n) return 0ull;
        const PixelJob j = jobs[k];
        return j.pixel < npix ? (unsigned long long)j.sample_count : 0ull;
    }
};

// The job of flat sample q (offsets[0] = 0 <= q < offsets[n] = total): the k with offsets[k] <=
// q < offsets[k + 1].  Jobs that count 0 share their successor's offset, so k's own count is > 0.
// Two interpolation probes first -- where the jobs' counts are equal (a frame, a crop window, a
// tile list) the first guess, lo + (q - offsets[lo]) / (offsets[hi] - offsets[lo]) * (hi - lo),
// is the job or its neighbour -- each two independent loads; then the binary search over what
// is left, so a list of any shape costs at most two round trips more than bisection alone.
__device__ __forceinline__ int px_job_of(const unsigned long long* __restrict__ offsets, int n,
                                         unsigned long long total, unsigned long long q) {
    int lo = 0, hi = n;   // offsets[lo] = olo <= q < ohi = offsets[hi]
    unsigned long long olo = 0, ohi = total;
    for (int it = 0; it < 2 && hi - lo > 1; ++it) {
        int g = lo + (int)((double)(q - olo) / (double)(ohi - olo) * (double)(hi - lo));
        g = g < lo ? lo : g > hi - 1 ? hi - 1 : g;
        const unsigned long long a = offsets[g], b = offsets[g + 1];
        if (a > q) {
            hi = g;
            ohi = a;
        } else if (q < b) {
            return g;
        } else {
            lo = g + 1;   // (< hi: b = offsets[hi] would be > q)
            olo = b;
        }
    }
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (offsets[mid] <= q)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// rt_camera_rays: one thread per flat sample (grid-stride): camera_ray<R> on the sample's
// stream, the draws it spent as the key's first_draw.
template <class R>
__global__ void camera_rays_kernel(RenderParams P, const PixelJob* __restrict__ jobs,
                                   const unsigned long long* __restrict__ offsets, int num_jobs, long long total,
                                   R* __restrict__ rays, PathKey* __restrict__ keys, int32_t* __restrict__ ray_job) {
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total;
         q += (long long)gridDim.x * blockDim.x) {
        const int k = px_job_of(offsets, num_jobs, (unsigned long long)total, (unsigned long long)q);
        const PixelJob jb = jobs[k];
        const uint32_t sample = jb.sample_begin + (uint32_t)((unsigned long long)q - offsets[k]);
        CounterRng rng;
        rng.start(hash32(P.seed32 ^ jb.pixel), sample);
        int rejected = 0;
        const Ray<R> r = camera_ray<R>(P, (int)(jb.pixel % (uint32_t)P.W), (int)(jb.pixel / (uint32_t)P.W), rng, -1,
                                       &rejected);
        R* o = rays + (size_t)q * 7;
        o[0] = r.o.x, o[1] = r.o.y, o[2] = r.o.z;
        o[3] = r.d.x, o[4] = r.d.y, o[5] = r.d.z;
        o[6] = r.time;
        PathKey key;
        key.pixel = jb.pixel;
        key.sample = sample;
        key.first_draw = 3u + (P.defocus ? 2u * (uint32_t)(rejected + 1) : 0u);   // square 2, disk 2 each, time 1
        key.pad = 0;
        keys[q] = key;
        if (ray_job) ray_job[q] = k;
    }
}

// Flat samples [q_begin, q_begin + n) of the job list's `total`.  P.max_depth >= 1.
// fp32 (!EXACT): acc (num_jobs x 3, units of 2^-FIX_SHIFT), flags (num_jobs), segs (num_jobs,
// or null) are added to.  fp64 (EXACT): samp (n x 3) and sseg (n) are written at q - q_begin.
template <class R, bool EXACT, int BLOCK, int MINW, int TRAV, bool MESH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(MINW))) void pixels_kernel(
    RenderParams P, const PixelJob* __restrict__ jobs, const unsigned long long* __restrict__ offsets, int num_jobs,
    unsigned long long total, unsigned long long q_begin, int n, unsigned long long* __restrict__ acc, uint32_t* __restrict__ flags,
    uint32_t* __restrict__ segs_out, R* __restrict__ samp, uint32_t* __restrict__ sseg) {
    static_assert(!EXACT || sizeof(R) == 8, "EXACT needs fp64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* s_stack;
    uint32_t* s_mstack;
    const SceneView<R> sc = load_scene_lds<R, BLOCK, TRAV, MESH>(P, smem, s_stack, s_mstack);
    __syncthreads();
    uint16_t* stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;

    // this lane's path: flat sample q_begin + idx, of job `job`
    int idx = 0, job = 0;
    bool live = false, fin = false;   // holds a path; the list ran out for this lane
    uint32_t segs = 0;
    CounterRng rng;
    rng.st = 0;
    Ray<R> ray;
    ray.o = ray.d = mk((R)0, (R)0, (R)0);
    ray.time = (R)0;
    V3<R> thr = mk((R)1, (R)1, (R)1);
    [[maybe_unused]] V3<R> att_stack[EXACT ? 64 : 1];   // EXACT: this path's attenuations (scratch)
    int nsc = 0;
    int self_id = NO_SELF;
    DiagCounters dg;
    // wave-uniform: this wave's XCD, and how many heads from there on it has found exhausted
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(6164) & 7u;   // hwreg(HW_REG_XCC_ID, 0, 4)
    uint32_t hdone = 0;
    for (;;) {
        // lanes without a path take the list's next samples (the whole wave runs this)
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
            // (64-bit: a head passes its last sample by at most 64 per wave of the grid, times 8)
            const unsigned long long c = (unsigned long long)base + rank;
            const unsigned long long i = ((c >> 6) * QUEUE_HEADS + q) * 64 + (c & 63);
            const bool got = need && i < (unsigned long long)n;
            if (got) {
                idx = (int)i;
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
            const Hit<R> h =
                closest_hit<R, EXACT, false, TRAV, MESH>(sc, ray, stack, BLOCK, EXACT ? NO_SELF : self_id, &dg);
            bool done = true;
            V3<R> L = mk((R)0, (R)0, (R)0);
            if (h.id == -1) {
                if constexpr (EXACT) {   // camera_cpu.h:19, innermost attenuation first
                    L = sky(ray.d);
                    for (int k = nsc - 1; k >= 0; --k) L = att_stack[k] * L;
                } else {
                    L = mul_rn(thr, sky(ray.d));
                }
            } else {
                const Shade<R> sh = shade<R, MESH>(sc, ray, h);
                V3<R> att, dir;
                if (scatter<R, EXACT>(sc.mat[sh.meta & META_MAT_MASK], (sh.meta >> 24) & 3u, ray.d, sh, rng, att,
                                      dir)) {
                    if constexpr (EXACT)
                        att_stack[nsc] = att;
                    else
                        thr = thr * att;
                    ++nsc;
                    ray.o = sh.p;
                    ray.d = dir;
                    self_id = h.id;
                    done = nsc >= P.max_depth;
                }
            }
            if (done) {
                if constexpr (EXACT) {
                    R* o = samp + (size_t)idx * 3;
                    o[0] = L.x;
                    o[1] = L.y;
                    o[2] = L.z;
                    sseg[idx] = segs;
                } else {
                    // render_lanes' rounding onto the 2^-FIX_SAMPLE_SHIFT grid, then flush_sample's
                    // 64-bit path: an exact integer in units of 2^-FIX_SHIFT, or a flag
                    constexpr float SC = (float)(1 << FIX_SAMPLE_SHIFT), ISC = 1.f / SC;
                    uint32_t fl = 0;
                    auto add = [&](float l, int c) {
                        const float v = __builtin_rintf(l * SC) * ISC;
                        if (v == 0.f) return;
                        const double q = (double)v * (double)(1ll << FIX_SHIFT);
                        if (fabs(q) < 0x1p62)
                            atomicAdd(acc + (size_t)job * 3 + c, (unsigned long long)(long long)q);
                        else   // NaN, inf or overflow
                            fl |= (q != q ? FIX_NAN : q > 0 ? FIX_POS : FIX_NEG) << (3 * c);
                    };
                    add(L.x, 0);
                    add(L.y, 1);
                    add(L.z, 2);
                    if (fl) atomicOr(flags + job, fl);
                    if (segs_out) atomicAdd(segs_out + job, segs);
                }
                live = false;
            }
        }
    }
}

// fp64: the samples of one pass, flat indices [q_begin, q_end), into their jobs' sums: one
// thread per job adds that job's samples of the pass in sample order.  A job whose first sample
// lies in this pass starts from 0 (accumulate: from out_sums, its segments from out_segs); one
// that began in an earlier pass continues.  In the first pass (q_begin == 0) the jobs that count
// 0 are zeroed unless accumulate.
template <class R>
__global__ void pixels_reduce_kernel(const unsigned long long* __restrict__ offsets, int num_jobs,
                                     unsigned long long q_begin, unsigned long long q_end,
                                     const R* __restrict__ samp, const uint32_t* __restrict__ sseg, int accumulate,
                                     R* __restrict__ out, uint32_t* __restrict__ out_segs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    const unsigned long long j0 = offsets[k], j1 = offsets[k + 1];
    R* o = out + (size_t)k * 3;
    if (j0 == j1) {
        if (q_begin == 0 && !accumulate) {
            o[0] = o[1] = o[2] = (R)0;
            if (out_segs) out_segs[k] = 0;
        }
        return;
    }
    const unsigned long long a = j0 > q_begin ? j0 : q_begin, b = j1 < q_end ? j1 : q_end;
    if (a >= b) return;
    const bool fresh = j0 >= q_begin && !accumulate;
    R x = fresh ? (R)0 : o[0], y = fresh ? (R)0 : o[1], z = fresh ? (R)0 : o[2];
    uint32_t sg = (fresh || !out_segs) ? 0u : out_segs[k];
    for (unsigned long long q = a; q < b; ++q) {
        const R* s = samp + (size_t)(q - q_begin) * 3;
        x += s[0];
        y += s[1];
        z += s[2];
        sg += sseg[q - q_begin];
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
    if (out_segs) out_segs[k] = sg;
}

}  // namespace rtx
