// rt_pixels.h -- sparse rendering (rt_render_pixels) and the device camera-ray generator
// (rt_camera_rays): a device list of jobs {pixel, sample_begin, sample_count}, each the sum of
// those samples of that pixel, bit for bit what rt_render / rt_render_range write for them.
//
// The flat sample list is job 0's samples in order, then job 1's, ...: offsets[k] (64-bit, an
// exclusive scan of the valid jobs' counts, offsets[num_jobs] = T) is job k's first flat index.
// A job with sample_count == 0 or pixel >= W * H counts 0, so no flat index maps to it and no
// kernel here reads or writes anything for it beyond its own output slots.
//
// pixels_kernel runs radiance_kernel's persistent loop (path_loop, rt_radiance.h: the per-XCD
// heads, the bounce loop in both arithmetics; the tree walk with rt_trace_rays' flags, or for a
// sphere-only scene the sphere grid's walk added to them where the call's plan says so -- the
// same hit either way); its own are the start and the end of a path.  A claimed index is a flat sample q, not a
// ray (px_sample_start): the lane finds its job by a search in offsets, one per path (px_job_of:
// interpolation, then bisection -- one or two round trips to an L2-resident array where the
// counts are equal, at most ceil(log2(num_jobs + 1)) + 2 otherwise, against the 44 or 72 bytes
// of ray and key that radiance_kernel reads per path), starts CounterRng at
// key(seed, pixel, sample) and computes its ray with camera_ray<R>; no ray or key is read.
//   * fp32: a finished path adds rintf(L 2^19) per channel, scaled to units of 2^-FIX_SHIFT
//     (fix_sample, rt_device.h), to the job's 64-bit sums with integer atomics (order-free),
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

// The start of flat sample fq's path: its job (returned), rng started on the stream of the job's
// pixel and that sample, and the camera ray drawn from it.  key: null, or where the path's
// rt_path_key goes -- the pixel, the sample and the draws camera_ray spent as first_draw.
template <class R>
__device__ __forceinline__ int px_sample_start(const RenderParams& P, const PixelJob* __restrict__ jobs,
                                               const unsigned long long* __restrict__ offsets, int num_jobs,
                                               unsigned long long total, unsigned long long fq, CounterRng& rng,
                                               Ray<R>& ray, PathKey* key = nullptr) {
    const int k = px_job_of(offsets, num_jobs, total, fq);
    const PixelJob jb = jobs[k];
    const uint32_t sample = jb.sample_begin + (uint32_t)(fq - offsets[k]);
    rng.start(hash32(P.seed32 ^ jb.pixel), sample);
    int rejected = 0;
    ray = camera_ray<R>(P, (int)(jb.pixel % (uint32_t)P.W), (int)(jb.pixel / (uint32_t)P.W), rng, -1,
                        key ? &rejected : nullptr);
    if (key) {
        key->pixel = jb.pixel;
        key->sample = sample;
        key->first_draw = 3u + (P.defocus ? 2u * (uint32_t)(rejected + 1) : 0u);   // square 2, disk 2 each, time 1
        key->pad = 0;
    }
    return k;
}

// rt_camera_rays: one thread per flat sample (grid-stride): its ray and its key.
template <class R>
__global__ void camera_rays_kernel(RenderParams P, const PixelJob* __restrict__ jobs,
                                   const unsigned long long* __restrict__ offsets, int num_jobs, long long total,
                                   R* __restrict__ rays, PathKey* __restrict__ keys, int32_t* __restrict__ ray_job) {
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total;
         q += (long long)gridDim.x * blockDim.x) {
        CounterRng rng;
        Ray<R> r;
        PathKey key;
        const int k = px_sample_start<R>(P, jobs, offsets, num_jobs, (unsigned long long)total, (unsigned long long)q,
                                         rng, r, &key);
        R* o = rays + (size_t)q * 7;
        o[0] = r.o.x, o[1] = r.o.y, o[2] = r.o.z;
        o[3] = r.d.x, o[4] = r.d.y, o[5] = r.d.z;
        o[6] = r.time;
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
    int idx = 0, job = 0;   // this lane's path: flat sample q_begin + idx, of job `job`
    path_loop<R, EXACT, BLOCK, TRAV, MESH>(
        P, n,
        [&](unsigned long long i, Ray<R>& ray, CounterRng& rng) {
            idx = (int)i;
            job = px_sample_start<R>(P, jobs, offsets, num_jobs, total, q_begin + i, rng, ray);
        },
        [&](const V3<R>& L, uint32_t segs) {
            if constexpr (EXACT) {
                R* o = samp + (size_t)idx * 3;
                o[0] = L.x;
                o[1] = L.y;
                o[2] = L.z;
                sseg[idx] = segs;
            } else {
                uint32_t fl = 0;
                const float l[3] = {L.x, L.y, L.z};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (const long long s = fix_sample(l[c], c, fl))
                        atomicAdd(acc + (size_t)job * 3 + c, (unsigned long long)s);
                if (fl) atomicOr(flags + job, fl);
                if (segs_out) atomicAdd(segs_out + job, segs);
            }
        });
}

// The product, rounded, whatever the translation unit's contraction setting: it cannot fuse
// into an addition that uses it.
__device__ __forceinline__ double dmul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

// fp64: the samples of one pass, flat indices [q_begin, q_end), into their jobs' sums: one
// thread per job adds that job's samples of the pass in sample order.  A job whose first sample
// lies in this pass starts from 0 (accumulate: from out_sums, its segments from out_segs); one
// that began in an earlier pass continues.  In the first pass (q_begin == 0) the jobs that count
// 0 are zeroed unless accumulate.  MOMENTS (rt_render_pixels_moments): out_sq continues as out
// does, with L L per channel, each product rounded on its own; else out_sq is not read.
template <class R, bool MOMENTS>
__global__ void pixels_reduce_kernel(const unsigned long long* __restrict__ offsets, int num_jobs,
                                     unsigned long long q_begin, unsigned long long q_end,
                                     const R* __restrict__ samp, const uint32_t* __restrict__ sseg, int accumulate,
                                     R* __restrict__ out, R* __restrict__ out_sq, uint32_t* __restrict__ out_segs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    const unsigned long long j0 = offsets[k], j1 = offsets[k + 1];
    R* o = out + (size_t)k * 3;
    [[maybe_unused]] R* o2 = MOMENTS ? out_sq + (size_t)k * 3 : nullptr;
    if (j0 == j1) {
        if (q_begin == 0 && !accumulate) {
            o[0] = o[1] = o[2] = (R)0;
            if constexpr (MOMENTS) o2[0] = o2[1] = o2[2] = (R)0;
            if (out_segs) out_segs[k] = 0;
        }
        return;
    }
    const unsigned long long a = j0 > q_begin ? j0 : q_begin, b = j1 < q_end ? j1 : q_end;
    if (a >= b) return;
    const bool fresh = j0 >= q_begin && !accumulate;
    R x = fresh ? (R)0 : o[0], y = fresh ? (R)0 : o[1], z = fresh ? (R)0 : o[2];
    [[maybe_unused]] R xx = (R)0, yy = (R)0, zz = (R)0;
    if constexpr (MOMENTS) {
        if (!fresh) xx = o2[0], yy = o2[1], zz = o2[2];
    }
    uint32_t sg = (fresh || !out_segs) ? 0u : out_segs[k];
    for (unsigned long long q = a; q < b; ++q) {
        const R* s = samp + (size_t)(q - q_begin) * 3;
        x += s[0];
        y += s[1];
        z += s[2];
        if constexpr (MOMENTS) {
            xx += dmul_rn(s[0], s[0]);
            yy += dmul_rn(s[1], s[1]);
            zz += dmul_rn(s[2], s[2]);
        }
        sg += sseg[q - q_begin];
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
    if constexpr (MOMENTS) {
        o2[0] = xx;
        o2[1] = yy;
        o2[2] = zz;
    }
    if (out_segs) out_segs[k] = sg;
}

}  // namespace rtx
