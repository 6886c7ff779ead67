// rt_render_f64.hip -- fp64 reference-exact path, built with -ffp-contract=off so every
// operation rounds as in the g++ build of the reference.  Also hosts the small
// precision-agnostic kernels (unshard, quantize).
#include "rt_occluded.h"   // (includes rt_render_impl.h)
#include "rt_radiance.h"
#include "rt_pixels.h"
#include "rt_moments.h"
#include "rt_aov.h"

#include <hipcub/hipcub.hpp>

namespace rtx {

// The fp64 kernels (rt_tuning.f64_kernel; rt_launch.h RenderKernel):
//  3 conservative fp32 slab tests (TRAV_F32BOX: each slab widened by a bound of its
//    rounding, so no box the exact ray enters is rejected) on persistent lanes over the
//    work queue (TRAV_PERSIST, render_lanes<EXACT>: each sample's radiance stored, ordered
//    reduction afterwards), 512-thread workgroups within 128 VGPRs: 4 waves per SIMD;
//  4 (default) kernel 3 with coherent primaries (TRAV_COH: render_coherent<double, EXACT>,
//    camera rays traced in per-tile batches, their fp64 hits queued in LDS): C2 11.9 ms,
//    C3 97.9 ms against kernel 3's 14.3 / 119.2 on the same box (f64_probe*_r03ak.jsonl).
// Both render the same frame bit for bit (the boxes only prune; spheres and triangles are
// tested in fp64; the sums are the reference's in-order fp64 additions).  Kernels 1 (fp64
// slabs, one wave per 8x8 tile: C2 26.2 ms) and 2 (kernel 3's box tests, one wave per
// tile: 23.6 ms) of rounds 1-3 were removed in r04
// (profiles/r03/f64_kernel_probe_r03{m,n,o}*.jsonl).
//  5 (default where rt_upload_scene built a sphere grid and the tuning's traversal asks for
//    it, RT_TRAV_GRID) kernel 4 walking the uniform sphere grid instead of the sphere tree:
//    the cells chosen in fp32 from the rounded ray (the listed boxes' padding covers the
//    rounding), every listed sphere tested in fp64 -- the same frame bit for bit.
//  6 (r06; never asked for: the C ABI runs it for 5 where the grid is one cell tall in y,
//    unless the traversal carries 262144) kernel 5 with the flat walk (TRAV_GFLAT).
//
// An entry's key and its kernel come from the same template arguments; each kernel is built for
// scenes with a mesh and without.
template <int K, int W, int T, int B, bool MESH>
constexpr RenderKernel entry() {
    return {B, W, T, MESH, false, K, render_kernel<double, true, B, W, false, T, MESH>};
}
constexpr int LANES = TRAV_F32BOX | TRAV_PERSIST, COH = LANES | TRAV_COH, GRID = COH | TRAV_GRID,
              GFLAT = GRID | TRAV_GFLAT;
constexpr RenderKernel F64_KERNELS[] = {
    entry<3, 4, LANES, 512, true>(), entry<3, 4, LANES, 512, false>(),   //
    entry<4, 4, COH, 512, true>(),   entry<4, 4, COH, 512, false>(),     //
    entry<5, 4, GRID, 512, true>(),  entry<5, 4, GRID, 512, false>(),    //
    entry<6, 4, GFLAT, 512, true>(), entry<6, 4, GFLAT, 512, false>(),
};

const RenderKernel* find_render_f64(int kernel, bool mesh) {
    for (const RenderKernel& k : F64_KERNELS)
        if (k.f64_kernel == kernel && k.mesh == mesh) return &k;
    return nullptr;
}

hipError_t launch_tape_f64(const RenderParams& P, int max_depth, const double* ray7, const double* tape, int tape_len,
                           double* out, int* used, hipStream_t stream) {
    hipLaunchKernelGGL(tape_kernel<double>, dim3(1), dim3(64), 0, stream, P, max_depth, ray7, tape, tape_len, out,
                       used);
    return hipGetLastError();
}

hipError_t launch_unshard(const void* gathered, void* frame, int elem_bytes, int channels, int W, int H, int tiles_x,
                          int nshards, int max_shard_tiles, hipStream_t stream) {
    const dim3 block(256), grid((W + 255) / 256, H);
    if (W <= 0 || H <= 0) return hipSuccess;
    if (elem_bytes == 8 && channels == 3)
        hipLaunchKernelGGL((unshard_kernel<double, 3>), grid, block, 0, stream, (const double*)gathered,
                           (double*)frame, W, H, tiles_x, nshards, max_shard_tiles);
    else if (elem_bytes == 4 && channels == 3)
        hipLaunchKernelGGL((unshard_kernel<float, 3>), grid, block, 0, stream, (const float*)gathered, (float*)frame,
                           W, H, tiles_x, nshards, max_shard_tiles);
    else if (elem_bytes == 4 && channels == 1)
        hipLaunchKernelGGL((unshard_kernel<uint32_t, 1>), grid, block, 0, stream, (const uint32_t*)gathered,
                           (uint32_t*)frame, W, H, tiles_x, nshards, max_shard_tiles);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_reduce(const void* samples, void* out, int elem_bytes, size_t n, int nsamples, int accumulate,
                         hipStream_t stream) {
    if (elem_bytes == 8)
        return launch_1d(reduce_kernel<double>, n, stream, (const double*)samples, (double*)out, n, nsamples,
                         accumulate);
    if (elem_bytes == 4)
        return launch_1d(reduce_kernel<float>, n, stream, (const float*)samples, (float*)out, n, nsamples, accumulate);
    return hipErrorInvalidValue;
}

hipError_t launch_quantize(const void* frame, int elem_bytes, int32_t* rgb, size_t n, int spp, hipStream_t stream) {
    if (elem_bytes == 8) return launch_1d(quantize_kernel<double>, n, stream, (const double*)frame, rgb, n, spp);
    if (elem_bytes == 4) return launch_1d(quantize_kernel<float>, n, stream, (const float*)frame, rgb, n, spp);
    return hipErrorInvalidValue;
}

hipError_t launch_finish_u8(const void* gathered, int elem_bytes, uint8_t* rgb, int W, int H, int tiles_x,
                            int nshards, int max_shard_tiles, int spp, hipStream_t stream) {
    const dim3 block(256), grid((W + 255) / 256, H);
    if (W <= 0 || H <= 0) return hipSuccess;
    const double scale = 1.0 / spp;
    if (elem_bytes == 8)
        hipLaunchKernelGGL(finish_u8_kernel<double>, grid, block, 0, stream, (const double*)gathered, rgb, W, H,
                           tiles_x, nshards, max_shard_tiles, scale);
    else if (elem_bytes == 4)
        hipLaunchKernelGGL(finish_u8_kernel<float>, grid, block, 0, stream, (const float*)gathered, rgb, W, H,
                           tiles_x, nshards, max_shard_tiles, scale);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// One pixel channel's fixed-point sum (and its flags) as the float out_sums value.
__device__ __forceinline__ float finalized(long long acc, uint32_t f) {
    if (f & FIX_NAN || (f & FIX_POS && f & FIX_NEG)) return __builtin_nanf("");
    if (f) return f & FIX_POS ? __builtin_huge_valf() : -__builtin_huge_valf();
    return (float)((double)acc * (1.0 / (double)(1ll << FIX_SHIFT)));
}

// fp32 fixed-point sums -> out_sums: one thread per pixel channel.
__global__ void finalize_kernel(long long* __restrict__ accum, const unsigned long long* __restrict__ packed,
                                const uint32_t* __restrict__ flags, float* __restrict__ out, size_t n) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (packed) {   // this launch's packed sums (units of 2^-FIX_SAMPLE_SHIFT) join the running sums
        const size_t p = e / 3;
        const int c = (int)(e % 3);
        const unsigned long long w = packed[2 * p + (c == 2 ? 1 : 0)];
        const unsigned long long u = c == 1 ? w >> 32 : c == 0 ? (w & 0xffffffffull) : w;
        accum[e] += (long long)(u << (FIX_SHIFT - FIX_SAMPLE_SHIFT));
    }
    out[e] = finalized(accum[e], (flags[e / 3] >> (3 * (e % 3))) & 7u);
}

// Continue sums the context holds no fixed-point state for: out_sums -> accum (rounded
// onto the grid), non-finite values -> flags.
__global__ void seed_accum_kernel(const float* __restrict__ out, long long* __restrict__ accum,
                                  uint32_t* __restrict__ flags, size_t npx) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npx) return;
    uint32_t fl = 0;
    for (int c = 0; c < 3; ++c) {
        const double v = rint((double)out[p * 3 + c] * (double)(1ll << FIX_SHIFT));
        if (fabs(v) < 0x1p62) {
            accum[p * 3 + c] = (long long)v;
        } else {
            accum[p * 3 + c] = 0;
            fl |= (v != v ? FIX_NAN : v > 0 ? FIX_POS : FIX_NEG) << (3 * c);
        }
    }
    flags[p] = fl;
}

// Continue sums the context DOES hold fixed-point state for, per pixel channel: the
// state is kept only where out_sums still holds, bit for bit, what finalize_kernel last
// wrote from it; anywhere else (the caller changed the buffer, or freed it and got the
// same address back for another frame) the channel restarts from out_sums' float value,
// as for a buffer the context has never seen.
__global__ void reconcile_accum_kernel(const float* __restrict__ out, long long* __restrict__ accum,
                                       uint32_t* __restrict__ flags, size_t npx) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npx) return;
    uint32_t fl = flags[p];
    for (int c = 0; c < 3; ++c) {
        const uint32_t fc = (fl >> (3 * c)) & 7u;
        const float have = out[p * 3 + c];
        if (__float_as_uint(finalized(accum[p * 3 + c], fc)) == __float_as_uint(have)) continue;
        const double v = rint((double)have * (double)(1ll << FIX_SHIFT));
        fl &= ~(7u << (3 * c));
        if (fabs(v) < 0x1p62) {
            accum[p * 3 + c] = (long long)v;
        } else {
            accum[p * 3 + c] = 0;
            fl |= (v != v ? FIX_NAN : v > 0 ? FIX_POS : FIX_NEG) << (3 * c);
        }
    }
    flags[p] = fl;
}

// Batched world.hit (rt_trace_rays), fp64: the reference's arithmetic (sphere.h:30-57).
hipError_t launch_trace_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                            void* hits, const int* remap, const int* origin_ids, const int* unmap, int n_unmap) {
    // the default fp64 kernel's box tests (conservative fp32 slabs)
    constexpr int B = TRACE_BLOCK, T = QUERY_TRAV_F64;
    const auto kernel =
        P.n_mnodes > 0 ? trace_kernel<double, true, B, T, true> : trace_kernel<double, true, B, T, false>;
    return launch_1d_capped(kernel, n, TRACE_MAX_GRID, lds_bytes, stream, P, (const double*)rays, n, (TraceHit*)hits,
                            remap, origin_ids, unmap, n_unmap);
}

// Batched any-hit visibility (rt_occluded), fp64: the reference's boolean (hittable.h:28) --
// spheres and triangles in its fp64 arithmetic, conservative fp32 boxes that only prune.
hipError_t launch_occluded_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* intervals, uint8_t* occluded) {
    constexpr int B = TRACE_BLOCK, T = QUERY_TRAV_F64;
    const auto kernel =
        P.n_mnodes > 0 ? occluded_kernel<double, true, B, T, true> : occluded_kernel<double, true, B, T, false>;
    return launch_1d_capped(kernel, n, TRACE_MAX_GRID, lds_bytes, stream, P, (const double*)rays, n,
                            (const double*)intervals, occluded);
}

// Batched ray_color (rt_radiance_rays), fp64: the reference's arithmetic with the default fp64
// kernel's box tests (conservative fp32 slabs, which only prune), at the fp64 render kernels'
// register budget (4 waves per SIMD, <= 128 VGPRs).
hipError_t launch_radiance_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* keys, void* radiance, uint32_t* segments, int n_cu) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    return launch_for_scene<radiance_kernel<double, true, B, 4, QUERY_TRAV_F64, true>,
                            radiance_kernel<double, true, B, 4, QUERY_TRAV_F64, false>, B>(
        P, lds_bytes, stream, n, n_cu, 0, (const double*)rays, n, (const PathKey*)keys, (double*)radiance, segments);
}

hipError_t launch_reconcile_accum(const float* out, long long* accum, uint32_t* flags, size_t npx,
                                  hipStream_t stream) {
    return launch_1d(reconcile_accum_kernel, npx, stream, out, accum, flags, npx);
}

hipError_t launch_finalize(long long* accum, const unsigned long long* packed, const uint32_t* flags, float* out,
                           size_t npx, hipStream_t stream) {
    return launch_1d(finalize_kernel, npx * 3, stream, accum, packed, flags, out, npx * 3);
}

// ---- sparse rendering (rt_render_pixels, rt_camera_rays; rt_pixels.h) -----------------------
hipError_t launch_pixel_scan(const void* jobs, int num_jobs, uint32_t npix, unsigned long long* offsets, void* temp,
                             size_t* temp_bytes, hipStream_t stream) {
    const PixelJobCount count{(const PixelJob*)jobs, num_jobs, npix};
    hipcub::CountingInputIterator<int> idx(0);
    hipcub::TransformInputIterator<unsigned long long, PixelJobCount, hipcub::CountingInputIterator<int>> in(idx, count);
    return hipcub::DeviceScan::ExclusiveSum(temp, *temp_bytes, in, offsets, num_jobs + 1, stream);
}

hipError_t launch_camera_rays_f64(const RenderParams& P, hipStream_t stream, const void* jobs,
                                  const unsigned long long* offsets, int num_jobs, long long total, void* rays,
                                  void* keys, int32_t* ray_job) {
    return launch_1d_capped(camera_rays_kernel<double>, total, CAMERA_RAYS_MAX_GRID, 0, stream, P,
                            (const PixelJob*)jobs, offsets, num_jobs, total, (double*)rays, (PathKey*)keys, ray_job);
}

// Sparse rendering (rt_render_pixels), fp64: launch_radiance_f64's box tests, register budget
// and grid.  grid: what the call's plan walks (rt_launch.h) -- the cells chosen in fp32, the listed
// spheres tested in fp64, as f64_kernel 5 / 6 walk them.
constexpr int TQ3 = QUERY_TRAV_F64 | QUERY_GRID, TQF = TQ3 | QUERY_GFLAT;
hipError_t launch_pixels_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                             const unsigned long long* offsets, int num_jobs, unsigned long long total,
                             unsigned long long q_begin, int n,
                             double* samples, uint32_t* sample_segs, int n_cu, int grid, int max_wgs) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    const PixelJob* j = (const PixelJob*)jobs;
    unsigned long long* const no_acc = nullptr;
    uint32_t* const no_u32 = nullptr;
    if (grid)
        return launch_for_grid<pixels_kernel<double, true, B, 4, TQ3, false>,
                               pixels_kernel<double, true, B, 4, TQF, false>, B>(
            P, grid, lds_bytes, stream, n, n_cu, max_wgs, j, offsets, num_jobs, total, q_begin, n, no_acc, no_u32,
            no_u32, samples, sample_segs);
    return launch_for_tree<pixels_kernel<double, true, B, 4, QUERY_TRAV_F64, true>,
                           pixels_kernel<double, true, B, 4, QUERY_TRAV_F64, false>, B>(
        P, lds_bytes, stream, n, n_cu, max_wgs, j, offsets, num_jobs, total, q_begin, n, no_acc, no_u32, no_u32, samples,
        sample_segs);
}

hipError_t launch_pixels_reduce(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                                unsigned long long q_end, const double* samples, const uint32_t* sample_segs,
                                int accumulate, double* out_sums, uint32_t* out_segments, hipStream_t stream) {
    return launch_1d(pixels_reduce_kernel<double, false>, num_jobs, stream, offsets, num_jobs, q_begin, q_end, samples,
                     sample_segs, accumulate, out_sums, (double*)nullptr, out_segments);
}

// fp32, one thread per job, before the path kernel: the job's fixed-point sums start at 0, or
// (accumulate, a job that has samples) where out_sums stands, as seed_accum_kernel rounds it.
__global__ void px_seed_kernel(const unsigned long long* __restrict__ offsets, int num_jobs, int accumulate,
                               const float* __restrict__ out, long long* __restrict__ acc,
                               uint32_t* __restrict__ flags, uint32_t* __restrict__ out_segs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    uint32_t fl = 0;
    const bool cont = accumulate && offsets[k] != offsets[k + 1];
    for (int c = 0; c < 3; ++c) {
        long long a = 0;
        if (cont) {
            const double v = rint((double)out[(size_t)k * 3 + c] * (double)(1ll << FIX_SHIFT));
            if (fabs(v) < 0x1p62)
                a = (long long)v;
            else
                fl |= (v != v ? FIX_NAN : v > 0 ? FIX_POS : FIX_NEG) << (3 * c);
        }
        acc[(size_t)k * 3 + c] = a;
    }
    flags[k] = fl;
    if (out_segs && !accumulate) out_segs[k] = 0;
}

// ... and after it: the sums as floats (finalize_kernel's value); with accumulate a job
// without samples keeps what out_sums holds.
__global__ void px_finalize_kernel(const unsigned long long* __restrict__ offsets, int num_jobs, int accumulate,
                                   const long long* __restrict__ acc, const uint32_t* __restrict__ flags,
                                   float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    if (accumulate && offsets[k] == offsets[k + 1]) return;
    for (int c = 0; c < 3; ++c) out[(size_t)k * 3 + c] = finalized(acc[(size_t)k * 3 + c], (flags[k] >> (3 * c)) & 7u);
}

hipError_t launch_pixels_seed(const unsigned long long* offsets, int num_jobs, int accumulate, const float* out_sums,
                              long long* acc, uint32_t* flags, uint32_t* out_segments, hipStream_t stream) {
    return launch_1d(px_seed_kernel, num_jobs, stream, offsets, num_jobs, accumulate, out_sums, acc, flags,
                     out_segments);
}

hipError_t launch_pixels_finalize(const unsigned long long* offsets, int num_jobs, int accumulate,
                                  const long long* acc, const uint32_t* flags, float* out_sums, hipStream_t stream) {
    return launch_1d(px_finalize_kernel, num_jobs, stream, offsets, num_jobs, accumulate, acc, flags, out_sums);
}

// First-hit auxiliary outputs (rt_render_pixels_aov), fp64: launch_trace_f64's box tests, so a
// sample's record is rt_trace_rays'; launch_pixels_f64's register budget and grid bound.
hipError_t launch_aov_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                          const unsigned long long* offsets, int num_jobs, unsigned long long total,
                          unsigned long long q_begin, int n, const int* remap, double* records, int32_t* record_ids,
                          int n_cu) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    const PixelJob* j = (const PixelJob*)jobs;
    return launch_for_tree<aov_kernel<double, true, B, 4, QUERY_TRAV_F64, true, false>,
                           aov_kernel<double, true, B, 4, QUERY_TRAV_F64, false, false>, B>(
        P, lds_bytes, stream, n, n_cu, 0, j, offsets, num_jobs, total, q_begin, n, remap, AovAcc{}, records, record_ids);
}

hipError_t launch_aov_reduce(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                             unsigned long long q_end, const double* records, const int32_t* record_ids,
                             int accumulate, void* carry, double* albedo, double* normal, double* depth, int32_t* id,
                             uint32_t* hits, hipStream_t stream) {
    return launch_1d(aov_reduce_kernel<double>, num_jobs, stream, offsets, num_jobs, q_begin, q_end, records,
                     record_ids, accumulate, (AovNear*)carry, albedo, normal, depth, id, hits);
}

// ---- second moments and refinement (rt_render_pixels_moments, rt_refine_jobs; rt_moments.h) ----
hipError_t launch_pixels_reduce_moments(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                                        unsigned long long q_end, const double* samples, const uint32_t* sample_segs,
                                        int accumulate, double* out_sums, double* out_sumsq, uint32_t* out_segments,
                                        hipStream_t stream) {
    return launch_1d(pixels_reduce_kernel<double, true>, num_jobs, stream, offsets, num_jobs, q_begin, q_end, samples,
                     sample_segs, accumulate, out_sums, out_sumsq, out_segments);
}

// fp32, one thread per job, before the path kernel: the second moment's two words start at 0,
// or (accumulate, a job that has samples) at X = rint((double)out_sq 2^38) for 0 <= out_sq <
// 2^57 -- high word X >> 32, low word X & 0xffffffff; a negative or NaN start is SQ_NAN, one of
// 2^57 or more SQ_INF.
__global__ void px_seed_moments_kernel(const unsigned long long* __restrict__ offsets, int num_jobs, int accumulate,
                                       const float* __restrict__ out_sq, unsigned long long* __restrict__ sq,
                                       uint32_t* __restrict__ sqflags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    uint32_t fl = 0;
    const bool cont = accumulate && offsets[k] != offsets[k + 1];
    for (int c = 0; c < 3; ++c) {
        unsigned long long lo = 0, hi = 0;
        if (cont) {
            const double s = (double)out_sq[(size_t)k * 3 + c];
            if (s != s || s < 0.0) {
                fl |= SQ_NAN << (2 * c);
            } else if (s >= 0x1p57) {
                fl |= SQ_INF << (2 * c);
            } else {   // X < 2^95: its halves are exact in doubles
                const double X = rint(dmul_rn(s, 0x1p38)), h = floor(dmul_rn(X, 0x1p-32));
                hi = (unsigned long long)h;
                lo = (unsigned long long)dsub_rn(X, dmul_rn(h, 0x1p32));
            }
        }
        sq[((size_t)k * 3 + c) * 2] = lo;
        sq[((size_t)k * 3 + c) * 2 + 1] = hi;
    }
    sqflags[k] = fl;
}

// ... and after it: out_sq = (float)(((double)high 2^32 + (double)low) 2^-38), NaN or +inf for
// a flagged channel (NaN wins); with accumulate a job without samples keeps what out_sq holds.
__global__ void px_finalize_moments_kernel(const unsigned long long* __restrict__ offsets, int num_jobs,
                                           int accumulate, const unsigned long long* __restrict__ sq,
                                           const uint32_t* __restrict__ sqflags, float* __restrict__ out_sq) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_jobs) return;
    if (accumulate && offsets[k] == offsets[k + 1]) return;
    for (int c = 0; c < 3; ++c) {
        const uint32_t f = (sqflags[k] >> (2 * c)) & 3u;
        const unsigned long long lo = sq[((size_t)k * 3 + c) * 2], hi = sq[((size_t)k * 3 + c) * 2 + 1];
        float v;
        if (f & SQ_NAN)
            v = __builtin_nanf("");
        else if (f)
            v = __builtin_huge_valf();
        else
            v = (float)dmul_rn(dmul_rn((double)hi, 0x1p32) + (double)lo, 0x1p-38);
        out_sq[(size_t)k * 3 + c] = v;
    }
}

hipError_t launch_pixels_seed_moments(const unsigned long long* offsets, int num_jobs, int accumulate,
                                      const float* out_sumsq, unsigned long long* sq, uint32_t* sqflags,
                                      hipStream_t stream) {
    return launch_1d(px_seed_moments_kernel, num_jobs, stream, offsets, num_jobs, accumulate, out_sumsq, sq, sqflags);
}

hipError_t launch_pixels_finalize_moments(const unsigned long long* offsets, int num_jobs, int accumulate,
                                          const unsigned long long* sq, const uint32_t* sqflags, float* out_sumsq,
                                          hipStream_t stream) {
    return launch_1d(px_finalize_moments_kernel, num_jobs, stream, offsets, num_jobs, accumulate, sq, sqflags,
                     out_sumsq);
}

hipError_t launch_refine_jobs(void* jobs, int num_jobs, const void* sums, const void* sumsq, int elem_bytes,
                              double rel_error, double abs_floor, uint32_t min_samples, uint32_t max_samples,
                              uint32_t max_step, unsigned long long* stats, hipStream_t stream) {
    const AdaptiveParams A{rel_error, abs_floor, min_samples, max_samples, max_step, 0u};
    if (elem_bytes == 8)
        return launch_1d(refine_jobs_kernel<double>, num_jobs, stream, (PixelJob*)jobs, num_jobs, (const double*)sums,
                         (const double*)sumsq, A, stats);
    return launch_1d(refine_jobs_kernel<float>, num_jobs, stream, (PixelJob*)jobs, num_jobs, (const float*)sums,
                     (const float*)sumsq, A, stats);
}

hipError_t launch_seed_accum(const float* out, long long* accum, uint32_t* flags, size_t npx, hipStream_t stream) {
    return launch_1d(seed_accum_kernel, npx, stream, out, accum, flags, npx);
}

}  // namespace rtx
