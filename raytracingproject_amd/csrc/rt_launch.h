// rt_launch.h -- host-side launchers exported by the per-precision kernel translation
// units and called by the C ABI (rt_abi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_trav.h"

namespace rtx {

struct RenderParams;

// One instantiated frame kernel, render_kernel<...> of rt_render_impl.h.  The kernel units keep
// one table of these per precision (rt_render_f32.hip, rt_render_f64.hip); every entry's key and
// kernel come from the same template arguments.
// block: 256, 448, 512, 768 or 1024 threads (4..16 tiles per workgroup, one scene copy in LDS);
// mesh: the scene has a triangle mesh (fewer instantiated variants); diag: the instrumented copy
// (rt_render_diag: loop utilisation counters and timeline stamps into P.diag), built for the
// kernels that render frames by default.
struct RenderKernel {
    int block, wpe, trav;   // the key, as the tuning and the plan name it (wpe 0: the compiler's budget)
    bool mesh, diag;
    int f64_kernel;         // rt_tuning.f64_kernel (3..6); 0 for fp32
    void (*fn)(RenderParams);   // the host handle of render_kernel<...>
};
const RenderKernel* find_render_f32(int block, int wpe, int trav, bool mesh, bool diag);   // null: not built
const RenderKernel* find_render_f64(int kernel, bool mesh);
// VGPRs per lane (they set how many workgroups share a CU) and static LDS bytes (the sphere
// grid's walk addresses its dynamic LDS from 0, so a grid kernel must have none); -1, -1 where
// HIP could not answer.  HIP is asked once per kernel and process; a failed query is not kept.
struct KernelAttrs { int vgprs, static_lds; };
KernelAttrs render_kernel_attrs(const RenderKernel* k);
// k over the work queue of P on persistent lanes: a workgroup per `block / 64` items, at most
// P.max_wgs; nothing to do is hipSuccess without a launch
hipError_t launch_render(const RenderKernel& k, const RenderParams& P, size_t lds_bytes, hipStream_t stream);

// The small kernels' launch: one thread per element of [0, n), 256 to a workgroup; nothing to do
// is hipSuccess without a launch.  The second form bounds the workgroups (max_grid) of a kernel
// that strides over the elements left, and gives it dynamic LDS.
template <class Kernel, class N, class... Args>
inline hipError_t launch_1d_capped(Kernel kernel, N n, N max_grid, size_t lds_bytes, hipStream_t stream,
                                   const Args&... args) {
    if (n <= 0) return hipSuccess;
    const N want = (n + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(want < max_grid ? want : max_grid)), dim3(256), lds_bytes, stream,
                       args...);
    return hipGetLastError();
}
template <class Kernel, class N, class... Args>
inline hipError_t launch_1d(Kernel kernel, N n, hipStream_t stream, const Args&... args) {
    return launch_1d_capped(kernel, n, n, 0, stream, args...);
}

// batched world.hit (rt_trace_rays, rt_trace_rays_from): n rays of 7 values (context precision)
// -> n rt_hit; origin_ids: null, or per ray the input id of the primitive it starts on, looked
// up in unmap (n_unmap entries)
constexpr int TRACE_BLOCK = 256, TRACE_MAX_GRID = 8192;   // (launch_1d_capped: the kernels stride over the rays left)
// The traversal flags of the query kernels: fp32 spheres (the default frame kernel's select root,
// whole-record LDS reads and pop culling), fp32 meshes (the if-if mesh loop), fp64 (conservative
// fp32 slabs).  The path kernel of rt_render_pixels (pixels_kernel; fp64: rt_render_pixels_moments' too) adds
// QUERY_GRID, or QUERY_GRID | QUERY_GFLAT, where the call's plan walks the sphere grid (rt_ctx.h
// plan_job_query) -- the `grid` argument of its launchers, 0 for the tree.  A mesh scene has no
// grid instantiation: grid != 0 there is refused.  The fp32 moments kernel and the first-hit
// kernels have none either: measured, the grid did not pay there.
constexpr int QUERY_TRAV_SPHERES = TRAV_SELROOT | TRAV_B128 | TRAV_CULL,
              QUERY_TRAV_MESH = TRAV_SELROOT | TRAV_CULL | TRAV_MIFIF, QUERY_TRAV_F64 = TRAV_F32BOX;
constexpr int QUERY_GRID = TRAV_GRID, QUERY_GFLAT = TRAV_GFLAT;
hipError_t launch_trace_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                            void* hits, const int* remap, const int* origin_ids, const int* unmap, int n_unmap,
                            bool diag);
hipError_t launch_trace_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                            void* hits, const int* remap, const int* origin_ids, const int* unmap, int n_unmap);
// batched any-hit visibility (rt_occluded): n rays as above, intervals: null (every ray over
// (0.001, inf)) or n records {tmin, tmax} of the context precision -> n bytes, 0 or 1
hipError_t launch_occluded_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* intervals, uint8_t* occluded);
hipError_t launch_occluded_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* intervals, uint8_t* occluded);
// batched ray_color (rt_radiance_rays): n rays as above, keys: null ({i, 0, 0} for ray i) or n
// rt_path_key -> n x 3 radiance values of the context precision and (segments: may be null) n
// closest-hit counts.  Persistent lanes that claim ray indices from the per-XCD heads of P.queue
// (QUEUE_CTRL_BYTES, zeroed on the stream by the caller); P.max_depth >= 1; n_cu: the device's compute units (<= 0: unknown),
// which with the kernel's registers and lds_bytes bound the grid to what stays resident.
hipError_t launch_radiance_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* keys, void* radiance, uint32_t* segments, int n_cu);
hipError_t launch_radiance_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* keys, void* radiance, uint32_t* segments, int n_cu);
// bytes of one fp64 sample record (3 doubles + one uint32, kept in two arrays): a pass of
// rt_render_pixels holds floor(sample_buffer_mb 2^20 / PX_SAMPLE_BYTES) samples
constexpr size_t PX_SAMPLE_BYTES = 28;
// sparse rendering (rt_render_pixels, rt_camera_rays; csrc/rt_pixels.h).  jobs: num_jobs
// rt_pixel_job (device); offsets: num_jobs + 1 64-bit values (device).
// launch_pixel_scan: offsets = the exclusive scan of the valid jobs' sample counts (pixel <
// npix, else 0), offsets[num_jobs] = T.  temp == null: only *temp_bytes is set, to what the
// scan needs; nothing is launched.
hipError_t launch_pixel_scan(const void* jobs, int num_jobs, uint32_t npix, unsigned long long* offsets, void* temp,
                             size_t* temp_bytes, hipStream_t stream);
// rt_camera_rays: flat samples [0, total) -> rays (7 values each), keys (rt_path_key), ray_job
// (may be null); P carries the camera and the seed only
constexpr long long CAMERA_RAYS_MAX_GRID = 65536;
hipError_t launch_camera_rays_f32(const RenderParams& P, hipStream_t stream, const void* jobs,
                                  const unsigned long long* offsets, int num_jobs, long long total, void* rays,
                                  void* keys, int32_t* ray_job);
hipError_t launch_camera_rays_f64(const RenderParams& P, hipStream_t stream, const void* jobs,
                                  const unsigned long long* offsets, int num_jobs, long long total, void* rays,
                                  void* keys, int32_t* ray_job);
// the fused path kernel over flat samples [q_begin, q_begin + n) of the list's `total`
// (= offsets[num_jobs]): persistent lanes as
// launch_radiance_* (P.queue zeroed by the caller, P.max_depth >= 1, the camera in P).
// fp32 adds into acc (num_jobs x 3 sums in units of 2^-28), flags (num_jobs) and segments
// (num_jobs, may be null); fp64 stores sample q at q - q_begin of samples (n x 3 doubles) and
// sample_segs (n).
hipError_t launch_pixels_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                             const unsigned long long* offsets, int num_jobs, unsigned long long total,
                             unsigned long long q_begin, int n,
                             unsigned long long* acc, uint32_t* flags, uint32_t* segments, int n_cu, int grid);
hipError_t launch_pixels_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                             const unsigned long long* offsets, int num_jobs, unsigned long long total,
                             unsigned long long q_begin, int n,
                             double* samples, uint32_t* sample_segs, int n_cu, int grid, int max_wgs = 0);
// fp64: one pass's samples [q_begin, q_end) into out_sums / out_segments (may be null), per job
// in sample order (pixels_reduce_kernel)
hipError_t launch_pixels_reduce(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                                unsigned long long q_end, const double* samples, const uint32_t* sample_segs,
                                int accumulate, double* out_sums, uint32_t* out_segments, hipStream_t stream);
// fp32: the per-job fixed-point sums before the path kernel -- 0, or (accumulate, valid jobs)
// seeded from out_sums as seed_accum_kernel does; out_segments (may be null) zeroed unless
// accumulate -- and after it: acc, flags -> out_sums (accumulate: valid jobs only)
hipError_t launch_pixels_seed(const unsigned long long* offsets, int num_jobs, int accumulate, const float* out_sums,
                              long long* acc, uint32_t* flags, uint32_t* out_segments, hipStream_t stream);
hipError_t launch_pixels_finalize(const unsigned long long* offsets, int num_jobs, int accumulate,
                                  const long long* acc, const uint32_t* flags, float* out_sums, hipStream_t stream);
// rt_render_pixels_moments (csrc/rt_moments.h): the launches above with the per-job second
// moment.  fp32: sq (num_jobs x 3 x 2 words: the low and high 32-bit halves of the squares,
// summed, in units of 2^-38) and sqflags (num_jobs) beside acc and flags, seeded from and
// finalized into out_sumsq; fp64: the reduction continues out_sumsq as it continues out_sums.
// max_wgs > 0 (rt_tuning.grid_workgroups) caps the path kernel's grid, here and in
// launch_pixels_f64.
hipError_t launch_pixels_moments_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                                     const unsigned long long* offsets, int num_jobs, unsigned long long total,
                                     unsigned long long q_begin, int n, unsigned long long* acc, uint32_t* flags,
                                     uint32_t* segments, unsigned long long* sq, uint32_t* sqflags, int n_cu,
                                     int max_wgs);
hipError_t launch_pixels_reduce_moments(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                                        unsigned long long q_end, const double* samples, const uint32_t* sample_segs,
                                        int accumulate, double* out_sums, double* out_sumsq, uint32_t* out_segments,
                                        hipStream_t stream);
hipError_t launch_pixels_seed_moments(const unsigned long long* offsets, int num_jobs, int accumulate,
                                      const float* out_sumsq, unsigned long long* sq, uint32_t* sqflags,
                                      hipStream_t stream);
hipError_t launch_pixels_finalize_moments(const unsigned long long* offsets, int num_jobs, int accumulate,
                                          const unsigned long long* sq, const uint32_t* sqflags, float* out_sumsq,
                                          hipStream_t stream);
// bytes of one fp64 first-hit record (7 doubles: albedo, normal, t; one int32 id, kept in two
// arrays): a pass of rt_render_pixels_aov holds floor(sample_buffer_mb 2^20 / AOV_SAMPLE_BYTES)
constexpr size_t AOV_SAMPLE_BYTES = 60;
// rt_render_pixels_aov (csrc/rt_aov.h): first-hit albedo, normal, depth, id and hit count per job
// over flat samples [q_begin, q_begin + n) of the list's `total`; remap: rt_trace_rays' id map.
// Not persistent (one segment per sample); the grid is what stays resident, as launch_pixels_*.
// fp32 adds into acc_albedo / acc_normal (num_jobs x 3 sums in units of 2^-28, with their flags;
// launch_pixels_seed / launch_pixels_finalize before and after), nearest (num_jobs words,
// float bits of t << 32 | id; launch_aov_seed / launch_aov_finalize) and hits; any of the four
// may be null.  combine: a wave's lanes of one job are reduced before the atomics (the default)
// or every sample issues its own; the outputs do not depend on it.
hipError_t launch_aov_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                          const unsigned long long* offsets, int num_jobs, unsigned long long total, const int* remap,
                          unsigned long long* acc_albedo, uint32_t* flags_albedo, unsigned long long* acc_normal,
                          uint32_t* flags_normal, unsigned long long* nearest, uint32_t* hits, int n_cu, bool combine);
hipError_t launch_aov_seed(const unsigned long long* offsets, int num_jobs, int accumulate, const float* depth,
                           const int32_t* id, unsigned long long* nearest, uint32_t* hits, hipStream_t stream);
hipError_t launch_aov_finalize(const unsigned long long* offsets, int num_jobs, int accumulate,
                               const unsigned long long* nearest, float* depth, int32_t* id, hipStream_t stream);
// fp64 stores sample q's record at q - q_begin of records (n x 7 doubles) and record_ids (n);
// launch_aov_reduce adds one pass's records [q_begin, q_end) per job in sample order into the
// outputs (each may be null) and keeps the nearest (t, id), carried between passes in `carry`
// (num_jobs x 16 bytes)
hipError_t launch_aov_f64(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                          const unsigned long long* offsets, int num_jobs, unsigned long long total,
                          unsigned long long q_begin, int n, const int* remap, double* records, int32_t* record_ids,
                          int n_cu);
hipError_t launch_aov_reduce(const unsigned long long* offsets, int num_jobs, unsigned long long q_begin,
                             unsigned long long q_end, const double* records, const int32_t* record_ids,
                             int accumulate, void* carry, double* albedo, double* normal, double* depth, int32_t* id,
                             uint32_t* hits, hipStream_t stream);
// rt_query_grid_f32.hip: launch_pixels_f32 for grid != 0 (it hands over): the fp32 sphere kernel
// over the grid, kept out of the render kernels' translation unit.  P, lds_bytes and grid are one plan's (rt_ctx.h plan_job_query, rt_abi.cpp
// apply_grid); a P that is not the grid's view of a sphere-only scene is hipErrorInvalidValue.
hipError_t launch_pixels_grid_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                                  const unsigned long long* offsets, int num_jobs, unsigned long long total,
                                  unsigned long long q_begin, int n, unsigned long long* acc, uint32_t* flags,
                                  uint32_t* segments, int n_cu, int grid);
// rt_refine_jobs: jobs (rt_pixel_job, device) rewritten in place from sums / sumsq (num_jobs x 3
// of elem_bytes 4 or 8) by rt_adaptive_params' fields; stats: two words, added to
hipError_t launch_refine_jobs(void* jobs, int num_jobs, const void* sums, const void* sumsq, int elem_bytes,
                              double rel_error, double abs_floor, uint32_t min_samples, uint32_t max_samples,
                              uint32_t max_step, unsigned long long* stats, hipStream_t stream);
// rt_denoise (csrc/rt_denoise.h, rt_denoise.hip): prepare, `iterations` a-trous passes of step
// 2^i that ping-pong between col_a and col_b, finish -- all on `stream`.  Images are width x
// height of elem_bytes 4 or 8; sumsq, counts, albedo (with hits), normal, depth and out_variance
// may be null; col_a, col_b, guide: scratch of width x height x 4 elements each, 4-element
// aligned.  The parameters are rt_denoise_params', validated by the caller.
struct DenoiseLaunch {
    int elem_bytes, width, height, samples, guide_samples, iterations, normal_log2_power;
    double sigma_depth, sigma_lum, lum_eps;
    const void *sums, *sumsq;
    const uint32_t* counts;
    const void *albedo, *normal, *depth;
    const uint32_t* hits;
    void *col_a, *col_b, *guide, *out, *out_variance;
};
hipError_t launch_denoise(const DenoiseLaunch& D, hipStream_t stream);
hipError_t launch_tape_f64(const RenderParams& P, int max_depth, const double* ray7, const double* tape, int tape_len,
                           double* out, int* used, hipStream_t stream);
// element: 4 (float/uint32) or 8 (double); channels: 1 or 3
hipError_t launch_unshard(const void* gathered, void* frame, int elem_bytes, int channels, int W, int H, int tiles_x,
                          int nshards, int max_shard_tiles, hipStream_t stream);
hipError_t launch_quantize(const void* frame, int elem_bytes, int32_t* rgb, size_t n, int spp, hipStream_t stream);
// gathered shard buffers -> row-major W*H*3 uint8 frame (unshard + write_color in one pass)
hipError_t launch_finish_u8(const void* gathered, int elem_bytes, uint8_t* rgb, int W, int H, int tiles_x,
                            int nshards, int max_shard_tiles, int spp, hipStream_t stream);
// sums of a sample-chunked launch: out[e] (+)= samples[0][e] + ... + samples[nsamples-1][e], in order
hipError_t launch_reduce(const void* samples, void* out, int elem_bytes, size_t n, int nsamples, int accumulate,
                         hipStream_t stream);
// fp32 fixed-point pixel sums (RenderParams::accum, 3 per pixel) -> float out_sums
hipError_t launch_finalize(long long* accum, const unsigned long long* packed, const uint32_t* flags, float* out,
                           size_t npx, hipStream_t stream);
// float out_sums -> fixed-point sums (continuing sums the context has no state for)
hipError_t launch_seed_accum(const float* out, long long* accum, uint32_t* flags, size_t npx, hipStream_t stream);
// continue the fixed-point sums where out still holds their finalized value, else re-seed
// that channel from out (a buffer reallocated at the same address, or changed by the caller)
hipError_t launch_reconcile_accum(const float* out, long long* accum, uint32_t* flags, size_t npx,
                                  hipStream_t stream);

}  // namespace rtx
