// rt_render_f32.hip -- fp32 fast path.  Built (raytracingproject_amd/build.py) with FMA
// contraction, hardware reciprocal / square root (-fno-hip-fp32-correctly-rounded-divide-sqrt:
// v_rcp_f32 / v_sqrt_f32 instead of the ~10-instruction IEEE sequences) and fp32
// denormals flushed; the parity tests bound the effect (<= 2 LSB vs the reference).
#include <algorithm>
#include <map>
#include <mutex>

#include "rt_occluded.h"   // (includes rt_render_impl.h)
#include "rt_radiance.h"
#include "rt_pixels.h"
#include "rt_moments.h"
#include "rt_aov.h"

namespace rtx {

// Batched world.hit (rt_trace_rays), fp32: the default kernel's traversal flags
// (select root, whole-record LDS reads for spheres, pop culling; meshes: the if-if mesh
// loop); DIAG counts loop utilisation (tools/sort_bound.py).
hipError_t launch_trace_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                            void* hits, const int* remap, const int* origin_ids, const int* unmap, int n_unmap,
                            bool diag) {
    constexpr int B = TRACE_BLOCK, TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    auto kernel = trace_kernel<float, false, B, TM, true>;
    if (P.n_mnodes == 0)
        kernel = diag ? trace_kernel<float, false, B, TS, false, true> : trace_kernel<float, false, B, TS, false>;
    return launch_1d_capped(kernel, n, TRACE_MAX_GRID, lds_bytes, stream, P, (const float*)rays, n, (TraceHit*)hits,
                            remap, origin_ids, unmap, n_unmap);
}

// Batched any-hit visibility (rt_occluded), fp32: launch_trace_f32's traversal flags, so that
// the primitive and box tests are the closest-hit query's instantiations.
hipError_t launch_occluded_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* intervals, uint8_t* occluded) {
    constexpr int B = TRACE_BLOCK, TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    const auto kernel =
        P.n_mnodes > 0 ? occluded_kernel<float, false, B, TM, true> : occluded_kernel<float, false, B, TS, false>;
    return launch_1d_capped(kernel, n, TRACE_MAX_GRID, lds_bytes, stream, P, (const float*)rays, n,
                            (const float*)intervals, occluded);
}

// Batched ray_color (rt_radiance_rays), fp32: launch_trace_f32's traversal flags, so that a
// ray's first segment is the closest-hit query's.  Register budgets: 8 waves per SIMD (<= 64
// VGPRs) for spheres, the sphere render kernels' -- the bounce loop without a camera and without
// sums takes 54 and spills nothing, so a small scene's LDS copy leaves the full 8 waves -- and
// the mesh render kernels' 6 (<= 80 VGPRs; 76, no spill) for meshes.
constexpr int RADIANCE_WPE = 8, RADIANCE_MESH_WPE = 6;
hipError_t launch_radiance_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* rays, int n,
                               const void* keys, void* radiance, uint32_t* segments, int n_cu) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    constexpr int TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    return launch_for_scene<radiance_kernel<float, false, B, RADIANCE_MESH_WPE, TM, true>,
                            radiance_kernel<float, false, B, RADIANCE_WPE, TS, false>, B>(
        P, lds_bytes, stream, n, n_cu, 0, (const float*)rays, n, (const PathKey*)keys, (float*)radiance, segments);
}

// Sparse rendering (rt_render_pixels), fp32: launch_radiance_f32's flags, register budgets and
// grid; the camera and the job search are live only while a lane takes a sample.  grid: what the
// call's plan walks (rt_launch.h); the kernels over the sphere grid are rt_query_grid_f32.hip's.
hipError_t launch_pixels_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                             const unsigned long long* offsets, int num_jobs, unsigned long long total,
                             unsigned long long q_begin, int n,
                             unsigned long long* acc, uint32_t* flags, uint32_t* segments, int n_cu, int grid) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    constexpr int TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    if (grid)
        return launch_pixels_grid_f32(P, lds_bytes, stream, jobs, offsets, num_jobs, total, q_begin, n, acc, flags,
                                      segments, n_cu, grid);
    return launch_for_tree<pixels_kernel<float, false, B, RADIANCE_MESH_WPE, TM, true>,
                           pixels_kernel<float, false, B, RADIANCE_WPE, TS, false>, B>(
        P, lds_bytes, stream, n, n_cu, 0, (const PixelJob*)jobs, offsets, num_jobs, total, q_begin, n, acc, flags,
        segments, (float*)nullptr, (uint32_t*)nullptr);
}

// rt_render_pixels_moments, fp32: launch_pixels_f32's tree flags, register budgets and grid (no
// kernel over the sphere grid: its atomics hide what the walk saves).
hipError_t launch_pixels_moments_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                                     const unsigned long long* offsets, int num_jobs, unsigned long long total,
                                     unsigned long long q_begin, int n, unsigned long long* acc, uint32_t* flags,
                                     uint32_t* segments, unsigned long long* sq, uint32_t* sqflags, int n_cu,
                                     int max_wgs) {
    if (n <= 0) return hipSuccess;
    constexpr int B = TRACE_BLOCK;
    constexpr int TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    return launch_for_tree<pixels_moments_kernel<B, RADIANCE_MESH_WPE, TM, true>,
                           pixels_moments_kernel<B, RADIANCE_WPE, TS, false>, B>(
        P, lds_bytes, stream, n, n_cu, max_wgs, (const PixelJob*)jobs, offsets, num_jobs, total, q_begin, n, acc, flags,
        segments, sq, sqflags);
}

// First-hit auxiliary outputs (rt_render_pixels_aov), fp32: launch_trace_f32's traversal flags,
// so a sample's record is rt_trace_rays'; launch_pixels_f32's register budgets and grid bound.
template <bool COMBINE>
static hipError_t launch_aov(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const PixelJob* jobs,
                             const unsigned long long* offsets, int num_jobs, unsigned long long total,
                             const int* remap, const AovAcc& A, int n_cu) {
    constexpr int B = TRACE_BLOCK;
    constexpr int TS = QUERY_TRAV_SPHERES, TM = QUERY_TRAV_MESH;
    return launch_for_tree<aov_kernel<float, false, B, RADIANCE_MESH_WPE, TM, true, COMBINE>,
                           aov_kernel<float, false, B, RADIANCE_WPE, TS, false, COMBINE>, B>(
        P, lds_bytes, stream, (int)total, n_cu, 0, jobs, offsets, num_jobs, total, 0ull, (int)total, remap, A,
        (float*)nullptr, (int32_t*)nullptr);
}

hipError_t launch_aov_f32(const RenderParams& P, size_t lds_bytes, hipStream_t stream, const void* jobs,
                          const unsigned long long* offsets, int num_jobs, unsigned long long total, const int* remap,
                          unsigned long long* acc_albedo, uint32_t* flags_albedo, unsigned long long* acc_normal,
                          uint32_t* flags_normal, unsigned long long* nearest, uint32_t* hits, int n_cu, bool combine) {
    if (total == 0) return hipSuccess;
    const PixelJob* j = (const PixelJob*)jobs;
    const AovAcc A{acc_albedo, flags_albedo, acc_normal, flags_normal, nearest, hits};
    return combine ? launch_aov<true>(P, lds_bytes, stream, j, offsets, num_jobs, total, remap, A, n_cu)
                   : launch_aov<false>(P, lds_bytes, stream, j, offsets, num_jobs, total, remap, A, n_cu);
}

hipError_t launch_aov_seed(const unsigned long long* offsets, int num_jobs, int accumulate, const float* depth,
                           const int32_t* id, unsigned long long* nearest, uint32_t* hits, hipStream_t stream) {
    return launch_1d(aov_seed_kernel<float>, num_jobs, stream, offsets, num_jobs, accumulate, depth, id, nearest, hits);
}

hipError_t launch_aov_finalize(const unsigned long long* offsets, int num_jobs, int accumulate,
                               const unsigned long long* nearest, float* depth, int32_t* id, hipStream_t stream) {
    return launch_1d(aov_finalize_kernel<float>, num_jobs, stream, offsets, num_jobs, accumulate, nearest, depth, id);
}

hipError_t launch_camera_rays_f32(const RenderParams& P, hipStream_t stream, const void* jobs,
                                  const unsigned long long* offsets, int num_jobs, long long total, void* rays,
                                  void* keys, int32_t* ray_job) {
    return launch_1d_capped(camera_rays_kernel<float>, total, CAMERA_RAYS_MAX_GRID, 0, stream, P, (const PixelJob*)jobs,
                            offsets, num_jobs, total, (float*)rays, (PathKey*)keys, ray_job);
}

// ---- the frame kernels (rt_launch.h RenderKernel) ---------------------------------------------
// An entry's key and its kernel, from the same template arguments.  W = 0 is the compiler's own
// register budget, which amdgpu_waves_per_eu spells 1.
template <int B, int W, int T, bool MESH = false, bool DIAG = false>
constexpr RenderKernel entry() {
    return {B, W, T, MESH, DIAG, 0, render_kernel<float, false, B, (W ? W : 1), DIAG, T, MESH>};
}

// The traversal keys, by the numbers the tuning, the tests, the tools and DESIGN.md know them by.
constexpr int DEFAULT = TRAV_SELROOT | TRAV_B128 | TRAV_COH | TRAV_CULL,   // the coherent kernel over the sphere tree
              NOSUM = DEFAULT | TRAV_NOSUM,                                // ... without its LDS item sums
              NOCULL = DEFAULT & ~TRAV_CULL, NOCULL_NOSUM = NOSUM & ~TRAV_CULL,   // ... without pop culling
              LANE = TRAV_SELROOT,                                         // one path per lane
              GRID = DEFAULT | TRAV_GRID, GRID_NOSUM = NOSUM | TRAV_GRID,  // the sphere grid, 3-D walk
              GFLAT = GRID | TRAV_GFLAT, GFLAT_NOSUM = GRID_NOSUM | TRAV_GFLAT,   // ... flat walk
              // meshes: the if-if mesh loop over the sphere tree, the sphere grid, the flat walk;
              // the while-while loop is NOSUM, the one-path-per-lane kernel LANE
              M_IFIF = DEFAULT | TRAV_MIFIF, M_IFIF_NOSUM = NOSUM | TRAV_MIFIF,
              M_GRID = M_IFIF | TRAV_GRID, M_GRID_NOSUM = M_IFIF_NOSUM | TRAV_GRID,
              M_GFLAT = M_GRID | TRAV_GFLAT, M_GFLAT_NOSUM = M_GRID_NOSUM | TRAV_GFLAT;
static_assert(DEFAULT == 600 && NOSUM == 728 && NOCULL == 88 && NOCULL_NOSUM == 216 && LANE == 8, "sphere tree keys");
static_assert(GRID == 66136 && GRID_NOSUM == 66264 && GFLAT == 197208 && GFLAT_NOSUM == 197336, "sphere grid keys");
static_assert(M_IFIF == 8792 && M_IFIF_NOSUM == 8920 && M_GRID == 74328 && M_GRID_NOSUM == 74456 &&
                  M_GFLAT == 205400 && M_GFLAT_NOSUM == 205528,
              "mesh keys");
constexpr bool MESH = true, SPHERES = false, DIAG = true;

// The instantiated (block, waves_per_eu, traversal) combinations (r04: the default kernel,
// its automatic no-LDS-sums form (128), the kernel without pop culling (88 / 216) for the
// culling equality tests, and the one-path-per-lane kernel that every coherent kernel is
// tested against; the time-binned trees 856 / 984 were removed).
//
// Scenes with a triangle mesh (MESH instantiation: HBM-resident mesh BVH): the if-if mesh
// loop (TRAV_MIFIF: 8792 / 8920 = 600 / 728 + 8192, with / without the LDS item sums) at
// both workgroup sizes the plan chooses from, within 80 VGPRs (6 waves per SIMD: C4 -5 %,
// C5 geometry -12 %, profiles/r04/mw6_ab_r04f.txt); as equality references the same loop
// at the compiler's budget (5 waves, the default of rounds 1-3), the while-while loop of
// rounds 1-3 (728, TRAV_MWHILE) and the one-path-per-lane kernel (8).  (7 waves, <= 72 VGPRs,
// spilled inside the traversal loop: C4 45.0 against 37.8 ms, r04i; not kept.)  (r04 removed the LDS
// tree-top kernels 4696 / 4824, measured -2.8 %, and the other 5-wave copies.)
// Whole-record sphere-BVH reads (TRAV_B128) are kept for meshes since r03ag: the mixed
// scene's sphere traversal gains 0.7-0.8 % (profiles/r03/mixed_b128_probe_r03ag.jsonl).
// r05: 768-thread workgroups (12 waves, two per CU = 6 waves per SIMD) for the mixed scene:
// one LDS copy of the sphere scene serves 12 waves instead of 8, which leaves room for the
// LDS item sums and two LDS mesh-stack entries per lane at the 6-wave occupancy (512-thread
// workgroups fit three per CU only without both).
// (r05 also built the quantised 64-B node kernels, 41560 / 41688: C4 +12 %, C5 +7 %, removed.)
// r06: the grid kernels again with the flat walk (TRAV_GFLAT, + 131072: 197208 / 197336 for
// spheres, 205400 / 205528 mixed), which the C ABI picks where the grid is one cell tall in y;
// the 3-D ones serve every other grid and the flat walk's equality tests (traversal | 262144).
//
// Instrumented builds (rt_render_diag): the same persistent kernels with loop-utilisation
// counters and phase / timeline stamps into P.diag, for exactly the instantiations that
// render frames; any other combination is refused, so the counters always describe the kernel
// that renders the frames.  Mesh scenes: the default mesh kernels (if-if loop, with / without
// LDS item sums) at the register budget they render with (6 waves per SIMD, <= 80 VGPRs), so
// that the occupancy, LDS stack depth and max_wgs the plan sized for them hold for the
// instrumented copy too.
//
// A new variant is one line here.  The entries stand in the order the kernels have always been
// instantiated in -- mesh, spheres, then the instrumented copies of each -- because the
// compiler's instruction order inside two of them depends on it (the one-path-per-lane mesh
// kernel and the instrumented 197336: one instruction each, tools/isa_compare.py).
constexpr RenderKernel F32_KERNELS[] = {
    entry<256, 6, M_IFIF, MESH>(), entry<512, 6, M_IFIF, MESH>(), entry<768, 6, M_IFIF, MESH>(),
    entry<256, 6, M_IFIF_NOSUM, MESH>(), entry<512, 6, M_IFIF_NOSUM, MESH>(), entry<768, 6, M_IFIF_NOSUM, MESH>(),
    entry<768, 6, M_GRID, MESH>(), entry<512, 6, M_GRID_NOSUM, MESH>(),
    entry<768, 6, M_GFLAT, MESH>(), entry<512, 6, M_GFLAT_NOSUM, MESH>(),
    entry<256, 0, M_IFIF, MESH>(), entry<512, 0, NOSUM, MESH>(), entry<512, 0, LANE, MESH>(),

    entry<1024, 8, DEFAULT>(), entry<1024, 8, NOSUM>(), entry<1024, 8, NOCULL>(), entry<1024, 8, NOCULL_NOSUM>(),
    entry<512, 8, LANE>(),
    entry<1024, 8, GRID>(), entry<1024, 8, GRID_NOSUM>(), entry<1024, 8, GFLAT>(), entry<1024, 8, GFLAT_NOSUM>(),

    entry<256, 6, M_IFIF, MESH, DIAG>(), entry<512, 6, M_IFIF, MESH, DIAG>(), entry<768, 6, M_IFIF, MESH, DIAG>(),
    entry<256, 6, M_IFIF_NOSUM, MESH, DIAG>(), entry<512, 6, M_IFIF_NOSUM, MESH, DIAG>(),
    entry<768, 6, M_IFIF_NOSUM, MESH, DIAG>(),
    entry<768, 6, M_GRID, MESH, DIAG>(), entry<512, 6, M_GRID_NOSUM, MESH, DIAG>(),
    entry<768, 6, M_GFLAT, MESH, DIAG>(), entry<512, 6, M_GFLAT_NOSUM, MESH, DIAG>(),

    entry<1024, 8, DEFAULT, SPHERES, DIAG>(), entry<1024, 8, NOSUM, SPHERES, DIAG>(),
    entry<512, 8, LANE, SPHERES, DIAG>(),
    entry<1024, 8, GRID, SPHERES, DIAG>(), entry<1024, 8, GRID_NOSUM, SPHERES, DIAG>(),
    entry<1024, 8, GFLAT, SPHERES, DIAG>(), entry<1024, 8, GFLAT_NOSUM, SPHERES, DIAG>(),
};

const RenderKernel* find_render_f32(int block, int wpe, int trav, bool mesh, bool diag) {
    for (const RenderKernel& k : F32_KERNELS)
        if (k.block == block && k.wpe == wpe && k.trav == trav && k.mesh == mesh && k.diag == diag) return &k;
    return nullptr;
}

KernelAttrs render_kernel_attrs(const RenderKernel* k) {
    static std::mutex mu;
    static std::map<const RenderKernel*, KernelAttrs> known;
    if (!k) return {-1, -1};
    std::lock_guard<std::mutex> g(mu);
    const auto it = known.find(k);
    if (it != known.end()) return it->second;
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, (const void*)k->fn) != hipSuccess) return {-1, -1};
    return known[k] = {a.numRegs, (int)a.sharedSizeBytes};
}

hipError_t launch_render(const RenderKernel& k, const RenderParams& P, size_t lds_bytes, hipStream_t stream) {
    const int waves = k.block / 64;
    long items = 0;   // the work queue's items (persistent lanes: resident workgroups only)
    for (int p = 0; p < P.nph; ++p) items += (long)P.shard_tiles * P.ph_k[p];
    int grid = (int)((items + waves - 1) / waves);
    if (grid > P.max_wgs) grid = P.max_wgs;
    if (grid == 0) return hipSuccess;
    void* args[] = {const_cast<RenderParams*>(&P)};
    return hipLaunchKernel((const void*)k.fn, dim3(grid), dim3(k.block), args, lds_bytes, stream);
}

}  // namespace rtx
