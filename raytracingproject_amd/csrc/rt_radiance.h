// rt_radiance.h -- batched ray_color (rt_radiance_rays): camera_cpu.h:8-26 for many rays the
// caller supplies, each on its own RT-CRNG-1 stream (rt_path_key), one radiance per ray.
//
// The bounce loop is render_lanes' (rt_render_impl.h) without a camera and without sums:
//   * fp64 (EXACT): closest_hit<double, true, ...> with no self-primitive rule, the path's
//     attenuations kept per bounce and multiplied innermost-first when the ray leaves the
//     scene (camera_cpu.h:19) -- the reference's ray_color bit for bit;
//   * fp32: thr = thr * att, mul_rn(thr, sky), and every scattered segment names the primitive
//     it starts on (self_id); the caller's first segment names none.
// rt_radiance_rays walks the tree, never the sphere grid (whose reach proof is made per launch
// camera, and these rays have none), with the traversal flags of rt_trace_rays, so a ray's first
// segment finds what rt_trace_rays finds.  The job-list kernels that share path_loop
// (rt_pixels.h, rt_moments.h) have a camera: for sphere-only scenes they are instantiated over
// the grid as well (TRAV | TRAV_GRID, and | TRAV_GFLAT), and the call's plan (rt_plan.cpp
// plan_job_query) picks one -- the same hit, so the same output bits.
//
// Paths last 1 .. max_depth segments, so lanes are persistent: a lane whose path has ended
// takes the next unclaimed ray index and goes on in the same bounce loop.  The hand-out is per
// wave -- a ballot of the lanes that need a ray, one returning atomic by the wave's first
// active lane for that many indices, v_mbcnt for a lane's rank among them.
// The head is sharded per XCD as render_lanes' work queue is (QUEUE_HEADS words 128 B apart in
// RenderParams::queue, zeroed on the stream before the launch): short paths claim often -- 4.1 M
// depth-1 rays are 64,800 claims, 0.74 ms at the ~88 claims/us one head word sustains, and the
// kernel takes 0.21 ms with eight (DESIGN.md §5 "rt_radiance_rays").  Head q hands out the
// 64-ray chunks q, q + 8, q + 16, ... of the batch: its counter value c is ray
// ((c / 64) * 8 + q) * 64 + c % 64.  A wave starts at its XCD's head (speed only -- any wave
// may claim from any head) and moves to the next when a claim runs past the batch's end; a
// head's rays ascend with its counter, so a head that gave one index >= n has none left, and a
// lane that has gone round all heads is done.  Every ray's result goes to its own slot, so the
// output does not depend on which lane traced it, on the grid, or on how a batch is split.
#pragma once
#include "rt_render_impl.h"

namespace rtx {

struct PathKey {   // = rt_path_key (include/rt_hip.h)
    uint32_t pixel, sample, first_draw, pad;
};
static_assert(sizeof(PathKey) == 16, "rt_path_key");

// The persistent loop itself, shared by radiance_kernel, pixels_kernel (rt_pixels.h) and
// pixels_moments_kernel (rt_moments.h): the scene load, the lane's path state, the claim from the
// per-XCD heads of P.queue over indices [0, n), and the bounce loop in both arithmetics.  A
// caller supplies the two places where the kernels differ:
//   start(i, ray, rng)   the lane has claimed index i < n: set the path's first ray and start rng
//                        on its stream (and keep what finish needs to know of i);
//   finish(L, segs)      the path has ended with radiance L after segs closest_hit calls.
// Both run under divergence, by the claiming / finishing lanes only.  P.max_depth >= 1.
template <class R, bool EXACT, int BLOCK, int TRAV, bool MESH, class Start, class Finish>
__device__ __forceinline__ void path_loop(const RenderParams& P, int n, Start&& start, Finish&& finish) {
    static_assert(!EXACT || sizeof(R) == 8, "EXACT needs fp64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* s_stack;
    uint32_t* s_mstack;
    const SceneView<R> sc = load_scene_lds<R, BLOCK, TRAV, MESH>(P, smem, s_stack, s_mstack);
    __syncthreads();
    uint16_t* stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;

    bool live = false, fin = false;   // holds a path; the indices ran out for this lane
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
        // lanes without a path take the next indices (the whole wave runs this)
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
            // (64-bit: a head passes its last index by at most 64 per wave of the grid, times 8)
            const unsigned long long c = (unsigned long long)base + rank;
            const unsigned long long i = ((c >> 6) * QUEUE_HEADS + q) * 64 + (c & 63);
            const bool got = need && i < (unsigned long long)n;
            if (got) {
                start(i, ray, rng);
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
                finish(L, segs);
                live = false;
            }
        }
    }
}

// keys: n records, or null for {i, 0, 0} on ray i.  P.max_depth >= 1 (the C ABI answers
// max_depth <= 0 without a launch).  segments: null, or n counts of closest_hit calls.
template <class R, bool EXACT, int BLOCK, int MINW, int TRAV, bool MESH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(MINW))) void radiance_kernel(
    RenderParams P, const R* __restrict__ rays, int n, const PathKey* __restrict__ keys, R* __restrict__ radiance,
    uint32_t* __restrict__ segments) {
    int idx = 0;   // this lane's path: ray `idx` of the batch
    path_loop<R, EXACT, BLOCK, TRAV, MESH>(
        P, n,
        [&](unsigned long long i, Ray<R>& ray, CounterRng& rng) {
            idx = (int)i;
            const R* r7 = rays + (size_t)i * 7;
            ray.o = mk(r7[0], r7[1], r7[2]);
            ray.d = mk(r7[3], r7[4], r7[5]);
            ray.time = r7[6];
            uint32_t pixel = (uint32_t)i, sample = 0, first = 0;
            if (keys) {
                pixel = keys[i].pixel;
                sample = keys[i].sample;
                first = keys[i].first_draw;
            }
            rng.start(hash32(P.seed32 ^ pixel), sample);
            rng.skip(first);
        },
        [&](const V3<R>& L, uint32_t segs) {
            R* o = radiance + (size_t)idx * 3;
            o[0] = L.x;
            o[1] = L.y;
            o[2] = L.z;
            if (segments) segments[idx] = segs;
        });
}

// The grid of a launch over n rays: one lane per ray up to the workgroups the device keeps
// resident, by the kernel's registers (512 VGPRs per SIMD lane in 8-register granules, at most
// 8 waves per SIMD, 4 SIMDs) and by its LDS (160 KiB per CU) -- the render kernels' occupancy
// model (rt_plan.cpp).  Speed only: a workgroup that starts late claims what is left.
// (v: the kernel's VGPRs, radiance_vgprs -- asked of HIP once per kernel by the launchers, not
// per launch: the query is host time between the launch's two timing events.)
inline int radiance_vgprs(const void* kernel) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, kernel) == hipSuccess ? a.numRegs : -1;
}
template <int BLOCK>
inline int radiance_grid(int v, size_t lds_bytes, int n, int n_cu) {
    int waves = v > 0 ? 512 / ((v + 7) & ~7) : 8;
    if (waves > 8) waves = 8;
    int wgs = waves * 4 / (BLOCK / 64);
    const int by_lds = lds_bytes > 0 ? (int)((size_t)160 * 1024 / lds_bytes) : wgs;
    if (wgs > by_lds) wgs = by_lds;
    if (wgs < 1) wgs = 1;
    const long resident = (long)wgs * (n_cu > 0 ? n_cu : 256);
    const long want = ((long)n + BLOCK - 1) / BLOCK;
    return (int)(want < resident ? want : resident);
}

// One launch of a kernel of this family over n indices: its VGPRs asked once, the grid that stays
// resident, max_wgs > 0 (rt_tuning.grid_workgroups) a cap on it.
template <auto KERNEL, int BLOCK, class... Args>
inline hipError_t launch_resident(size_t lds_bytes, hipStream_t stream, int n, int n_cu, int max_wgs,
                                  const Args&... args) {
    static const int v = radiance_vgprs((const void*)KERNEL);
    int grid = radiance_grid<BLOCK>(v, lds_bytes, n, n_cu);
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(BLOCK), lds_bytes, stream, args...);
    return hipGetLastError();
}
// ... of the mesh or the sphere instantiation, by the scene; P is the kernels' first argument.
template <auto MESH_KERNEL, auto SPHERE_KERNEL, int BLOCK, class... Args>
inline hipError_t launch_for_scene(const RenderParams& P, size_t lds_bytes, hipStream_t stream, int n, int n_cu,
                                   int max_wgs, const Args&... args) {
    return P.n_mnodes > 0 ? launch_resident<MESH_KERNEL, BLOCK>(lds_bytes, stream, n, n_cu, max_wgs, P, args...)
                          : launch_resident<SPHERE_KERNEL, BLOCK>(lds_bytes, stream, n, n_cu, max_wgs, P, args...);
}

// static LDS bytes of a kernel (-1: the query failed)
inline int kernel_static_lds(const void* kernel) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, kernel) == hipSuccess ? (int)a.sharedSizeBytes : -1;
}
// A sphere kernel over the grid.  The kernel's TRAV and the parameters the host sized for it must
// be one pair: a grid kernel reads P.nodes as the grid, by LDS byte address from 0, and has no
// traversal stack, so P must be what apply_grid (rt_abi.cpp) made of it -- the grid's header, no
// stack, a sphere-only scene -- and the kernel must have no static LDS (asked once).  Anything
// else is refused before the launch.
template <auto KERNEL, int BLOCK, class... Args>
inline hipError_t launch_grid_resident(const RenderParams& P, size_t lds_bytes, hipStream_t stream, int n, int n_cu,
                                       int max_wgs, const Args&... args) {
    static const int slds = kernel_static_lds((const void*)KERNEL);
    if (slds != 0 || P.n_mnodes > 0 || P.stack_size != 0 || P.n_nodes <= 0 || P.grid.res[0] <= 0)
        return hipErrorInvalidValue;
    return launch_resident<KERNEL, BLOCK>(lds_bytes, stream, n, n_cu, max_wgs, P, args...);
}
// ... of the grid kernel a job-list query's plan names: grid = TRAV_GRID the 3-D walk, TRAV_GRID |
// TRAV_GFLAT the flat walk (of a grid one cell tall in y).
template <auto GRID_KERNEL, auto GFLAT_KERNEL, int BLOCK, class... Args>
inline hipError_t launch_for_grid(const RenderParams& P, int grid, size_t lds_bytes, hipStream_t stream, int n,
                                  int n_cu, int max_wgs, const Args&... args) {
    if (grid == (TRAV_GRID | TRAV_GFLAT))
        return P.grid.res[1] != 1
                   ? hipErrorInvalidValue
                   : launch_grid_resident<GFLAT_KERNEL, BLOCK>(P, lds_bytes, stream, n, n_cu, max_wgs, args...);
    if (grid == TRAV_GRID) return launch_grid_resident<GRID_KERNEL, BLOCK>(P, lds_bytes, stream, n, n_cu, max_wgs, args...);
    return hipErrorInvalidValue;
}
// ... and of its tree kernels (grid = 0, launch_for_scene), which take P as fill_params made it:
// no grid header.
template <auto MESH_KERNEL, auto SPHERE_KERNEL, int BLOCK, class... Args>
inline hipError_t launch_for_tree(const RenderParams& P, size_t lds_bytes, hipStream_t stream, int n, int n_cu,
                                  int max_wgs, const Args&... args) {
    if (P.grid.res[0] != 0) return hipErrorInvalidValue;
    return launch_for_scene<MESH_KERNEL, SPHERE_KERNEL, BLOCK>(P, lds_bytes, stream, n, n_cu, max_wgs, args...);
}

}  // namespace rtx
