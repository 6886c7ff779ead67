// rt_ctx.h -- the context behind the C ABI (include/rt_hip.h) and the helpers its
// implementation files share (rt_abi.cpp: scene, render, frames; rt_plan.cpp: the launch plan;
// rt_comm.cpp: RCCL).
// Internal: not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <array>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_devbuf.h"
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_lbvh.h"
#include "rt_pack.h"

using namespace rtx;

// What a context owns, and the order it goes in (rt_destroy is `delete`): ~rt_ctx's body makes
// the device current, waits for the context's stream and frees the pinned staging buffer; then
// rt_ctx's members go, which is every byte of device memory (DevBuf: the scene, the mesh
// builder's scratch, the scratch of the calls, the Accum slots); then the base, ~rt_ctx_base:
// the communicator, the events, the stream.  A DevBuf member added to rt_ctx is freed with the
// rest, in that place; the base holds no device memory.
struct rt_ctx_base {
    int device = 0;
    int precision = RT_PREC_F32;
    uint64_t seed = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    std::string err;
    // RCCL communicator (rt_comm_init_rank / rt_comm_init_all): rank comm_rank of comm_size
    void* comm = nullptr;   // ncclComm_t
    int comm_rank = 0, comm_size = 0;
    bool comm_nonblocking = false;   // made by rt_comm_init_rank[_timeout] (ncclConfig_t.blocking = 0)

    rt_ctx_base() = default;
    rt_ctx_base(const rt_ctx_base&) = delete;
    ~rt_ctx_base();   // rt_abi.cpp
};

struct rt_ctx : rt_ctx_base {
    ~rt_ctx();   // rt_abi.cpp

    // measured best (tools/sweep.py, tools/mesh_sweep.py; profiles/r01)
    rt_tuning tuning{1024, 6, 1.0, 0.25, 8, RT_TRAV_DEFAULT, 2, -1, 2.0, 65536, 16384, RT_MESH_BUILD_HOST, -1, -1, 0, 32, 8.0, 20.0, 48, 0, 0, -1, 2.0, 32};

    // The uploaded scene, device buffers and host facts together: rt_upload_scene_ex fills a
    // local one and moves it in, and `scene = Scene{}` forgets all of it at once.
    struct Scene {
        bool has_scene = false;
        DevBuf d_nodes;     // Node
        DevBuf d_sph;       // SphereF | SphereD
        DevBuf d_mat;       // MatF | MatD
        DevBuf d_big;       // SphereD
        DevBuf d_bigf;      // BigF: the big spheres relative to their near points (fp32 kernels)
        int n_nodes = 0, n_sph = 0, n_mat = 0, n_big = 0, depth = 0, leaves = 0, n_input = 0;
        int n_front = 0;   // spheres [0, n_front) are tested before the BVH (rt_tuning.front_spheres)
        float box_extent = 0.f;   // bound of |coordinate| over the node boxes (RenderParams::box_extent)
        DevBuf d_grid;              // fp32: the uniform sphere grid (GridHdr ...), when the scene suits one
        int grid_nodes = 0;         // its size in sizeof(Node) units (it takes the nodes' LDS region)
        GridHdr grid_hdr{};         // its header (RenderParams::grid)
        int grid_entries = 0;       // sphere references over its cells
        double grid_density = 0.0;  // the sphere_grid_density it was built with (rt_scene_info, ABI 10)
        SceneReach reach;           // where a launch's rays can start (rt_pack.h grid_reach_ok)
        DevBuf d_remap;     // int; rt_trace_rays: kernel id slot -> input index (spheres | big | triangles)
        DevBuf d_unmap;     // int; rt_trace_rays_from: input index -> Hit::id (d_remap's inverse), n_unmap entries
        int n_unmap = 0;
        DevBuf d_mnodes;    // Node4; mesh BVH (4-wide) + triangles (HBM-resident)
        DevBuf d_tris;      // TriF | TriD
        DevBuf d_tmeta;     // uint32_t; fp32: per-triangle meta words (leaf order), beside the 48-B TriF records
        int n_mnodes = 0, n_tris = 0, mdepth = 0, mleaves = 0;
        float mbox[6] = {};         // the mesh's box (lo xyz, hi xyz): union of the root's child boxes
    } scene;
    // r07: resumable flat grid walks (RenderParams::gsus_lanes / gsus_iters), from the
    // environment's RT_GRID_SUSPEND at rt_create
    int gsus_lanes = GSUS_DEFAULT_LANES, gsus_iters = GSUS_DEFAULT_ITERS;
    // r09: per-item candidate lists (RenderParams::batch_cap), from the environment's
    // RT_BATCH_CULL at rt_create
    int batch_cap = BATCH_CAND_CAP;
    // r10: waiting lanes adopt their own batch hits (RenderParams::batch_adopt), from the
    // environment's RT_BATCH_ADOPT at rt_create
    int batch_adopt = 1;
    LbvhScratch lbvh;           // GPU mesh-BVH build scratch

    // scratch for the host-in/host-out paths (grown on demand, outside timed code)
    DevBuf d_shard, d_frame;
    DevBuf d_segs, d_segs_frame;   // uint32_t
    DevBuf d_rgb;                  // int32_t
    DevBuf d_tape;                 // double
    DevBuf d_small;                // double: ray7 + out3
    DevBuf d_used;                 // int
    DevBuf d_samples;              // per-sample radiance of chunked launches
    DevBuf d_queue64;     // fp64 persistent lanes (f64_kernel 3): work-queue control block
    DevBuf d_queue_rad;   // rt_radiance_rays: the launch's per-XCD heads (a control block of its own)
    // rt_render_pixels / rt_camera_rays (grown on demand): the scan's offsets (num_jobs + 1 x 8 B)
    // and work space, a control block of per-XCD heads of their own, fp32: the per-job
    // fixed-point sums (num_jobs x 3) and flags, fp64: one pass's samples (x 3 doubles) and
    // segment counts
    DevBuf d_px_offsets;   // unsigned long long
    DevBuf d_px_scan;
    DevBuf d_queue_px;
    DevBuf d_px_acc;       // long long
    DevBuf d_px_flags;     // uint32_t
    DevBuf d_px_samples;   // double
    DevBuf d_px_sseg;      // uint32_t
    // rt_render_pixels_moments, fp32: the second moments' two words per job and channel
    // (num_jobs x 6) and their flags
    DevBuf d_px_sq;        // unsigned long long
    DevBuf d_px_sqflags;   // uint32_t
    // rt_render_pixels_aov: the per-job nearest hit (num_jobs x 16 B: fp32 one packed word, fp64
    // the (t, id) carried between passes); its sums use d_px_acc / d_px_flags twice over, its
    // fp64 records d_px_samples / d_px_sseg.  aov_combine: the wave combine before the atomics,
    // from the environment's RT_AOV_COMBINE at rt_create
    DevBuf d_aov_near;
    int aov_combine = 1;
    // rt_denoise (grown on demand): the two colour record images its passes ping-pong between and
    // the guide record image, width x height x 4 values of the context precision each
    DevBuf d_dn_a, d_dn_b, d_dn_guide;
    DevBuf d_gather;  // rt_render_frame_multi: all contexts' shards

    // fp32 fixed-point pixel sums (RenderParams::accum), one slot per output buffer the
    // context renders into: rt_render_range(accumulate=1) continues a slot exactly.
    struct Accum {
        const void* out = nullptr;   // the out_sums buffer these sums belong to
        int W = 0, H = 0, shard = 0, nshards = 0;
        DevBuf acc;     // long long, npx * 3
        DevBuf flags;   // uint32_t, npx
        DevBuf queue;   // persistent-lane work counter of launches into this buffer
        DevBuf accp;    // unsigned long long, npx * 2: one launch's packed sums
        uint64_t used = 0;           // LRU stamp
    };
    static constexpr int ACCUM_SLOTS = 4;
    Accum accum[ACCUM_SLOTS];
    uint64_t accum_clock = 0;
    int n_cu = 0;                  // compute units of the device
    unsigned long long* diag_buf = nullptr;   // set only inside rt_render_diag: the instrumented kernel runs (not owned)

    // 8-bit host-bound frames (rt_finish_frame_u8 / rt_render_frame_u8): device frame and
    // a pinned host staging buffer (DMA-able, so the copy runs at full PCIe rate)
    DevBuf d_rgb8;   // uint8_t
    void* h_pinned = nullptr;
    size_t pinned_cap = 0;
};

namespace rtx_abi {

inline int fail(rt_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(ctx, expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(ctx, RT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

inline int reserve(rt_ctx* c, DevBuf& b, size_t bytes) {
    HIPCHK(c, b.reserve(bytes));
    return RT_OK;
}

// The fp64 kernel (rt_tuning.f64_kernel; 0 = the measured best, rt_render_f64.hip)
// fp64 kernel: the tuning's, or (0) kernel 5 -- 4 over the sphere grid -- where the scene has
// a grid and the traversal flags ask for it, else 4; 5 without a grid runs as 4 (the same
// frame: the grid only picks which spheres are tested)
// (6, internal: kernel 5 with the flat walk, where the grid is one cell tall in y)
constexpr int F64_KERNEL_DEFAULT = 4, F64_KERNEL_GRID = 5, F64_KERNEL_GRID_FLAT = 6;

// rt_plan.cpp: the plan of one launch -- which render kernel runs (threads per workgroup,
// traversal flags, the register-budget key waves_per_eu of its instantiation; fp64: the
// f64_kernel), the mesh traversal stack entries per lane it keeps in LDS
// (RenderParams::mstack), its dynamic LDS per workgroup, and the workgroups of it a CU keeps
// resident (the smaller of the register and LDS limits, at least 1).  grid_in_reach: every ray
// the launch can start lies within the sphere grid's reach (grid_reach_ok), so a scene with a
// grid may walk it; queries that belong to no launch plan one within reach.
// kernel: the uninstrumented instantiation for (block, wpe, trav) or the f64_kernel; null where
// none is built -- block / trav / wpe are then the tuning's own key, for the refusal to name.
struct LaunchPlan {
    int block, trav, wpe, f64_kernel, mesh_stack;
    size_t lds_bytes;
    int wgs_per_cu;
    const rtx::RenderKernel* kernel;
};
LaunchPlan plan_launch(const rt_ctx* c, bool grid_in_reach);
// rt_plan.cpp: what a job-list query (call: RT_QUERY_PIXELS rt_render_pixels, RT_QUERY_MOMENTS
// rt_render_pixels_moments, RT_QUERY_AOV rt_render_pixels_aov; reported by rt_pixels_plan[_call])
// runs for a camera whose reach proof gave grid_in_reach; call < 0: a per-ray query, the tree.  grid: 0 for the sphere tree, else TRAV_GRID or TRAV_GRID | TRAV_GFLAT -- the one
// value the kernel's instantiation, lds_bytes and apply_grid's view of the scene all follow.
// trav: that kernel's flags (0 for an fp64 tree); lds_bytes may exceed 160 KiB, which the
// caller answers with RT_ERR_LIMIT (then the tree's does not fit either).
struct QueryPlan {
    int grid, trav, block, mesh_stack;
    size_t lds_bytes;
};
QueryPlan plan_job_query(const rt_ctx* c, int call, bool grid_in_reach);
int stack_entries(const rt_ctx* c);
size_t lds_scene_bytes_at(const rt_ctx* c, int block, int tr = 0);

}  // namespace rtx_abi

// rt_comm.cpp: drop the context's communicator (rt_destroy); the grouped gather of
// rt_render_frame_multi (every context rank r of n, shards in their d_shard)
void rt_comm_release(rt_ctx_base* c);
int rt_comm_gather_group(rt_ctx** cs, int n, size_t elems, void* gathered);
