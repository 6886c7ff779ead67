// rt_plan.cpp -- the launch plan of a context's scene (rt_ctx.h plan_launch): the occupancy
// model of the render kernels (registers and LDS per workgroup) and the search over the
// instantiated candidates.  Pure host arithmetic over the context's scene sizes and tuning,
// plus the kernels' register counts (render_kernel_attrs).
#include <algorithm>

#include "rt_ctx.h"
#include "rt_launch.h"

using namespace rtx;

namespace rtx_abi {

// LDS traversal-stack entries per lane.  A far child is pushed only at an inner node with
// both children hit, and each pending one belongs to a distinct ancestor of the node being
// visited, so at most `depth` (inner levels) are pending; the latest sits in a register
// (closest_hit's `top`), the rest in LDS.
int stack_entries(const rt_ctx* c) { return c->scene.depth > 1 ? c->scene.depth - 1 : 1; }

// LDS of the sphere scene copy and the traversal stacks of one workgroup (kernel flags tr:
// TRAV_GRID kernels hold the grid where the tree's nodes go, and no traversal stack).
size_t lds_scene_bytes_at(const rt_ctx* c, int block, int tr) {
    const bool grid = (tr & TRAV_GRID) != 0;
    const size_t sph = c->precision == RT_PREC_F64 ? sizeof(SphereD) : sizeof(SphereF);
    const size_t mat = c->precision == RT_PREC_F64 ? sizeof(MatD) : sizeof(MatF);
    const size_t stack = grid ? 0 : (size_t)block * (size_t)stack_entries(c) * 2;
    return (size_t)(grid ? c->scene.grid_nodes : c->scene.n_nodes) * sizeof(Node) + (size_t)c->scene.n_sph * sph +
           (size_t)c->scene.n_mat * mat + (size_t)c->scene.n_big * (sizeof(SphereD) + sizeof(BigF)) + ((stack + 15) & ~(size_t)15);
}


namespace {

// The planner of one launch: the context's scene and tuning, and whether the launch may walk
// the sphere grid.
struct Planner {
    const rt_ctx* c;
    // the sphere grid serves the launch: built, and every ray the launch can start lies
    // within its walk's reach (grid_reach_ok; otherwise the tree, the same frame)
    bool grid_usable;

    // ...and is one cell tall in y, so that its walk steps in x and z only (TRAV_GFLAT, r06),
    // unless the tuning keeps the 3-D walk (TRAV_G3D)
    bool grid_flat() const {
        return grid_usable && c->scene.grid_hdr.res[1] == 1 && !(c->tuning.traversal & TRAV_G3D);
    }
    int f64_kernel_of() const {
        const int k = c->tuning.f64_kernel > 0 ? c->tuning.f64_kernel
                      : (c->tuning.traversal & TRAV_GRID) ? F64_KERNEL_GRID : F64_KERNEL_DEFAULT;
        if (k != F64_KERNEL_GRID) return k;
        return !grid_usable ? F64_KERNEL_DEFAULT : grid_flat() ? F64_KERNEL_GRID_FLAT : k;
    }

    // The uninstrumented render kernel at (block, tr, wpe) -- fp64: the f64_kernel -- or null.
    const RenderKernel* kernel_at(int block, int tr, int wpe) const {
        const bool mesh = c->scene.n_mnodes > 0;
        return c->precision == RT_PREC_F64 ? find_render_f64(f64_kernel_of(), mesh)
                                           : find_render_f32(block, wpe, tr, mesh, false);
    }

    // LDS of the sphere part of one workgroup at (block, kernel flags tr): the scene copy and
    // stacks, plus the coherent kernel's per-wave FIFO (+ item sums) and constants block.
    size_t lds_sphere_bytes_bt(int block, int tr) const {
        const bool f32 = c->precision == RT_PREC_F32;
        const size_t nw = (size_t)(block / 64);
        const size_t coh = c->scene.n_mnodes > 0 || !(tr & TRAV_COH)
                               ? 0
                               : nw * coh_wave_bytes(false, (tr & TRAV_NOSUM) == 0, coh_fifo_entries(tr), !f32, false,
                                                    coh_cands(false, tr, !f32)) +
                                     COH_CAM_BYTES;
        return lds_scene_bytes_at(c, block, tr) + coh;
    }

    // LDS of a mesh scene's per-lane state beyond the sphere part, with `s` mesh traversal
    // stack entries per lane in LDS (the rest in scratch).  fp32 mesh kernels also keep each
    // lane's three item sums (floats) in LDS; the coherent kernel (fp32) puts its per-wave FIFO
    // + item sums and the CohConst block there instead.
    size_t lds_mesh_bytes_at(int block, int tr, int s) const {
        if (c->scene.n_mnodes == 0) return 0;
        const size_t stack = (size_t)block * (size_t)s * 4;
        const bool f64 = c->precision != RT_PREC_F32;
        if (tr & TRAV_COH)
            return stack +
                   (size_t)(block / 64) *
                       coh_wave_bytes(true, (tr & TRAV_NOSUM) == 0, coh_fifo_entries(tr), f64, coh_parks(true, tr, f64)) +
                   COH_CAM_BYTES;
        if (f64) return stack;
        return stack + (size_t)block * 3 * sizeof(float);
    }

    // Workgroups of the render kernel (block, traversal tr, waves_per_eu key wpe) that the
    // register file lets share a CU (LDS aside): 512 VGPRs per SIMD lane, 8-register granules,
    // at most 8 waves per SIMD, 4 SIMDs.
    int wgs_per_cu_bt(int block, int tr, int wpe) const {
        const int v = render_kernel_attrs(kernel_at(block, tr, wpe)).vgprs;
        int waves = v > 0 ? 512 / ((v + 7) & ~7) : 8;
        if (waves > 8) waves = 8;
        const int wgs = waves * 4 / (block / 64);
        return wgs > 0 ? wgs : 1;
    }

    // Workgroups per CU by registers and by the LDS a workgroup needs with s mesh stack
    // entries per lane in LDS.
    int occupancy_at(int block, int tr, int wpe, int s) const {
        const int reg = wgs_per_cu_bt(block, tr, wpe);
        const size_t need = lds_sphere_bytes_bt(block, tr) + lds_mesh_bytes_at(block, tr, s);
        const int lds = need > 0 ? (int)(160 * 1024 / need) : 64;
        return reg < lds ? reg : lds;
    }

    // Mesh traversal stack entries per lane kept in LDS: the tuning's mesh_lds_stack, or (-1,
    // the default) the most entries up to MESH_LDS_STACK_AUTO that cost no workgroup per CU.
    // A mesh-only scene keeps all 12 at six 256-thread workgroups; the mixed scene's 512-thread
    // workgroups carry the sphere scene as well and reach 3 per CU (6 waves per SIMD with the
    // 6-wave kernel) only with the whole mesh stack in scratch: C5 geometry at 4K @ 32 takes
    // 55.6 ms that way against 63.0 ms with 12 LDS entries at 2 per CU (r04f mw6c5).
    static constexpr int MESH_LDS_STACK_AUTO = 12;
    // r06: none for the mixed-scene kernels over the sphere grid -- the C5 geometry at 4K @ 1024
    // ran 1,525.6-1,528.5 ms with the whole mesh stack in scratch against 1,567.5-1,569.1 with the
    // 5 LDS entries that cost no workgroup (2 entries: 1,565.4-1,566.8), frames identical, though
    // its traffic per launch rises 32.6 -> 38.3 GB at 4K @ 32 (profiles/r06/r06h, r06i, r06j);
    // mesh-only C4 keeps its 12 (none: +9 %).
    int mesh_stack_bt(int block, int tr, int wpe) const {
        if (c->scene.n_mnodes == 0) return 0;
        if (c->tuning.mesh_lds_stack >= 0) return c->tuning.mesh_lds_stack;
        if (tr & TRAV_GRID) return 0;
        const int most = occupancy_at(block, tr, wpe, 0);
        for (int s = MESH_LDS_STACK_AUTO; s > 0; --s)
            if (occupancy_at(block, tr, wpe, s) >= most) return s;
        return 0;
    }

    // Workgroups per CU at (block, tr, wpe) by registers and by the LDS a workgroup needs.
    int occupancy_bt(int block, int tr, int wpe) const {
        return occupancy_at(block, tr, wpe, mesh_stack_bt(block, tr, wpe));
    }

    // The kernel the context's scene runs: threads per workgroup, traversal flags and the
    // register-budget key (waves_per_eu) of its instantiation.
    //  * fp64: the block of the f64_kernel (the flags are not used);
    //  * fp32 spheres: the tuning's block and waves_per_eu; the coherent kernel drops its LDS
    //    pixel sums (TRAV_NOSUM) where they would cost a workgroup per CU;
    //  * fp32 meshes: mesh_block, or (0 = auto) whichever of 256 / 512 / 768 keeps more waves
    //    resident per CU, counting registers and LDS: a mesh-only scene fits six 256-thread
    //    workgroups with the 6-wave kernel (24 waves) against three of 512; with the sphere
    //    scene also in LDS the bigger workgroups win (bench_mesh_block_r01al.jsonl), and of
    //    those the 768-thread ones keep the item sums and two LDS stack entries (r05).  At
    //    each block the coherent kernel keeps its LDS item sums unless they cost occupancy,
    //    and mesh_waves_per_eu -1 (the default) weighs the 6-wave kernels (<= 80 VGPRs) against
    //    the compiler's budget (0, 5 waves per SIMD) the same way -- equal occupancy keeps the
    //    unspilled one.  The 6-wave kernels measured C4 37.7-37.9 ms against 39.7-40.0 and C5
    //    geometry (with the mesh stack in scratch, above) 55.6 against 63.0 ms, frames identical
    //    (profiles/r04/mw6_ab_r04f.txt).
    // (fills block, trav and wpe; plan_launch derives the rest from them)
    LaunchPlan plan_of() const {
        int t = c->tuning.traversal;
        if (c->precision != RT_PREC_F32 || c->scene.n_mnodes == 0) t &= ~TRAV_MIFIF;   // fp32 mesh kernels only
        // the if-if mesh loop is added wherever it is instantiated unless the while-while loop
        // (TRAV_MWHILE, never part of a kernel key) is asked for
        const bool want_mifif = (t & TRAV_MIFIF) || !(t & TRAV_MWHILE);
        t &= ~(TRAV_MWHILE | TRAV_MIFIF | TRAV_GFLAT | TRAV_G3D);
        if (c->precision == RT_PREC_F64) {
            const RenderKernel* k = find_render_f64(f64_kernel_of(), false);   // (rt_set_tuning: an instantiated one)
            return {k ? k->block : -1, k ? k->trav : 0, 0};
        }
        // the sphere grid wherever the scene has one (build_sphere_grid): the fp32 sphere kernels,
        // the fp32 mixed-scene mesh kernels (74328 / 74456, candidates below) and, through
        // f64_kernel 5, fp64 (handled above); else the tree
        if (!grid_usable) t &= ~TRAV_GRID;
        // the flat walk (TRAV_GFLAT) wherever the grid is one cell tall in y and its kernel exists
        const bool flat = grid_flat();
        auto gflat = [&](int b, int w, int x, bool mesh) {
            return flat && (x & TRAV_GRID) && find_render_f32(b, w, x | TRAV_GFLAT, mesh, false) ? x | TRAV_GFLAT : x;
        };
        if (c->scene.n_mnodes == 0) {
            const int b = c->tuning.block, w = c->tuning.waves_per_eu;
            if ((t & TRAV_COH) && !(t & TRAV_NOSUM)) {
                const size_t base = lds_scene_bytes_at(c, b, t), nw = (size_t)(b / 64);
                const int fifo = coh_fifo_entries(t);
                const bool cand = coh_cands(false, t, false);   // (fp32 here: the grid kernels' lists)
                const size_t with = base + nw * coh_wave_bytes(false, true, fifo, false, false, cand) + COH_CAM_BYTES,
                             without = base + nw * coh_wave_bytes(false, false, fifo, false, false, cand) + COH_CAM_BYTES;
                // (occupancy counts registers too: a small scene whose sums only lower a
                // workgroup count the registers never reach keeps them)
                const int reg = wgs_per_cu_bt(b, t, w);
                if (std::min<size_t>(reg, 160 * 1024 / with) < std::min<size_t>(reg, 160 * 1024 / without))
                    t |= TRAV_NOSUM;
            }
            return {b, gflat(b, w, t, false), w};
        }
        if (!(t & TRAV_COH)) t &= ~TRAV_NOSUM;
        const int wt = c->tuning.mesh_waves_per_eu;
        const int t0 = t;
        LaunchPlan cand[12];
        int nc = 0;
        for (int b : {256, 512, 768}) {
            if (c->tuning.mesh_block > 0 && b != c->tuning.mesh_block) continue;
            // (an explicit budget alone; auto weighs the compiler's against the 6-wave kernels)
            const int ws[2] = {wt >= 0 ? wt : 0, 6};
            for (int wi = 0; wi < (wt >= 0 ? 1 : 2); ++wi)
            for (int gi = 0; gi < ((t & TRAV_GRID) ? 2 : 1); ++gi) {   // (the sphere grid, then the tree)
                const int w = ws[wi];
                const int t = gi ? t0 & ~TRAV_GRID : t0;
                // (the if-if loop where its kernel exists, decided before the LDS sums are weighed)
                auto mifif = [&](int x) {
                    return want_mifif && find_render_f32(b, w, x | TRAV_MIFIF, true, false) ? x | TRAV_MIFIF : x;
                };
                int tb = mifif(t);
                if ((t & TRAV_COH) && !(t & TRAV_NOSUM)) {
                    const int tn = mifif(t | TRAV_NOSUM);
                    const bool ok_with = find_render_f32(b, w, tb, true, false) != nullptr;
                    const bool ok_without = find_render_f32(b, w, tn, true, false) != nullptr;
                    // (an uninstantiated kernel has no register count: only instantiated ones compete)
                    if (!ok_with || (ok_without && occupancy_bt(b, tb, w) < occupancy_bt(b, tn, w))) tb = tn;
                }
                if (find_render_f32(b, w, tb, true, false)) cand[nc++] = {b, gflat(b, w, tb, true), w};
            }
        }
        // the if-if loop wherever one of its kernels serves the request: the while-while kernels
        // that remain (equality references) run only when asked for
        bool any_mifif = false;
        for (int i = 0; i < nc; ++i) any_mifif = any_mifif || (cand[i].trav & TRAV_MIFIF) != 0;
        // ...and never in its place: a coherent request whose (block, budget) has no if-if
        // kernel (512 threads at the compiler's budget has only the while-while 728) is refused
        // by the render with its own key instead of silently running another loop
        if (want_mifif && (t & TRAV_COH) && !any_mifif) nc = 0;
        // nothing instantiated: the tuning's own key, which the render refuses with its name
        // The most waves resident per CU wins; at equal waves the plan with the LDS item sums
        // (no per-sample 64-bit atomics to HBM), then the sphere grid over the sphere tree (worth
        // more than any number of LDS mesh-stack entries: the grid's lists take less LDS than the
        // tree's nodes, and C5's geometry ran 9.5 % faster with it, r05), then the one with more
        // mesh-stack entries in LDS (less scratch traffic), then the smaller block (the order above).  The mixed scene:
        // 512 threads reach 24 waves per CU only with neither (3 x 8 waves); 768 threads reach
        // them with both (2 x 12 waves, sums and 2 LDS entries), and win (r05).
        LaunchPlan best{c->tuning.mesh_block > 0 ? c->tuning.mesh_block : c->tuning.block, t, wt >= 0 ? wt : 0};
        long best_score = -1;
        for (int i = 0; i < nc; ++i) {
            if (any_mifif && !(cand[i].trav & TRAV_MIFIF)) continue;
            const int waves = occupancy_bt(cand[i].block, cand[i].trav, cand[i].wpe) * (cand[i].block / 64);
            const int sums = (cand[i].trav & TRAV_COH) && !(cand[i].trav & TRAV_NOSUM) ? 1 : 0;
            const int grid = (cand[i].trav & TRAV_GRID) ? 1 : 0;
            const long score = (long)waves * 4096 + sums * 1024 + grid * 512 +
                               mesh_stack_bt(cand[i].block, cand[i].trav, cand[i].wpe);
            if (score > best_score) {
                best = cand[i];
                best_score = score;
            }
        }
        return best;
    }
};

}  // namespace

LaunchPlan plan_launch(const rt_ctx* c, bool grid_in_reach) {
    const Planner p{c, c->scene.grid_nodes > 0 && grid_in_reach};
    LaunchPlan r = p.plan_of();
    r.f64_kernel = p.f64_kernel_of();
    r.kernel = p.kernel_at(r.block, r.trav, r.wpe);
    r.mesh_stack = p.mesh_stack_bt(r.block, r.trav, r.wpe);
    r.lds_bytes = p.lds_sphere_bytes_bt(r.block, r.trav) + p.lds_mesh_bytes_at(r.block, r.trav, r.mesh_stack);
    // persistent lanes: no more workgroups than the device keeps resident
    r.wgs_per_cu = std::max(1, p.occupancy_at(r.block, r.trav, r.wpe, r.mesh_stack));
    return r;
}

// A job-list query walks the sphere grid where a frame from the same camera would: a sphere-only
// scene with a grid, the tuning's traversal asking for it (read now, as rt_render reads it),
// the camera within the walk's reach, in fp64 an f64_kernel that resolves to a grid kernel (3 and
// 4 force the tree, as for frames) -- and the grid's layout at TRACE_BLOCK within the LDS, else
// the tree's, which may fit where the grid's does not.  Mesh and mixed scenes keep the tree: there
// is no grid instantiation of the query kernels for them.
// ...and where the grid was measured faster than the tree by more than the two spreads at every
// sample count (C3, 1080p, depth 50, 2 and 16 spp; DESIGN.md §5 "Queries over the sphere grid"):
// rt_render_pixels in both precisions and rt_render_pixels_moments in fp64 (pixels_kernel).  The
// fp32 moments kernel (0.95 / 0.99 of the tree's time, within the spreads) and the first-hit call
// (fp32 1.09 / 1.10; fp64 0.93 / 0.92, within the spreads at 2 spp) keep the tree, and have no
// grid instantiation.
static bool grid_pays(int call, bool f64) {
    return call == RT_QUERY_PIXELS || (call == RT_QUERY_MOMENTS && f64);
}

QueryPlan plan_job_query(const rt_ctx* c, int call, bool grid_in_reach) {
    const Planner p{c, c->scene.grid_nodes > 0 && grid_in_reach};
    const bool f64 = c->precision == RT_PREC_F64, mesh = c->scene.n_mnodes > 0;
    QueryPlan q;
    q.block = TRACE_BLOCK;
    q.mesh_stack = plan_launch(c, true).mesh_stack;
    const size_t mstack = (size_t)TRACE_BLOCK * (size_t)q.mesh_stack * 4;
    q.grid = 0;
    if (!mesh && p.grid_usable && (c->tuning.traversal & TRAV_GRID) && grid_pays(call, f64)) {
        const int k = p.f64_kernel_of();
        if (!f64 || k == F64_KERNEL_GRID || k == F64_KERNEL_GRID_FLAT)
            q.grid = TRAV_GRID | (p.grid_flat() ? TRAV_GFLAT : 0);
    }
    if (q.grid && lds_scene_bytes_at(c, TRACE_BLOCK, q.grid) + mstack > 160 * 1024) q.grid = 0;
    q.lds_bytes = lds_scene_bytes_at(c, TRACE_BLOCK, q.grid) + mstack;
    q.trav = f64 ? (q.grid ? QUERY_TRAV_F64 | q.grid : 0) : (mesh ? QUERY_TRAV_MESH : QUERY_TRAV_SPHERES) | q.grid;
    return q;
}

}  // namespace rtx_abi
