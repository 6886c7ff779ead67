// rt_abi.cpp -- implementation of the C ABI declared in include/rt_hip.h.
//
// Host-side responsibilities: pack the scene (rt_pack.cpp: validation, the trees of
// rt_bvh.cpp, the records of the LDS-resident kernel), own device memory and the stream, plan
// each launch (rt_plan.cpp), launch the kernels (rt_render_f32.hip / rt_render_f64.hip) and
// time them with HIP events on the stream they run on.  Every failure is reported as a
// negative status + message; there is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_lbvh.h"
#include "rt_ctx.h"

using namespace rtx;
using namespace rtx_abi;


namespace {

void free_scene(rt_ctx* c) { c->scene = rt_ctx::Scene{}; }

// the stream a call runs on: the caller's, or the context's
hipStream_t stream_of(rt_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }

// The end of a timed call, after its launches (e: the first error of them, reported under
// `what`): ev1 on the stream, and the context has a time to report.
int timed_end(rt_ctx* c, hipStream_t st, hipError_t e, const char* what) {
    if (e != hipSuccess) return fail(c, RT_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    HIPCHK(c, hipEventRecord(c->ev1, st));
    c->timed = true;
    return RT_OK;
}

size_t elem_bytes(const rt_ctx* c) { return c->precision == RT_PREC_F64 ? 8 : 4; }

// The render launch's view of the sphere scene for kernel flags tr: the grid in the nodes'
// place (RenderParams::nodes / n_nodes), no traversal stack.
void apply_grid(const rt_ctx* c, int tr, RenderParams& P) {
    if (!(tr & TRAV_GRID)) return;
    P.nodes = (const Node*)c->scene.d_grid.p;
    P.n_nodes = c->scene.grid_nodes;
    P.stack_size = 0;
    P.grid = c->scene.grid_hdr;
}

// the scene has a sphere grid and every ray a launch from cam can start lies within its
// walk's reach (rt_pack.h grid_reach_ok: a host-side proof, made once per launch and handed
// to the planner)
bool grid_in_reach(const rt_ctx* c, const rt_camera* cam) {
    return c->scene.grid_nodes > 0 && grid_reach_ok(c->scene.reach, c->scene.grid_hdr.far_o, *cam);
}

int check_camera(rt_ctx* c, const rt_camera* cam) {
    if (!cam) return fail(c, RT_ERR_INVALID, "camera is NULL");
    if (cam->image_width <= 0 || cam->image_height <= 0)
        return fail(c, RT_ERR_INVALID, "image size %dx%d", cam->image_width, cam->image_height);
    if ((long long)cam->image_width * cam->image_height > (1ll << 31) / 4)
        return fail(c, RT_ERR_LIMIT, "image too large");
    return RT_OK;
}

// what camera_ray reads of the parameters: the image size, the seed and the camera's vectors
// (rt_camera_rays needs no more, and no scene)
void fill_camera(const rt_ctx* c, const rt_camera* cam, RenderParams& P) {
    P.W = cam->image_width;
    P.H = cam->image_height;
    P.seed32 = seed32_of(c->seed);
    P.defocus = cam->defocus_angle > 0;  // camera.h:94 tests defocus_angle <= 0
    for (int a = 0; a < 3; ++a) {
        P.f_center[a] = (float)cam->center[a];
        P.f_p00[a] = (float)cam->pixel00_loc[a];
        P.f_du[a] = (float)cam->pixel_delta_u[a];
        P.f_dv[a] = (float)cam->pixel_delta_v[a];
        P.f_ddu[a] = (float)cam->defocus_disk_u[a];
        P.f_ddv[a] = (float)cam->defocus_disk_v[a];
        P.cam_center[a] = cam->center[a];
        P.p00[a] = cam->pixel00_loc[a];
        P.du[a] = cam->pixel_delta_u[a];
        P.dv[a] = cam->pixel_delta_v[a];
        P.ddu[a] = cam->defocus_disk_u[a];
        P.ddv[a] = cam->defocus_disk_v[a];
    }
}

void fill_params(const rt_ctx* c, const rt_camera* cam, int spp, int max_depth, int mesh_stack, RenderParams& P) {
    std::memset(&P, 0, sizeof(P));
    fill_camera(c, cam, P);
    P.spp = spp;
    P.max_depth = max_depth;
    P.tiles_x = (P.W + 7) / 8;
    P.tiles_x_inv = 1.0 / P.tiles_x;
    P.tiles_x_inv_half = 0.5 * P.tiles_x_inv;
    P.n_nodes = c->scene.n_nodes;
    P.n_spheres = c->scene.n_sph;
    P.n_mats = c->scene.n_mat;
    P.n_big = c->scene.n_big;
    P.n_front = c->scene.n_front;
    P.stack_size = stack_entries(c);
    P.nodes = c->scene.d_nodes.as<Node>();
    P.spheres = c->scene.d_sph.p;
    P.mats = c->scene.d_mat.p;
    P.big = c->scene.d_big.as<SphereD>();
    P.bigf = c->scene.d_bigf.as<BigF>();
    P.mnodes = c->scene.d_mnodes.as<Node4>();
    P.tris = c->scene.d_tris.p;
    P.tmeta = c->scene.d_tmeta.as<uint32_t>();
    P.n_mnodes = c->scene.n_mnodes;
    P.mstack = mesh_stack;
    P.box_extent = c->scene.box_extent;
    std::copy(c->scene.mbox, c->scene.mbox + 6, P.mbox);
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* rt_error_string(int code) {
    switch (code) {
        case RT_OK: return "ok";
        case RT_ERR_INVALID: return "invalid argument";
        case RT_ERR_HIP: return "HIP runtime error";
        case RT_ERR_NO_SCENE: return "no scene uploaded";
        case RT_ERR_LIMIT: return "scene or image exceeds kernel limits";
        case RT_ERR_COMM: return "RCCL error";
        default: return "unknown error";
    }
}

// RT_GRID_SUSPEND: "LANES,ITERS" (resumable flat grid walks, rt_device.h closest_hit SUSP),
// "0" for none; unset or empty keeps the defaults.  A tuning that is no rt_tuning field: the
// frame does not depend on it, and the ABI stays what it is.
static bool parse_grid_suspend(const char* s, int& lanes, int& iters) {
    if (!s || !*s) return true;
    int l = 0, i = 0, n = 0;
    if (sscanf(s, "%d,%d%n", &l, &i, &n) == 2 && !s[n] && l >= 1 && l <= 64 && i >= 1 && i <= 65535) {
        lanes = l;
        iters = i;
        return true;
    }
    if (s[0] == '0' && !s[1]) {
        lanes = 0;
        iters = 0x7fffffff;   // (one block: the countdown never ends a walk)
        return true;
    }
    return false;
}

// RT_BATCH_CULL: "0" (every camera-ray batch walks the grid) or the candidate lists' cap,
// 1..BATCH_CAND_CAP; unset or empty keeps the default.  Like RT_GRID_SUSPEND no rt_tuning
// field: the frame does not depend on it.
static bool parse_batch_cull(const char* s, int& cap) {
    if (!s || !*s) return true;
    int v = 0, n = 0;
    if (sscanf(s, "%d%n", &v, &n) == 1 && !s[n] && v >= 0 && v <= BATCH_CAND_CAP) {
        cap = v;
        return true;
    }
    return false;
}

// RT_BATCH_ADOPT: "1" (a lane waiting for a path keeps the hit of its own camera ray in a
// batch; the default, also unset or empty) or "0" (every primary hit goes through the FIFO,
// the kernel of before).  No rt_tuning field either: the frame does not depend on it.
static bool parse_batch_adopt(const char* s, int& on) {
    if (!s || !*s) return true;
    if ((s[0] != '0' && s[0] != '1') || s[1]) return false;
    on = s[0] - '0';
    return true;
}

rt_ctx* rt_create(int device, uint64_t seed, int precision) {
    if (precision != RT_PREC_F32 && precision != RT_PREC_F64) return nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    rt_ctx* c = new rt_ctx();
    c->device = device;
    c->seed = seed;
    c->precision = precision;
    // RT_AOV_COMBINE: "1" (rt_render_pixels_aov reduces a wave's lanes of one job before the
    // atomics; the default, also unset or empty) or "0" (one set of atomics per sample).  The
    // outputs do not depend on it.
    const struct {
        bool ok;
        const char* must;   // (a format of one int, BATCH_CAND_CAP)
    } env[] = {
        {parse_grid_suspend(getenv("RT_GRID_SUSPEND"), c->gsus_lanes, c->gsus_iters),
         "rt_create: RT_GRID_SUSPEND must be \"0\" or \"LANES,ITERS\" (1..64, 1..65535)\n"},
        {parse_batch_cull(getenv("RT_BATCH_CULL"), c->batch_cap), "rt_create: RT_BATCH_CULL must be 0..%d\n"},
        {parse_batch_adopt(getenv("RT_BATCH_ADOPT"), c->batch_adopt), "rt_create: RT_BATCH_ADOPT must be 0 or 1\n"},
        {parse_batch_adopt(getenv("RT_AOV_COMBINE"), c->aov_combine), "rt_create: RT_AOV_COMBINE must be 0 or 1\n"},
    };
    for (const auto& v : env)
        if (!v.ok) {
            fprintf(stderr, v.must, BATCH_CAND_CAP);
            delete c;
            return nullptr;
        }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) c->n_cu = 0;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        c->d_small.reserve(16 * sizeof(double)) != hipSuccess || c->d_used.reserve(sizeof(int)) != hipSuccess) {
        delete c;
        return nullptr;
    }
    return c;
}

// (the order: rt_ctx.h)
rt_ctx::~rt_ctx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (h_pinned) (void)hipHostFree(h_pinned);
}

rt_ctx_base::~rt_ctx_base() {
    rt_comm_release(this);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
}

void rt_destroy(rt_ctx* c) { delete c; }

const char* rt_last_error(const rt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int rt_set_seed(rt_ctx* c, uint64_t seed) {
    if (!c) return RT_ERR_INVALID;
    c->seed = seed;
    return RT_OK;
}

void* rt_stream(rt_ctx* c) { return c ? (void*)c->stream : nullptr; }

int rt_get_tuning(rt_ctx* c, rt_tuning* t) {
    if (!c || !t) return RT_ERR_INVALID;
    *t = c->tuning;
    return RT_OK;
}

int rt_set_tuning(rt_ctx* c, const rt_tuning* t) {
    if (!c || !t) return RT_ERR_INVALID;
    if (t->block != 256 && t->block != 448 && t->block != 512 && t->block != 768 && t->block != 1024)
        return fail(c, RT_ERR_INVALID, "block %d (256, 448, 512, 768 or 1024)", t->block);
    if (t->max_leaf < 1 || t->max_leaf > LEAF_MAX) return fail(c, RT_ERR_INVALID, "max_leaf %d", t->max_leaf);
    if (!(t->cost_traverse > 0) || !(t->cost_intersect > 0)) return fail(c, RT_ERR_INVALID, "SAH costs must be > 0");
    if (t->waves_per_eu != 0 && t->waves_per_eu != 4 && t->waves_per_eu != 6 && t->waves_per_eu != 8)
        return fail(c, RT_ERR_INVALID, "waves_per_eu 0, 4, 6 or 8");
    if (t->mesh_waves_per_eu != -1 && t->mesh_waves_per_eu != 0 && t->mesh_waves_per_eu != 6)
        return fail(c, RT_ERR_INVALID, "mesh_waves_per_eu -1 (auto: the instantiated kernel keeping more waves "
                                       "per CU), 0 (the compiler's register budget) or 6 (<= 80 VGPRs); 5 / 7 / 8 "
                                       "are not built (7 spilled inside the traversal loop: C4 +19 %)");
    if (t->coh_refill < 1 || t->coh_refill > 64) return fail(c, RT_ERR_INVALID, "coh_refill %d (1..64)", t->coh_refill);
    if (t->f64_kernel != 0 && (t->f64_kernel == F64_KERNEL_GRID_FLAT || !find_render_f64(t->f64_kernel, false)))
        return fail(c, RT_ERR_INVALID, "f64_kernel %d (0 = default, or an instantiated one)", t->f64_kernel);
    if (t->front_spheres < -1 || t->front_spheres > 16)
        return fail(c, RT_ERR_INVALID, "front_spheres %d (-1 = auto, 0..16)", t->front_spheres);
    if (!(t->sphere_grid_density >= 0 && t->sphere_grid_density <= 64))
        return fail(c, RT_ERR_INVALID, "sphere_grid_density %g (0 = no grid, up to 64 cells per sphere)",
                    t->sphere_grid_density);
    if (t->sphere_grid_time_slabs < 1 || t->sphere_grid_time_slabs > GRID_SLAB_MAX)
        return fail(c, RT_ERR_INVALID, "sphere_grid_time_slabs %d (1..%d)", t->sphere_grid_time_slabs, GRID_SLAB_MAX);
    if (t->grid_workgroups < 0 || t->grid_workgroups > (1 << 20))
        return fail(c, RT_ERR_INVALID, "grid_workgroups %d (0 = resident)", t->grid_workgroups);
    if (t->traversal < 0 || (t->traversal & ~(1023 | TRAV_MIFIF | TRAV_MWHILE | TRAV_GRID | TRAV_GFLAT | TRAV_G3D)) != 0 ||
        (t->traversal & TRAV_REMOVED) != 0 || (t->traversal & TRAV_MIFIF && t->traversal & TRAV_MWHILE) ||
        (t->traversal & TRAV_GFLAT && t->traversal & TRAV_G3D))
        return fail(c, RT_ERR_INVALID,
                    "traversal flags: 0..1023 without 256 (time-binned trees, removed in r04), + 8192 / 16384 (mesh "
                    "if-if / while-while loop, not both), + 65536 (sphere grid), + 131072 / 262144 (its flat / 3-D "
                    "walk, not both); 4096 (mesh LDS tree top, r04) and 32768 (quantised mesh nodes, r05) were "
                    "measured slower and removed");
    if (t->mesh_max_leaf < 1 || t->mesh_max_leaf > MESH_LEAF_MAX)
        return fail(c, RT_ERR_INVALID, "mesh_max_leaf %d (1..%d)", t->mesh_max_leaf, MESH_LEAF_MAX);
    if (t->mesh_lds_nodes < -1 || t->mesh_lds_nodes > MESH_TOP_MAX)
        return fail(c, RT_ERR_INVALID, "mesh_lds_nodes %d (-1 = auto, 0..%d)", t->mesh_lds_nodes, MESH_TOP_MAX);
    if (!(t->mesh_cost_traverse > 0)) return fail(c, RT_ERR_INVALID, "mesh_cost_traverse must be > 0");
    if (t->chunk_waves < 0) return fail(c, RT_ERR_INVALID, "chunk_waves %d (0 = off)", t->chunk_waves);
    // (>= 16 until rt_render_pixels_moments: a 1 MiB pass, 37,449 samples of a job list, lets a test cross a
    // pass boundary with a small list; rt_render's passes hold at least one sample per pixel whatever the cap)
    if (t->sample_buffer_mb < 1) return fail(c, RT_ERR_INVALID, "sample_buffer_mb %d (>= 1)", t->sample_buffer_mb);
    if (t->mesh_block != 0 && t->mesh_block != 256 && t->mesh_block != 512 && t->mesh_block != 768)
        return fail(c, RT_ERR_INVALID, "mesh_block %d (0 = auto, 256, 512 or 768)", t->mesh_block);
    if (t->mesh_lds_stack < -1 || t->mesh_lds_stack > MESH_STACK_MAX)
        return fail(c, RT_ERR_INVALID, "mesh_lds_stack %d (-1 = auto, 0..%d)", t->mesh_lds_stack, MESH_STACK_MAX);
    if (t->item_samples < 1 || t->item_samples > FIX_ITEM_SAMPLES || !(t->item_balance >= 0) ||
        !(t->mesh_item_balance >= 0))
        return fail(c, RT_ERR_INVALID, "item_samples %d (1..%d), item_balance %g, mesh_item_balance %g (>= 0)",
                    t->item_samples, FIX_ITEM_SAMPLES, t->item_balance, t->mesh_item_balance);
    if (t->mesh_builder != RT_MESH_BUILD_HOST && t->mesh_builder != RT_MESH_BUILD_GPU &&
        t->mesh_builder != RT_MESH_BUILD_GPU_LBVH)
        return fail(c, RT_ERR_INVALID, "mesh_builder %d", t->mesh_builder);
    if (!find_render_f32(t->block, t->waves_per_eu, t->traversal & ~(TRAV_MIFIF | TRAV_MWHILE | TRAV_GFLAT | TRAV_G3D),
                         false, false))
        return fail(c, RT_ERR_INVALID, "no fp32 kernel instantiated for block %d, waves_per_eu %d, traversal %d",
                    t->block, t->waves_per_eu, t->traversal);
    const rt_tuning old = c->tuning;
    c->tuning = *t;
    if (c->scene.has_scene && plan_launch(c, true).lds_bytes > 160 * 1024) {
        c->tuning = old;
        return fail(c, RT_ERR_LIMIT, "scene does not fit LDS at this block");
    }
    return RT_OK;
}

int rt_camera_initialize(const rt_camera_desc* d, rt_camera* cam) {
    if (!d || !cam) return RT_ERR_INVALID;
    // camera.h:52-85; vec3 ops as vec3.h (v / t is (1/t) * v; dot and length_squared
    // associate left to right).  Built with -ffp-contract=off.
    struct v3 { double x, y, z; };
    auto add = [](v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; };
    auto sub = [](v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    auto scl = [](double t, v3 v) { return v3{t * v.x, t * v.y, t * v.z}; };
    auto dvs = [&](v3 v, double t) { return scl(1 / t, v); };
    auto cross = [](v3 u, v3 v) {
        return v3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
    };
    auto unit = [&](v3 v) { return dvs(v, std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z)); };
    auto ld = [](const double* p) { return v3{p[0], p[1], p[2]}; };
    auto st = [](double* p, v3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; };
    const double pi = 3.1415926535897932385;                    // rtweekend.h:17
    auto deg2rad = [&](double deg) { return deg * pi / 180.0; };  // rtweekend.h:21-23

    if (d->image_width <= 0 || !(d->aspect_ratio > 0)) return RT_ERR_INVALID;
    int H = static_cast<int>(d->image_width / d->aspect_ratio);
    H = (H < 1) ? 1 : H;
    const v3 center = ld(d->lookfrom);
    const double theta = deg2rad(d->vfov);
    const double h = std::tan(theta / 2);
    const double viewport_height = 2 * h * d->focus_dist;
    const double viewport_width = viewport_height * (static_cast<double>(d->image_width) / H);
    const v3 w = unit(sub(ld(d->lookfrom), ld(d->lookat)));
    const v3 u = unit(cross(ld(d->vup), w));
    const v3 v = cross(w, u);
    const v3 viewport_u = scl(viewport_width, u);
    const v3 viewport_v = scl(viewport_height, v3{-v.x, -v.y, -v.z});
    const v3 du = dvs(viewport_u, (double)d->image_width);
    const v3 dv = dvs(viewport_v, (double)H);
    const v3 upper_left = sub(sub(sub(center, scl(d->focus_dist, w)), dvs(viewport_u, 2)), dvs(viewport_v, 2));
    const v3 p00 = add(upper_left, scl(0.5, add(du, dv)));
    const double defocus_radius = d->focus_dist * std::tan(deg2rad(d->defocus_angle / 2));
    std::memset(cam, 0, sizeof(*cam));
    cam->image_width = d->image_width;
    cam->image_height = H;
    st(cam->center, center);
    st(cam->pixel00_loc, p00);
    st(cam->pixel_delta_u, du);
    st(cam->pixel_delta_v, dv);
    st(cam->defocus_disk_u, scl(defocus_radius, u));
    st(cam->defocus_disk_v, scl(defocus_radius, v));
    cam->defocus_angle = d->defocus_angle;
    return RT_OK;
}

int rt_upload_scene(rt_ctx* c, const rt_sphere* s, int n, const rt_material* m, int nm) {
    return rt_upload_scene_ex(c, s, n, m, nm, nullptr, 0);
}

// The packed scene onto the device, into a scene record `s` of its own (the caller moves it
// into the context once this has succeeded), in the order of the records in PackedScene; the
// mesh tree is uploaded, or built there from the caller's triangles.
static int upload_packed(rt_ctx* c, rt_ctx::Scene& s, PackedScene& pk, int n, const rt_material* m, int nm,
                         const rt_triangle* tri, int ntri) {
    const bool f64 = pk.f64;
    auto upload = [&](DevBuf& dst, const void* src, size_t bytes) -> int {
        HIPCHK(c, dst.reserve(bytes));
        if (bytes) HIPCHK(c, hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice));
        return RT_OK;
    };
    int rc;
    if ((rc = upload(s.d_nodes, pk.bvh.nodes.data(), pk.bvh.nodes.size() * sizeof(Node))) != RT_OK) return rc;
    if ((rc = f64 ? upload(s.d_sph, pk.sd.data(), pk.sd.size() * sizeof(SphereD))
                  : upload(s.d_sph, pk.sf.data(), pk.sf.size() * sizeof(SphereF))) != RT_OK)
        return rc;
    if ((rc = f64 ? upload(s.d_mat, pk.md.data(), pk.md.size() * sizeof(MatD))
                  : upload(s.d_mat, pk.mf.data(), pk.mf.size() * sizeof(MatF))) != RT_OK)
        return rc;
    if (!pk.grid.empty()) {
        if ((rc = upload(s.d_grid, pk.grid.data(), pk.grid.size())) != RT_OK) return rc;
        s.grid_nodes = (int)(pk.grid.size() / sizeof(Node));
        s.grid_hdr = pk.grid_hdr;
        s.grid_density = c->tuning.sphere_grid_density;
        s.grid_entries = pk.grid_entries;
    }
    if ((rc = upload(s.d_big, pk.big.data(), pk.big.size() * sizeof(SphereD))) != RT_OK) return rc;
    if ((rc = upload(s.d_bigf, pk.bigf.data(), pk.bigf.size() * sizeof(BigF))) != RT_OK) return rc;
    if (pk.gpu_build) {
        DevBuf d_in, d_types;
        std::vector<uint32_t> types(nm);
        for (int k = 0; k < nm; ++k) types[k] = (uint32_t)m[k].type;
        if ((rc = upload(d_in, tri, (size_t)ntri * sizeof(rt_triangle))) != RT_OK) return rc;
        if ((rc = upload(d_types, types.data(), types.size() * 4)) != RT_OK) return rc;
        const int cap = ntri > 1 ? ntri - 1 : 1;
        hipError_t e = s.d_mnodes.reserve((size_t)cap * sizeof(Node4));
        if (e == hipSuccess) e = s.d_tris.reserve(f64 ? (size_t)ntri * sizeof(TriD) : (size_t)ntri * sizeof(TriF) + TRIF_SLACK);
        if (e == hipSuccess && !f64) e = s.d_tmeta.reserve((size_t)ntri * sizeof(uint32_t));
        if (e == hipSuccess && !f64)
            e = hipMemsetAsync(s.d_tris.as<char>() + (size_t)ntri * sizeof(TriF), 0, TRIF_SLACK, c->stream);
        LbvhInput in{};
        in.tris = d_in.as<rt_triangle>();
        in.n = ntri;
        in.mat_type = d_types.as<uint32_t>();
        for (int a = 0; a < 3; ++a) {
            in.lo[a] = pk.clo[a];
            in.inv[a] = pk.chi[a] > pk.clo[a] ? 1.0 / (pk.chi[a] - pk.clo[a]) : 0.0;
        }
        in.max_leaf = std::max(1, std::min(c->tuning.mesh_max_leaf, MESH_LEAF_MAX));
        in.f64 = f64;
        // two rounds of treelet restructuring: the 4-wide SAH cost of the C4 blob's tree 28.56
        // -> 25.77 -> 25.41 (3: 25.32) against the host SAH tree's 24.7 (tests/cpp/treelet_check.cpp)
        in.treelet_rounds = c->tuning.mesh_builder == RT_MESH_BUILD_GPU ? 2 : 0;
        LbvhOutput out{s.d_mnodes.as<Node4>(), cap, s.d_tris.p, s.d_tmeta.as<uint32_t>()};
        if (e == hipSuccess) e = lbvh_build(in, c->lbvh, out, c->stream);
        if (e != hipSuccess) return fail(c, RT_ERR_HIP, "GPU mesh BVH build: %s", hipGetErrorString(e));
        if (3 * out.depth4 + 1 > MESH_STACK_MAX)
            return fail(c, RT_ERR_LIMIT, "GPU mesh BVH depth %d exceeds the traversal stack (use the host builder)",
                        out.depth4);
        s.n_mnodes = out.node_count;
        s.n_tris = ntri;
        s.mdepth = out.depth4;
        s.mleaves = out.leaves;
    } else if (ntri > 0) {
        const MeshBvh& mbvh = pk.mbvh;
        if ((rc = upload(s.d_mnodes, mbvh.nodes4.data(), mbvh.nodes4.size() * sizeof(Node4))) != RT_OK)
            return rc;
        if (f64) {
            if ((rc = upload(s.d_tris, pk.td.data(), pk.td.size() * sizeof(TriD))) != RT_OK) return rc;
        } else {
            if ((rc = upload(s.d_tris, pk.tf.data(), pk.tf.size() * sizeof(TriF))) != RT_OK) return rc;
            if ((rc = upload(s.d_tmeta, pk.tmeta.data(), pk.tmeta.size() * sizeof(uint32_t))) != RT_OK) return rc;
        }
        s.n_mnodes = (int)mbvh.nodes4.size();
        s.n_tris = ntri;
        s.mdepth = mbvh.depth4;
        s.mleaves = mbvh.leaves;
    }
    if (s.n_mnodes > 0) {
        // the mesh's box: the union of the root's child boxes, as the kernels test them
        // (read back from the device, so either builder's tree gives it)
        Node4 root;
        const hipError_t e = hipMemcpy(&root, s.d_mnodes.p, sizeof(Node4), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(c, RT_ERR_HIP, "mesh root read-back: %s", hipGetErrorString(e));
        const float inf = std::numeric_limits<float>::infinity();
        float b[6] = {inf, inf, inf, -inf, -inf, -inf};
        for (int k = 0; k < 4; ++k) {
            if (root.ref[k] == MREF_EMPTY) continue;
            b[0] = std::min(b[0], root.lox[k]), b[1] = std::min(b[1], root.loy[k]), b[2] = std::min(b[2], root.loz[k]);
            b[3] = std::max(b[3], root.hix[k]), b[4] = std::max(b[4], root.hiy[k]), b[5] = std::max(b[5], root.hiz[k]);
        }
        std::copy(b, b + 6, s.mbox);
    }
    if (pk.gpu_build) {
        // rt_trace_rays' id map, the triangle part: the device builder's leaf order
        std::vector<uint32_t> perm((size_t)ntri);
        HIPCHK(c, hipMemcpy(perm.data(), lbvh_sorted_index(c->lbvh, ntri), (size_t)ntri * 4, hipMemcpyDeviceToHost));
        for (uint32_t k : perm) pk.remap.push_back(n + (int)k);
        invert_remap(pk.remap, (int)pk.bvh.order.size(), (int)pk.big.size(), n + ntri, pk.unmap);
    }
    if ((rc = upload(s.d_remap, pk.remap.data(), pk.remap.size() * sizeof(int))) != RT_OK) return rc;
    if ((rc = upload(s.d_unmap, pk.unmap.data(), pk.unmap.size() * sizeof(int))) != RT_OK) return rc;
    s.n_unmap = (int)pk.unmap.size();
    s.box_extent = pk.box_extent;
    s.reach = pk.reach;
    s.n_nodes = (int)pk.bvh.nodes.size();
    s.n_sph = (int)pk.bvh.order.size();
    s.n_front = pk.bvh.front;
    s.n_mat = nm;
    s.n_big = (int)pk.big.size();
    s.depth = pk.bvh.depth;
    s.leaves = pk.bvh.leaves;
    s.n_input = n;
    return RT_OK;
}

int rt_upload_scene_ex(rt_ctx* c, const rt_sphere* s, int n, const rt_material* m, int nm, const rt_triangle* tri,
                       int ntri) {
    if (!c) return RT_ERR_INVALID;
    PackedScene pk;
    std::string err;
    int rc = pack_scene(s, n, m, nm, tri, ntri, c->tuning, c->precision == RT_PREC_F64, pk, err);
    if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());
    HIPCHK(c, hipSetDevice(c->device));
    // from here on the old scene is gone (its memory is free for the new one's); the new one
    // is the context's only once it is whole, and only where a launch of it fits LDS (the plan
    // reads the context, so that one check follows the move and takes the scene back out)
    free_scene(c);
    rt_ctx::Scene up;
    if ((rc = upload_packed(c, up, pk, n, m, nm, tri, ntri)) != RT_OK) return rc;
    c->scene = std::move(up);
    const size_t lds = plan_launch(c, true).lds_bytes;
    if (lds > 160 * 1024) {
        free_scene(c);
        return fail(c, RT_ERR_LIMIT, "scene needs %zu B of LDS per workgroup (> 160 KiB)", lds);
    }
    c->scene.has_scene = true;
    return RT_OK;
}

int rt_scene_info_get(rt_ctx* c, rt_scene_info* info) {
    if (!c || !info) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "no scene");
    info->num_spheres = c->scene.n_input;
    info->num_materials = c->scene.n_mat;
    info->bvh_nodes = c->scene.n_nodes;
    info->bvh_depth = c->scene.depth;
    info->bvh_leaves = c->scene.leaves;
    info->big_spheres = c->scene.n_big;
    // (the plan of a launch whose rays all start within the sphere grid's reach: rt_grid_reach)
    const LaunchPlan plan = plan_launch(c, true);
    info->lds_bytes = (int)plan.lds_bytes;
    info->render_block = plan.block;
    info->render_traversal = plan.trav;
    info->render_waves_per_eu = plan.wpe;
    info->render_mesh_lds_stack = plan.mesh_stack;
    for (int a = 0; a < 3; ++a) info->grid_res[a] = c->scene.grid_nodes > 0 ? c->scene.grid_hdr.res[a] : 0;
    info->grid_entries = c->scene.grid_entries;
    info->grid_time_slabs = c->scene.grid_nodes > 0 ? c->scene.grid_hdr.n_slab : 0;
    info->grid_far_o = c->scene.grid_nodes > 0 ? c->scene.grid_hdr.far_o : 0.f;
    info->grid_density = c->scene.grid_nodes > 0 ? c->scene.grid_density : 0.0;
    info->precision = c->precision;
    info->num_triangles = c->scene.n_tris;
    info->mesh_nodes = c->scene.n_mnodes;
    info->mesh_depth = c->scene.mdepth;
    info->mesh_leaves = c->scene.mleaves;
    return RT_OK;
}

int rt_grid_reach(rt_ctx* c, const rt_camera* cam, int32_t* walks) {
    if (!c || !walks) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_grid_reach before rt_upload_scene");
    int rc = check_camera(c, cam);
    if (rc) return rc;
    *walks = grid_in_reach(c, cam) ? 1 : 0;
    return RT_OK;
}

int rt_pixels_plan(rt_ctx* c, const rt_camera* cam, rt_pixels_plan_info* info) {
    return rt_pixels_plan_call(c, cam, RT_QUERY_PIXELS, info);
}

int rt_pixels_plan_call(rt_ctx* c, const rt_camera* cam, int call, rt_pixels_plan_info* info) {
    if (!c || !info) return RT_ERR_INVALID;
    if (!cam) return fail(c, RT_ERR_INVALID, "camera is NULL");
    if (call != RT_QUERY_PIXELS && call != RT_QUERY_MOMENTS && call != RT_QUERY_AOV)
        return fail(c, RT_ERR_INVALID, "rt_pixels_plan_call: call %d (RT_QUERY_PIXELS, _MOMENTS or _AOV)", call);
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_pixels_plan before rt_upload_scene");
    int rc = check_camera(c, cam);
    if (rc) return rc;
    const QueryPlan q = plan_job_query(c, call, grid_in_reach(c, cam));
    if (q.lds_bytes > 160 * 1024)
        return fail(c, RT_ERR_LIMIT, "rt_pixels_plan: a query needs %zu B of LDS per workgroup", q.lds_bytes);
    info->walks_grid = q.grid ? 1 : 0;
    info->traversal = q.trav;
    info->block = q.block;
    info->lds_bytes = (int32_t)q.lds_bytes;
    return RT_OK;
}

int rt_shard_layout(int width, int height, int shard, int num_shards, rt_shard_info* info) {
    if (!info || width <= 0 || height <= 0 || num_shards <= 0 || shard < 0 || shard >= num_shards)
        return RT_ERR_INVALID;
    info->tile_w = 8;
    info->tile_h = 8;
    info->tiles_x = (width + 7) / 8;
    info->tiles_y = (height + 7) / 8;
    info->num_tiles = info->tiles_x * info->tiles_y;
    info->shard = shard;
    info->num_shards = num_shards;
    info->shard_tiles = (info->num_tiles - shard + num_shards - 1) / num_shards;
    info->max_shard_tiles = (info->num_tiles + num_shards - 1) / num_shards;
    return RT_OK;
}

// Largest work item (samples) of a persistent launch.  Coherent kernels: a work item
// belongs to one wave, so on small shards (many lanes per pixel) big items leave too few
// items per wave to even out; cap the item at the power of two <= 12 pixels per lane, but
// not below the power of two <= min(8, 24 pixels per lane) (C3 shards of 1 / 2 / 4 / 8
// GPUs: 32 / 16 / 8 / 8 -- measured 50.5 / 25.8 / 13.4 / 7.14 ms against 50.5 / 26.3 /
// 13.6 / 7.17 with the earlier 24-pixel cap (32 / 32 / 16 / 8),
// profiles/r02/item_cap_scaling_r02bn.log; 4 at 8 GPUs lost, item_size_sweep_r02ai.log)
static int item_cap(const rt_ctx* c, int trav, double lanes, double pixels) {
    int cmax = std::min(c->tuning.item_samples, FIX_ITEM_SAMPLES);
    if ((trav & TRAV_COH) && c->scene.n_mnodes == 0) {
        const double ppl = pixels / std::max(1.0, lanes);
        int cap = 1, floor_cap = 1;
        while (cap * 2 <= 12.0 * ppl && cap < FIX_ITEM_SAMPLES) cap *= 2;
        while (floor_cap * 2 <= 24.0 * ppl && floor_cap < 8) floor_cap *= 2;
        cmax = std::min(cmax, std::max(cap, floor_cap));
    }
    return cmax;
}

// Work-queue item phases of a persistent launch of spp samples, largest chunks first: a
// chunk of c samples is handed out only while the samples left after it keep every
// resident lane busy for `balance` chunks of that size, i.e. while
// left - c >= balance * c * lanes / pixels; single samples take the rest.
static void plan_phases(RenderParams& P, int spp, double lanes, double pixels, double balance, int cmax) {
    int left = spp, s0 = 0;
    P.nph = 0;
    for (int ch = 1 << 5; ch >= 1; ch >>= 1) {
        if (ch > cmax || left <= 0) continue;
        int k = left;   // single samples: the rest
        if (ch > 1) {
            const double keep = balance * ch * lanes / std::max(1.0, pixels);
            k = left - ch >= keep ? (int)((left - keep) / ch) : 0;
        }
        if (k <= 0) continue;
        P.ph_s0[P.nph] = s0;
        P.ph_c[P.nph] = ch;
        P.ph_k[P.nph] = k;
        ++P.nph;
        s0 += k * ch;
        left -= k * ch;
    }
}

// Item balance of an fp32 launch: the tuning's, doubled for a mesh scene whose shard has
// fewer pixels than the launch has resident lanes, so its single samples start earlier.
// On C4 at 8 GPUs that cuts the shard 6.25 -> 6.06 ms (predicted 5.94x -> 6.12x), and the
// 1-GPU frame (2.07 M pixels for 0.39 M lanes) is unchanged (profiles/r04/r04n/sc4c_ib*.log:
// mesh_item_balance 20 / 40 / 80 / 160 gave N = 8 shards of 6.25 / 6.06 / 6.12 / 6.10 ms and
// N = 1 frames of 37.14 / 37.22 / 37.67 / 37.99 ms).  Sphere scenes were not measured this
// way and keep item_balance.
static double item_balance_of(const rt_ctx* c, double lanes, double pixels) {
    if (c->scene.n_mnodes == 0) return c->tuning.item_balance;
    return c->tuning.mesh_item_balance * (lanes > pixels ? 2.0 : 1.0);
}

// One fp32 launch of P.spp <= FIX_LAUNCH_SAMPLES samples from P.sample_begin: lanes add their
// chunk's fixed-point sums into the context's accumulator for this buffer (integer atomics:
// order-free), finalize_kernel writes out_sums.  e: the first launch error.
static int render_range_f32(rt_ctx* c, const LaunchPlan& plan, const RenderKernel& k, RenderParams P, size_t npx,
                            hipStream_t st, hipError_t& e) {
    float* out_sums = (float*)P.out_sums;
    int rc;
    rt_ctx::Accum* slot = nullptr;
    for (auto& a : c->accum)
        if (a.out == out_sums && a.W == P.W && a.H == P.H && a.shard == P.shard && a.nshards == P.nshards) slot = &a;
    const bool have = slot != nullptr;
    if (!slot) {
        slot = &c->accum[0];
        for (auto& a : c->accum)
            if (a.used < slot->used) slot = &a;
    }
    if ((rc = reserve(c, slot->acc, npx * 3 * sizeof(long long)))) return rc;
    if ((rc = reserve(c, slot->accp, npx * 2 * sizeof(unsigned long long)))) return rc;
    if ((rc = reserve(c, slot->flags, npx * sizeof(uint32_t)))) return rc;
    slot->out = out_sums;
    slot->W = P.W;
    slot->H = P.H;
    slot->shard = P.shard;
    slot->nshards = P.nshards;
    slot->used = ++c->accum_clock;
    long long* acc = slot->acc.as<long long>();
    unsigned long long* accp = slot->accp.as<unsigned long long>();
    uint32_t* flags = slot->flags.as<uint32_t>();
    P.accum = acc;
    P.accum_flags = flags;
    P.accp = accp;
    P.diag = c->diag_buf;
    P.gsus_lanes = c->gsus_lanes;
    P.gsus_iters = c->gsus_iters;
    P.batch_cap = c->batch_cap;
    P.batch_adopt = c->batch_adopt;
    HIPCHK(c, slot->queue.reserve(QUEUE_CTRL_BYTES));
    P.queue = slot->queue.as<uint32_t>();
    {
        const double lanes = (double)P.max_wgs * plan.block, pixels = (double)npx;
        plan_phases(P, P.spp, lanes, pixels, item_balance_of(c, lanes, pixels), item_cap(c, plan.trav, lanes, pixels));
    }
    HIPCHK(c, hipMemsetAsync(P.queue, 0, QUEUE_CTRL_BYTES, st));
    HIPCHK(c, hipMemsetAsync(accp, 0, npx * 2 * sizeof(unsigned long long), st));
    if (!P.accumulate) {
        e = hipMemsetAsync(acc, 0, npx * 3 * sizeof(long long), st);
        if (e == hipSuccess) e = hipMemsetAsync(flags, 0, npx * sizeof(uint32_t), st);
        if (e == hipSuccess && P.out_segs) e = hipMemsetAsync(P.out_segs, 0, npx * sizeof(uint32_t), st);
    } else if (!have) {
        // no fixed-point state for this buffer: continue from its float values
        e = launch_seed_accum(out_sums, acc, flags, npx, st);
    } else {
        // state for this address: kept where out_sums still holds what it last
        // finalized to, restarted from the floats elsewhere (a reallocated buffer)
        e = launch_reconcile_accum(out_sums, acc, flags, npx, st);
    }
    if (e == hipSuccess && P.spp > 0) e = launch_render(k, P, plan.lds_bytes, st);
    if (e == hipSuccess) e = launch_finalize(acc, accp, flags, out_sums, npx, st);
    return RT_OK;
}

// fp64 on persistent lanes (TRAV_PERSIST): every sample's radiance goes to d_samples, then
// the ordered reduction; passes bound the buffer to sample_buffer_mb (a shard with no tiles
// has nothing to store: npx = 0)
static int render_range_f64(rt_ctx* c, const LaunchPlan& plan, const RenderKernel& k, const RenderParams& P,
                            size_t npx, hipStream_t st, hipError_t& e) {
    const int spp = P.spp;
    const size_t eb = elem_bytes(c);
    int rc;
    // The coherent kernel's FIFO entries carry a sample's index within the pass in 16
    // bits (CohEntryD::sid, the hit id above it): a pass holds at most 65535 samples.
    constexpr size_t MAX_PASS_SAMPLES = 0xffff;
    const size_t fit = std::min(MAX_PASS_SAMPLES, npx > 0 ? ((size_t)c->tuning.sample_buffer_mb << 20) /
                                                                (npx * 3 * eb) : (size_t)spp);
    const int pass_spp = std::max(1, (size_t)spp < fit ? spp : (int)std::max<size_t>(1, fit));
    if ((rc = reserve(c, c->d_samples, npx * 3 * eb * (size_t)std::max(1, pass_spp)))) return rc;
    HIPCHK(c, c->d_queue64.reserve(QUEUE_CTRL_BYTES));
    const double balance = c->scene.n_mnodes > 0 ? c->tuning.mesh_item_balance : c->tuning.item_balance;
    if (P.out_segs && !P.accumulate) e = hipMemsetAsync(P.out_segs, 0, npx * sizeof(uint32_t), st);
    if (e == hipSuccess && spp == 0 && !P.accumulate) e = hipMemsetAsync(P.out_sums, 0, npx * 3 * eb, st);
    for (int done = 0; done < spp && npx > 0 && e == hipSuccess; done += pass_spp) {
        RenderParams Q = P;
        Q.queue = c->d_queue64.as<uint32_t>();
        Q.sample_begin = P.sample_begin + done;
        Q.spp = spp - done < pass_spp ? spp - done : pass_spp;
        Q.samples = c->d_samples.p;
        const double lanes = (double)Q.max_wgs * plan.block;
        plan_phases(Q, Q.spp, lanes, (double)npx, balance, item_cap(c, plan.trav, lanes, (double)npx));
        e = hipMemsetAsync(Q.queue, 0, QUEUE_CTRL_BYTES, st);
        if (e == hipSuccess) e = launch_render(k, Q, plan.lds_bytes, st);
        if (e == hipSuccess)
            e = launch_reduce(c->d_samples.p, P.out_sums, (int)eb, npx * 3, Q.spp, (P.accumulate || done > 0) ? 1 : 0, st);
    }
    return RT_OK;
}

int rt_render_range(rt_ctx* c, const rt_camera* cam, int sample_begin, int spp, int max_depth, int shard,
                    int num_shards, int accumulate, void* out_sums, uint32_t* out_segments, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_render before rt_upload_scene");
    int rc = check_camera(c, cam);
    if (rc) return rc;
    if (spp < 0 || sample_begin < 0) return fail(c, RT_ERR_INVALID, "samples [%d, +%d)", sample_begin, spp);
    if (c->precision == RT_PREC_F64 && max_depth > 64)
        return fail(c, RT_ERR_LIMIT, "fp64 path keeps at most 64 bounces (max_depth %d)", max_depth);
    if (!out_sums) return fail(c, RT_ERR_INVALID, "out_sums is NULL");
    rt_shard_info si;
    if (rt_shard_layout(cam->image_width, cam->image_height, shard, num_shards, &si) != RT_OK)
        return fail(c, RT_ERR_INVALID, "bad shard %d of %d", shard, num_shards);
    HIPCHK(c, hipSetDevice(c->device));
    const bool f32 = c->precision == RT_PREC_F32, mesh = c->scene.n_mnodes > 0;
    const LaunchPlan plan = plan_launch(c, grid_in_reach(c, cam));
    if (plan.lds_bytes > 160 * 1024)
        return fail(c, RT_ERR_LIMIT, "render needs %zu B of LDS per workgroup", plan.lds_bytes);
    // the kernel that runs: the plan's, or with rt_render_diag's buffer set its instrumented copy
    const RenderKernel* k =
        f32 && c->diag_buf ? find_render_f32(plan.block, plan.wpe, plan.trav, mesh, true) : plan.kernel;
    if (f32 && mesh && !plan.kernel)
        return fail(c, RT_ERR_INVALID, "no mesh kernel instantiated for block %d, mesh_waves_per_eu %d, traversal %d",
                    plan.block, plan.wpe, plan.trav);
    if (f32 && !mesh && !plan.kernel)
        return fail(c, RT_ERR_INVALID,
                    "no fp32 kernel instantiated for block %d, waves_per_eu %d, traversal %d (tuning traversal %d; "
                    "128 = no LDS sums is added where they would cost occupancy)",
                    plan.block, c->tuning.waves_per_eu, plan.trav, c->tuning.traversal);
    if (f32 && c->diag_buf && !k)
        return fail(c, RT_ERR_INVALID, "no instrumented build of block %d, waves_per_eu %d, traversal %d (rt_render_diag)",
                    plan.block, plan.wpe, plan.trav);
    if (!k) return fail(c, RT_ERR_INVALID, "no fp64 kernel instantiated for f64_kernel %d", plan.f64_kernel);
    if (plan.trav & TRAV_GRID) {
        // the grid walk reads cells and records by LDS byte address, counting from 0: the
        // kernel's dynamic LDS must start there, i.e. the kernel has no static LDS (rt_device.h)
        // (the instrumented copy is another kernel, with its own)
        const int s = render_kernel_attrs(k).static_lds;
        if (s != 0) return fail(c, RT_ERR_HIP, "grid render kernel with %d B of static LDS (needs none)", s);
    }
    RenderParams P;
    fill_params(c, cam, spp, max_depth, plan.mesh_stack, P);
    P.shard = shard;
    P.nshards = num_shards;
    P.shard_tiles = si.shard_tiles;
    P.out_sums = out_sums;
    P.out_segs = out_segments;
    P.coh_refill = c->tuning.coh_refill;
    // persistent lanes: no more workgroups than the device keeps resident
    P.max_wgs = std::max(1, plan.wgs_per_cu * (c->n_cu > 0 ? c->n_cu : 256));
    if (c->tuning.grid_workgroups > 0) P.max_wgs = c->tuning.grid_workgroups;
    apply_grid(c, plan.trav, P);
    hipStream_t st = stream_of(c, stream);
    const size_t npx = (size_t)si.shard_tiles * 64;
    HIPCHK(c, hipEventRecord(c->ev0, st));
    // fp32: packed per-launch sums hold <= FIX_LAUNCH_SAMPLES samples: consecutive ranges,
    // timed as one (rt_last_kernel_ms spans all of them)
    const int range = f32 ? FIX_LAUNCH_SAMPLES : std::max(1, spp);
    int done = 0;
    hipError_t e = hipSuccess;
    do {
        P.sample_begin = sample_begin + done;
        P.spp = std::min(spp - done, range);
        P.accumulate = accumulate || done > 0 ? 1 : 0;
        if ((rc = f32 ? render_range_f32(c, plan, *k, P, npx, st, e) : render_range_f64(c, plan, *k, P, npx, st, e)))
            return rc;
        done += range;
    } while (done < spp && e == hipSuccess);
    return timed_end(c, st, e, "render launch");
}

int rt_render(rt_ctx* c, const rt_camera* cam, int spp, int max_depth, int shard, int num_shards, void* out_sums,
              uint32_t* out_segments, void* stream) {
    return rt_render_range(c, cam, 0, spp, max_depth, shard, num_shards, 0, out_sums, out_segments, stream);
}

int rt_last_kernel_ms(rt_ctx* c, float* ms) {
    if (!c || !ms) return RT_ERR_INVALID;
    if (!c->timed) return fail(c, RT_ERR_INVALID, "no kernel launched yet");
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return RT_OK;
}

int rt_unshard(rt_ctx* c, const void* gathered, int width, int height, int num_shards, void* frame, void* stream) {
    if (!c || !gathered || !frame || width <= 0 || height <= 0 || num_shards <= 0) return RT_ERR_INVALID;
    rt_shard_info si;
    rt_shard_layout(width, height, 0, num_shards, &si);
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_unshard(gathered, frame, (int)elem_bytes(c), 3, width, height, si.tiles_x, num_shards,
                             si.max_shard_tiles, st));
    return RT_OK;
}

int rt_quantize(rt_ctx* c, const void* frame, int width, int height, int spp, int32_t* rgb, void* stream) {
    if (!c || !frame || !rgb || width <= 0 || height <= 0) return RT_ERR_INVALID;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_quantize(frame, (int)elem_bytes(c), rgb, (size_t)width * height * 3, spp, st));
    return RT_OK;
}

int rt_render_frame(rt_ctx* c, const rt_camera* cam, int spp, int max_depth, void* sums_host, int32_t* rgb_host,
                    uint32_t* segments_host) {
    if (!c) return RT_ERR_INVALID;
    int rc = check_camera(c, cam);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int W = cam->image_width, H = cam->image_height;
    rt_shard_info si;
    rt_shard_layout(W, H, 0, 1, &si);
    const size_t npx_tiles = (size_t)si.num_tiles * 64, npx = (size_t)W * H, eb = elem_bytes(c);
    if ((rc = reserve(c, c->d_shard, npx_tiles * 3 * eb))) return rc;
    if ((rc = reserve(c, c->d_frame, npx * 3 * eb))) return rc;
    if ((rc = reserve(c, c->d_segs, npx_tiles * 4))) return rc;
    if ((rc = reserve(c, c->d_segs_frame, npx * 4))) return rc;
    if ((rc = reserve(c, c->d_rgb, npx * 3 * 4))) return rc;
    if ((rc = rt_render(c, cam, spp, max_depth, 0, 1, c->d_shard.p, c->d_segs.as<uint32_t>(), nullptr))) return rc;
    HIPCHK(c, launch_unshard(c->d_shard.p, c->d_frame.p, (int)eb, 3, W, H, si.tiles_x, 1, si.max_shard_tiles, c->stream));
    if (segments_host)
        HIPCHK(c, launch_unshard(c->d_segs.p, c->d_segs_frame.p, 4, 1, W, H, si.tiles_x, 1, si.max_shard_tiles,
                                 c->stream));
    if (rgb_host) HIPCHK(c, launch_quantize(c->d_frame.p, (int)eb, c->d_rgb.as<int32_t>(), npx * 3, spp, c->stream));
    if (sums_host)
        HIPCHK(c, hipMemcpyAsync(sums_host, c->d_frame.p, npx * 3 * eb, hipMemcpyDeviceToHost, c->stream));
    if (rgb_host) HIPCHK(c, hipMemcpyAsync(rgb_host, c->d_rgb.p, npx * 3 * 4, hipMemcpyDeviceToHost, c->stream));
    if (segments_host)
        HIPCHK(c, hipMemcpyAsync(segments_host, c->d_segs_frame.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_finish_frame_u8(rt_ctx* c, const void* gathered, int width, int height, int num_shards, int spp,
                       uint8_t* rgb8, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (!gathered || !rgb8 || width <= 0 || height <= 0 || num_shards <= 0 || spp <= 0)
        return fail(c, RT_ERR_INVALID, "finish %dx%d over %d shards at %d spp", width, height, num_shards, spp);
    rt_shard_info si;
    rt_shard_layout(width, height, 0, num_shards, &si);
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_finish_u8(gathered, (int)elem_bytes(c), rgb8, width, height, si.tiles_x, num_shards,
                               si.max_shard_tiles, spp, st));
    return RT_OK;
}

void* rt_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void rt_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int rt_render_frame_u8(rt_ctx* c, const rt_camera* cam, int spp, int max_depth, uint8_t* rgb8_host) {
    if (!c) return RT_ERR_INVALID;
    int rc = check_camera(c, cam);
    if (rc) return rc;
    if (!rgb8_host || spp <= 0) return fail(c, RT_ERR_INVALID, "rgb8_host %p, spp %d", (void*)rgb8_host, spp);
    HIPCHK(c, hipSetDevice(c->device));
    const int W = cam->image_width, H = cam->image_height;
    rt_shard_info si;
    rt_shard_layout(W, H, 0, 1, &si);
    const size_t bytes = (size_t)W * H * 3;
    if ((rc = reserve(c, c->d_shard, (size_t)si.num_tiles * 64 * 3 * elem_bytes(c)))) return rc;
    if ((rc = reserve(c, c->d_rgb8, bytes))) return rc;
    // copy straight into page-locked caller memory, else through the context's staging buffer
    hipPointerAttribute_t attr;
    bool pinned = hipPointerGetAttributes(&attr, rgb8_host) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    if (!pinned && c->pinned_cap < bytes) {
        if (c->h_pinned) HIPCHK(c, hipHostFree(c->h_pinned));
        c->h_pinned = nullptr;
        c->pinned_cap = 0;
        HIPCHK(c, hipHostMalloc(&c->h_pinned, bytes, hipHostMallocDefault));
        c->pinned_cap = bytes;
    }
    if ((rc = rt_render(c, cam, spp, max_depth, 0, 1, c->d_shard.p, nullptr, nullptr))) return rc;
    HIPCHK(c, launch_finish_u8(c->d_shard.p, (int)elem_bytes(c), c->d_rgb8.as<uint8_t>(), W, H, si.tiles_x, 1,
                               si.max_shard_tiles, spp, c->stream));
    HIPCHK(c, hipMemcpyAsync(pinned ? (void*)rgb8_host : c->h_pinned, c->d_rgb8.p, bytes, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!pinned) std::memcpy(rgb8_host, c->h_pinned, bytes);
    return RT_OK;
}

int rt_render_frame_multi(rt_ctx** cs, int n, const rt_camera* cam, int spp, int max_depth, void* sums_host,
                          int32_t* rgb_host) {
    if (!cs || n <= 0) return RT_ERR_INVALID;
    for (int r = 0; r < n; ++r) {
        if (!cs[r]) return RT_ERR_INVALID;
        if (cs[r]->precision != cs[0]->precision)
            return fail(cs[0], RT_ERR_INVALID, "contexts %d and 0 differ in precision", r);
        for (int q = 0; q < r; ++q)
            if (cs[q] == cs[r]) return fail(cs[0], RT_ERR_INVALID, "context %d is listed twice", r);
    }
    if (n == 1) return rt_render_frame(cs[0], cam, spp, max_depth, sums_host, rgb_host, nullptr);
    rt_ctx* c0 = cs[0];
    int rc = check_camera(c0, cam);
    if (rc) return rc;
    const int W = cam->image_width, H = cam->image_height;
    rt_shard_info si;
    rt_shard_layout(W, H, 0, n, &si);
    const size_t eb = elem_bytes(c0), per = (size_t)si.max_shard_tiles * 64 * 3 * eb, npx = (size_t)W * H;
    // each context renders its shard into its own device buffer, on its own stream
    for (int r = 0; r < n; ++r) {
        rt_ctx* c = cs[r];
        HIPCHK(c0, hipSetDevice(c->device));
        if ((rc = reserve(c, c->d_shard, per))) return rc;
        if ((rc = rt_render(c, cam, spp, max_depth, r, n, c->d_shard.p, nullptr, nullptr)) != RT_OK) {
            if (c != c0) c0->err = std::string("context ") + std::to_string(r) + ": " + c->err;
            return rc;
        }
    }
    // gather to ctxs[0]'s device: it waits for each shard's render, then copies it
    HIPCHK(c0, hipSetDevice(c0->device));
    for (int r = 1; r < n; ++r) {
        int can = 0;
        if (cs[r]->device != c0->device && hipDeviceCanAccessPeer(&can, c0->device, cs[r]->device) == hipSuccess &&
            can) {
            const hipError_t e = hipDeviceEnablePeerAccess(cs[r]->device, 0);   // direct xGMI copies
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                return fail(c0, RT_ERR_HIP, "peer access %d -> %d: %s", c0->device, cs[r]->device,
                            hipGetErrorString(e));
            (void)hipGetLastError();
        }
    }
    if ((rc = reserve(c0, c0->d_gather, per * (size_t)n))) return rc;
    if ((rc = reserve(c0, c0->d_frame, npx * 3 * eb))) return rc;
    if ((rc = reserve(c0, c0->d_rgb, npx * 3 * 4))) return rc;
    if (c0->comm) {
        // RCCL: one grouped ncclGather, rank r on context r's stream after its render
        if ((rc = rt_comm_gather_group(cs, n, per / eb, c0->d_gather.p))) return rc;
    } else {
        for (int r = 0; r < n; ++r) {
            rt_ctx* c = cs[r];
            HIPCHK(c0, hipStreamWaitEvent(c0->stream, c->ev1, 0));   // ev1: end of that context's render
            void* dst = (char*)c0->d_gather.p + (size_t)r * per;
            if (c->device == c0->device)
                HIPCHK(c0, hipMemcpyAsync(dst, c->d_shard.p, per, hipMemcpyDeviceToDevice, c0->stream));
            else
                HIPCHK(c0, hipMemcpyPeerAsync(dst, c0->device, c->d_shard.p, c->device, per, c0->stream));
        }
    }
    HIPCHK(c0, launch_unshard(c0->d_gather.p, c0->d_frame.p, (int)eb, 3, W, H, si.tiles_x, n, si.max_shard_tiles,
                              c0->stream));
    if (rgb_host) HIPCHK(c0, launch_quantize(c0->d_frame.p, (int)eb, c0->d_rgb.as<int32_t>(), npx * 3, spp, c0->stream));
    if (sums_host) HIPCHK(c0, hipMemcpyAsync(sums_host, c0->d_frame.p, npx * 3 * eb, hipMemcpyDeviceToHost, c0->stream));
    if (rgb_host) HIPCHK(c0, hipMemcpyAsync(rgb_host, c0->d_rgb.p, npx * 3 * 4, hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(c0, hipStreamSynchronize(c0->stream));
    return RT_OK;
}

// The query launches: the scene in LDS at TRACE_BLOCK threads, and its size there with the mesh
// stack's LDS columns.  The per-ray queries (rt_trace_rays*, rt_occluded, rt_radiance_rays) take
// the caller's rays and walk the tree.  view: the camera of a query that makes its own rays (the
// job-list queries; call: which, RT_QUERY_*), which walks what plan_job_query says for it -- *grid
// receives that plan's flags (0: the tree), and P, lds and the kernel the caller launches all
// follow that one value.
static int query_setup(rt_ctx* c, const char* what, RenderParams& P, size_t& lds, const rt_camera* view = nullptr,
                       int call = -1, int* grid = nullptr) {
    HIPCHK(c, hipSetDevice(c->device));
    rt_camera cam{};
    cam.image_width = cam.image_height = 1;
    const QueryPlan q = plan_job_query(c, call, view && grid && grid_in_reach(c, view));
    fill_params(c, view ? view : &cam, 1, 1, q.mesh_stack, P);
    P.nodes = c->scene.d_nodes.as<Node>();   // (the time-binned copies are a render-kernel option)
    apply_grid(c, q.grid, P);
    lds = q.lds_bytes;
    if (grid) *grid = q.grid;
    if (lds > 160 * 1024) return fail(c, RT_ERR_LIMIT, "%s needs %zu B of LDS per workgroup", what, lds);
    return RT_OK;
}

static int trace_rays(rt_ctx* c, const void* rays, int n, const int32_t* origin_ids, rt_hit* hits, void* stream,
                      unsigned long long* diag) {
    if (!c) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_trace_rays before rt_upload_scene");
    if (n < 0 || (n > 0 && (!rays || !hits))) return fail(c, RT_ERR_INVALID, "rt_trace_rays: %d rays, rays %p, hits %p", n, rays, hits);
    RenderParams P;
    size_t lds;
    if (int rc = query_setup(c, "rt_trace_rays", P, lds)) return rc;
    P.diag = diag;
    const int *remap = c->scene.d_remap.as<int>(), *unmap = c->scene.d_unmap.as<int>();
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    const hipError_t e =
        c->precision == RT_PREC_F64
            ? launch_trace_f64(P, lds, st, rays, n, hits, remap, origin_ids, unmap, c->scene.n_unmap)
            : launch_trace_f32(P, lds, st, rays, n, hits, remap, origin_ids, unmap, c->scene.n_unmap, diag != nullptr);
    return timed_end(c, st, e, "trace launch");
}

int rt_trace_rays(rt_ctx* c, const void* rays, int n, rt_hit* hits, void* stream) {
    return trace_rays(c, rays, n, nullptr, hits, stream, nullptr);
}

int rt_trace_rays_from(rt_ctx* c, const void* rays, int n, const int32_t* origin_ids, rt_hit* hits, void* stream) {
    return trace_rays(c, rays, n, origin_ids, hits, stream, nullptr);
}

int rt_occluded(rt_ctx* c, const void* rays, int n, const void* intervals, uint8_t* occluded, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_occluded before rt_upload_scene");
    if (n < 0 || (n > 0 && (!rays || !occluded)))
        return fail(c, RT_ERR_INVALID, "rt_occluded: %d rays, rays %p, occluded %p", n, rays, (void*)occluded);
    RenderParams P;
    size_t lds;
    if (int rc = query_setup(c, "rt_occluded", P, lds)) return rc;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    const hipError_t e = c->precision == RT_PREC_F64 ? launch_occluded_f64(P, lds, st, rays, n, intervals, occluded)
                                                     : launch_occluded_f32(P, lds, st, rays, n, intervals, occluded);
    return timed_end(c, st, e, "occlusion launch");
}

int rt_radiance_rays(rt_ctx* c, const void* rays, int n, const rt_path_key* keys, int max_depth, void* radiance,
                     uint32_t* segments, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_radiance_rays before rt_upload_scene");
    if (n < 0 || (n > 0 && (!rays || !radiance)))
        return fail(c, RT_ERR_INVALID, "rt_radiance_rays: %d rays, rays %p, radiance %p", n, rays, radiance);
    if (c->precision == RT_PREC_F64 && max_depth > 64)
        return fail(c, RT_ERR_LIMIT, "fp64 path keeps at most 64 bounces (max_depth %d)", max_depth);
    RenderParams P;
    size_t lds;
    if (int rc = query_setup(c, "rt_radiance_rays", P, lds)) return rc;
    if (n == 0) return RT_OK;
    P.max_depth = max_depth;
    HIPCHK(c, c->d_queue_rad.reserve(QUEUE_CTRL_BYTES));
    P.queue = c->d_queue_rad.as<uint32_t>();
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    hipError_t e;
    if (max_depth <= 0) {   // camera_cpu.h:9-10: no path, no light (all-zero bits are 0 in either precision)
        e = hipMemsetAsync(radiance, 0, (size_t)n * 3 * elem_bytes(c), st);
        if (e == hipSuccess && segments) e = hipMemsetAsync(segments, 0, (size_t)n * sizeof(uint32_t), st);
    } else {
        e = hipMemsetAsync(P.queue, 0, QUEUE_CTRL_BYTES, st);
        if (e == hipSuccess)
            e = c->precision == RT_PREC_F64
                    ? launch_radiance_f64(P, lds, st, rays, n, keys, radiance, segments, c->n_cu)
                    : launch_radiance_f32(P, lds, st, rays, n, keys, radiance, segments, c->n_cu);
    }
    return timed_end(c, st, e, "radiance launch");
}

// rt_render_pixels / rt_camera_rays: offsets = the exclusive scan of the valid jobs' counts on
// `st` (c->d_px_offsets), and T = offsets[num_jobs] read back -- the calls' one synchronisation.
// T > 2^31 - 1 is RT_ERR_LIMIT, the only one from here, and `total` holds T all the same.
static int pixel_scan(rt_ctx* c, const char* what, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs,
                      hipStream_t st, unsigned long long& total) {
    int rc;
    if ((rc = reserve(c, c->d_px_offsets, ((size_t)num_jobs + 1) * sizeof(unsigned long long))))
        return rc;
    const uint32_t npix = (uint32_t)((long long)cam->image_width * cam->image_height);   // (check_camera: < 2^29)
    size_t tmp = 0;
    unsigned long long* off = c->d_px_offsets.as<unsigned long long>();
    HIPCHK(c, launch_pixel_scan(jobs, num_jobs, npix, off, nullptr, &tmp, st));
    if ((rc = reserve(c, c->d_px_scan, tmp))) return rc;
    HIPCHK(c, launch_pixel_scan(jobs, num_jobs, npix, off, c->d_px_scan.p, &tmp, st));
    HIPCHK(c, hipMemcpyAsync(&total, off + num_jobs, sizeof(total), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (total > 0x7fffffffull) return fail(c, RT_ERR_LIMIT, "%s: %llu samples (> 2^31 - 1)", what, total);
    return RT_OK;
}

int rt_camera_rays(rt_ctx* c, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, void* rays,
                   rt_path_key* keys, int32_t* ray_job, int64_t max_rays, int64_t* num_rays, void* stream) {
    if (!c) return RT_ERR_INVALID;
    int rc = check_camera(c, cam);
    if (rc) return rc;
    if (num_jobs < 0 || (num_jobs > 0 && (!jobs || !rays || !keys)))
        return fail(c, RT_ERR_INVALID, "rt_camera_rays: %d jobs, jobs %p, rays %p, keys %p", num_jobs, (const void*)jobs,
                    rays, (void*)keys);
    if (num_jobs == 0) {
        if (num_rays) *num_rays = 0;
        return RT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    unsigned long long total = 0;
    rc = pixel_scan(c, "rt_camera_rays", cam, jobs, num_jobs, st, total);
    if (num_rays && (rc == RT_OK || rc == RT_ERR_LIMIT)) *num_rays = (int64_t)total;   // (the scan has run)
    if (rc) return rc;
    if ((int64_t)total > max_rays)
        return fail(c, RT_ERR_INVALID, "rt_camera_rays: %llu rays for buffers of %lld", total, (long long)max_rays);
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    fill_camera(c, cam, P);
    const unsigned long long* off = c->d_px_offsets.as<unsigned long long>();
    const hipError_t e =
        c->precision == RT_PREC_F64
            ? launch_camera_rays_f64(P, st, jobs, off, num_jobs, (long long)total, rays, keys, ray_job)
            : launch_camera_rays_f32(P, st, jobs, off, num_jobs, (long long)total, rays, keys, ray_job);
    return timed_end(c, st, e, "camera-ray launch");
}

// What a job-list query (rt_render_pixels, rt_render_pixels_moments, rt_render_pixels_aov) holds
// once job_query_begin has run.
struct JobQuery {
    RenderParams P;
    size_t lds;
    int grid;   // what the call walks: 0 the tree, else TRAV_GRID [| TRAV_GFLAT] (plan_job_query)
    hipStream_t st;
    unsigned long long total;   // T = offsets[num_jobs] (c->d_px_offsets), where the list was scanned
};

// The prologue of those calls, in the order their errors are found: the context, the scene, the
// camera; the call's own argument checks (`args`: RT_OK, or what fail returned); query_setup; then,
// for a list that has jobs, the stream, ev0 and -- with `scan` -- pixel_scan.  A caller returns
// what this returns where that is an error or num_jobs == 0.
static int job_query_begin(rt_ctx* c, const char* what, int call, const rt_camera* cam, const rt_pixel_job* jobs,
                           int num_jobs, void* stream, bool scan, const std::function<int()>& args, JobQuery& q) {
    if (!c) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "%s before rt_upload_scene", what);
    int rc = check_camera(c, cam);
    if (rc) return rc;
    if ((rc = args())) return rc;
    if ((rc = query_setup(c, what, q.P, q.lds, cam, call, &q.grid))) return rc;
    q.total = 0;
    if (num_jobs == 0) return RT_OK;
    q.st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, q.st));
    return scan ? pixel_scan(c, what, cam, jobs, num_jobs, q.st, q.total) : RT_OK;
}

// The fp64 passes of those calls: a sample's record is doubles and one 32-bit word, sample_bytes
// in all, kept in two arrays (c->d_px_samples.as<double>(), c->d_px_sseg.as<uint32_t>()) that hold a pass -- at most
// floor(sample_buffer_mb 2^20 / sample_bytes) samples.  run(q0, q1) launches and reduces flat
// samples [q0, q1), in order; the first pass also fills the jobs without samples, so it runs even
// when T = 0.  e: the first launch error.
static int sample_passes(rt_ctx* c, unsigned long long total, size_t sample_bytes, hipError_t& e,
                         const std::function<hipError_t(unsigned long long, unsigned long long)>& run) {
    const unsigned long long fit = ((unsigned long long)c->tuning.sample_buffer_mb << 20) / sample_bytes;
    const unsigned long long pass = std::max(1ull, std::min(fit, total));
    int rc;
    if ((rc = reserve(c, c->d_px_samples, (size_t)pass * (sample_bytes - sizeof(uint32_t)))))
        return rc;
    if ((rc = reserve(c, c->d_px_sseg, (size_t)pass * sizeof(uint32_t)))) return rc;
    unsigned long long q0 = 0;
    do {
        const unsigned long long q1 = std::min(total, q0 + pass);
        e = run(q0, q1);
        q0 = q1;
    } while (q0 < total && e == hipSuccess);
    return RT_OK;
}

// rt_render_pixels, and with `moments` rt_render_pixels_moments: the same launches, with the
// second moment's path kernel (fp32, csrc/rt_moments.h) or reduction (fp64).
static int render_pixels(rt_ctx* c, const char* what, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs,
                         int max_depth, int accumulate, void* out_sums, bool moments, void* out_sumsq,
                         uint32_t* out_segments, void* stream) {
    JobQuery q;
    // (max_depth <= 0 renders nothing and needs no scan)
    int rc = job_query_begin(c, what, moments ? RT_QUERY_MOMENTS : RT_QUERY_PIXELS, cam, jobs, num_jobs, stream,
                             max_depth > 0, [&] {
        if (num_jobs < 0 || (num_jobs > 0 && (!jobs || !out_sums || (moments && !out_sumsq))))
            return fail(c, RT_ERR_INVALID, "%s: %d jobs, jobs %p, out_sums %p, out_sumsq %p", what, num_jobs,
                        (const void*)jobs, out_sums, out_sumsq);
        if (c->precision == RT_PREC_F64 && max_depth > 64)
            return fail(c, RT_ERR_LIMIT, "fp64 path keeps at most 64 bounces (max_depth %d)", max_depth);
        return (int)RT_OK;
    }, q);
    if (rc || num_jobs == 0) return rc;
    RenderParams& P = q.P;
    const size_t lds = q.lds, nj = (size_t)num_jobs;
    const unsigned long long total = q.total;
    const hipStream_t st = q.st;
    const int acc = accumulate ? 1 : 0;
    hipError_t e = hipSuccess;
    if (max_depth <= 0) {   // camera_cpu.h:9-10: no path, no light; accumulate: nothing to add
        if (!accumulate) {
            e = hipMemsetAsync(out_sums, 0, nj * 3 * elem_bytes(c), st);
            if (e == hipSuccess && moments) e = hipMemsetAsync(out_sumsq, 0, nj * 3 * elem_bytes(c), st);
            if (e == hipSuccess && out_segments) e = hipMemsetAsync(out_segments, 0, nj * sizeof(uint32_t), st);
        }
    } else {
        P.max_depth = max_depth;
        HIPCHK(c, c->d_queue_px.reserve(QUEUE_CTRL_BYTES));
        P.queue = c->d_queue_px.as<uint32_t>();
        const unsigned long long* off = c->d_px_offsets.as<unsigned long long>();
        if (c->precision != RT_PREC_F64) {
            if ((rc = reserve(c, c->d_px_acc, nj * 3 * sizeof(long long)))) return rc;
            if ((rc = reserve(c, c->d_px_flags, nj * sizeof(uint32_t)))) return rc;
            if (moments) {
                if ((rc = reserve(c, c->d_px_sq, nj * 6 * sizeof(unsigned long long)))) return rc;
                if ((rc = reserve(c, c->d_px_sqflags, nj * sizeof(uint32_t)))) return rc;
            }
            long long* sum = c->d_px_acc.as<long long>();
            uint32_t* flags = c->d_px_flags.as<uint32_t>();
            unsigned long long* sq = c->d_px_sq.as<unsigned long long>();
            uint32_t* sqflags = c->d_px_sqflags.as<uint32_t>();
            e = launch_pixels_seed(off, num_jobs, acc, (const float*)out_sums, sum, flags, out_segments, st);
            if (e == hipSuccess && moments)
                e = launch_pixels_seed_moments(off, num_jobs, acc, (const float*)out_sumsq, sq, sqflags, st);
            if (e == hipSuccess) e = hipMemsetAsync(P.queue, 0, QUEUE_CTRL_BYTES, st);
            if (e == hipSuccess)
                e = moments ? launch_pixels_moments_f32(P, lds, st, jobs, off, num_jobs, total, 0, (int)total,
                                                        (unsigned long long*)sum, flags, out_segments, sq, sqflags,
                                                        c->n_cu, c->tuning.grid_workgroups)
                            : launch_pixels_f32(P, lds, st, jobs, off, num_jobs, total, 0, (int)total,
                                                (unsigned long long*)sum, flags, out_segments, c->n_cu, q.grid);
            if (e == hipSuccess) e = launch_pixels_finalize(off, num_jobs, acc, sum, flags, (float*)out_sums, st);
            if (e == hipSuccess && moments)
                e = launch_pixels_finalize_moments(off, num_jobs, acc, sq, sqflags, (float*)out_sumsq, st);
        } else {
            rc = sample_passes(c, total, PX_SAMPLE_BYTES, e, [&](unsigned long long q0, unsigned long long q1) {
                double* smp = c->d_px_samples.as<double>();
                uint32_t* sseg = c->d_px_sseg.as<uint32_t>();
                hipError_t pe = hipMemsetAsync(P.queue, 0, QUEUE_CTRL_BYTES, st);
                if (pe == hipSuccess)
                    pe = launch_pixels_f64(P, lds, st, jobs, off, num_jobs, total, q0, (int)(q1 - q0), smp, sseg, c->n_cu,
                                           q.grid, moments ? c->tuning.grid_workgroups : 0);
                if (pe == hipSuccess)
                    pe = moments ? launch_pixels_reduce_moments(off, num_jobs, q0, q1, smp, sseg, acc, (double*)out_sums,
                                                                (double*)out_sumsq, out_segments, st)
                                 : launch_pixels_reduce(off, num_jobs, q0, q1, smp, sseg, acc, (double*)out_sums,
                                                        out_segments, st);
                return pe;
            });
            if (rc) return rc;
        }
    }
    return timed_end(c, st, e, "pixel render launch");
}

int rt_render_pixels(rt_ctx* c, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, int max_depth,
                     int accumulate, void* out_sums, uint32_t* out_segments, void* stream) {
    return render_pixels(c, "rt_render_pixels", cam, jobs, num_jobs, max_depth, accumulate, out_sums, false, nullptr,
                         out_segments, stream);
}

int rt_render_pixels_moments(rt_ctx* c, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, int max_depth,
                             int accumulate, void* out_sums, void* out_sumsq, uint32_t* out_segments, void* stream) {
    return render_pixels(c, "rt_render_pixels_moments", cam, jobs, num_jobs, max_depth, accumulate, out_sums, true,
                         out_sumsq, out_segments, stream);
}

// rt_render_pixels_aov: rt_render_pixels' prologue, scratch and passes; one first-hit kernel in
// place of the path kernel, the sums' seed and finalize launches once per summed output.
int rt_render_pixels_aov(rt_ctx* c, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, int accumulate,
                         const rt_aov_buffers* out, void* stream) {
    const char* what = "rt_render_pixels_aov";
    JobQuery q;
    int rc = job_query_begin(c, what, RT_QUERY_AOV, cam, jobs, num_jobs, stream, true, [&] {
        if (num_jobs < 0 || (num_jobs > 0 && (!jobs || !out)))
            return fail(c, RT_ERR_INVALID, "%s: %d jobs, jobs %p, out %p", what, num_jobs, (const void*)jobs,
                        (const void*)out);
        if (out && !out->albedo && !out->normal && !out->depth && !out->id && !out->hits)
            return fail(c, RT_ERR_INVALID, "%s: every member of rt_aov_buffers is NULL", what);
        return (int)RT_OK;
    }, q);
    if (rc || num_jobs == 0) return rc;
    const RenderParams& P = q.P;
    const size_t lds = q.lds, nj = (size_t)num_jobs;
    const unsigned long long total = q.total;
    const hipStream_t st = q.st;
    const rt_aov_buffers o = *out;
    const int acc = accumulate ? 1 : 0;
    const unsigned long long* off = c->d_px_offsets.as<unsigned long long>();
    const int* remap = c->scene.d_remap.as<int>();
    if ((rc = reserve(c, c->d_aov_near, nj * 16))) return rc;
    hipError_t e = hipSuccess;
    if (c->precision != RT_PREC_F64) {
        // albedo's sums and flags, then normal's, in rt_render_pixels' scratch
        if ((rc = reserve(c, c->d_px_acc, nj * 6 * sizeof(long long)))) return rc;
        if ((rc = reserve(c, c->d_px_flags, nj * 2 * sizeof(uint32_t)))) return rc;
        long long* acc_a = o.albedo ? c->d_px_acc.as<long long>() : nullptr;
        long long* acc_n = o.normal ? c->d_px_acc.as<long long>() + nj * 3 : nullptr;
        uint32_t *fl_a = c->d_px_flags.as<uint32_t>(), *fl_n = c->d_px_flags.as<uint32_t>() + nj;
        unsigned long long* near = (o.depth || o.id) ? c->d_aov_near.as<unsigned long long>() : nullptr;
        if (acc_a) e = launch_pixels_seed(off, num_jobs, acc, (const float*)o.albedo, acc_a, fl_a, nullptr, st);
        if (e == hipSuccess && acc_n)
            e = launch_pixels_seed(off, num_jobs, acc, (const float*)o.normal, acc_n, fl_n, nullptr, st);
        if (e == hipSuccess && (near || o.hits))
            e = launch_aov_seed(off, num_jobs, acc, (const float*)o.depth, o.id, near, o.hits, st);
        if (e == hipSuccess)
            e = launch_aov_f32(P, lds, st, jobs, off, num_jobs, total, remap, (unsigned long long*)acc_a, fl_a,
                               (unsigned long long*)acc_n, fl_n, near, o.hits, c->n_cu, c->aov_combine != 0);
        if (e == hipSuccess && acc_a) e = launch_pixels_finalize(off, num_jobs, acc, acc_a, fl_a, (float*)o.albedo, st);
        if (e == hipSuccess && acc_n) e = launch_pixels_finalize(off, num_jobs, acc, acc_n, fl_n, (float*)o.normal, st);
        if (e == hipSuccess && near) e = launch_aov_finalize(off, num_jobs, acc, near, (float*)o.depth, o.id, st);
    } else {
        rc = sample_passes(c, total, AOV_SAMPLE_BYTES, e, [&](unsigned long long q0, unsigned long long q1) {
            double* smp = c->d_px_samples.as<double>();
            int32_t* sid = c->d_px_sseg.as<int32_t>();
            const hipError_t pe =
                launch_aov_f64(P, lds, st, jobs, off, num_jobs, total, q0, (int)(q1 - q0), remap, smp, sid, c->n_cu);
            return pe != hipSuccess
                       ? pe
                       : launch_aov_reduce(off, num_jobs, q0, q1, smp, sid, acc, c->d_aov_near.p, (double*)o.albedo,
                                           (double*)o.normal, (double*)o.depth, o.id, o.hits, st);
        });
        if (rc) return rc;
    }
    return timed_end(c, st, e, "aov launch");
}

int rt_refine_jobs(rt_ctx* c, rt_pixel_job* jobs, int num_jobs, const void* sums, const void* sumsq,
                   const rt_adaptive_params* ap, uint64_t* stats, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (num_jobs < 0 || (num_jobs > 0 && (!jobs || !sums || !sumsq || !ap || !stats)))
        return fail(c, RT_ERR_INVALID, "rt_refine_jobs: %d jobs, jobs %p, sums %p, sumsq %p, params %p, stats %p",
                    num_jobs, (void*)jobs, sums, sumsq, (const void*)ap, (void*)stats);
    if (ap && (ap->min_samples < 2 || ap->min_samples > ap->max_samples || ap->max_samples > 0x7fffffffu ||
               ap->max_step == 0))
        return fail(c, RT_ERR_INVALID, "rt_refine_jobs: 2 <= min_samples %u <= max_samples %u <= 2^31 - 1, max_step %u >= 1",
                    ap->min_samples, ap->max_samples, ap->max_step);
    if (ap && !(std::isfinite(ap->rel_error) && ap->rel_error >= 0.0 && std::isfinite(ap->abs_floor) &&
                ap->abs_floor >= 0.0))
        return fail(c, RT_ERR_INVALID, "rt_refine_jobs: rel_error %g and abs_floor %g must be finite and >= 0",
                    ap->rel_error, ap->abs_floor);
    if (!stats) return RT_OK;   // (no jobs, nothing to count)
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(uint64_t), st);
    if (e == hipSuccess && num_jobs > 0)
        e = launch_refine_jobs(jobs, num_jobs, sums, sumsq, (int)elem_bytes(c), ap->rel_error, ap->abs_floor,
                               ap->min_samples, ap->max_samples, ap->max_step, (unsigned long long*)stats, st);
    return timed_end(c, st, e, "refine launch");
}

static const rt_denoise_params DENOISE_DEFAULTS = {5, 7, 0.05, 4.0, 1e-6};

int rt_denoise_default_params(rt_denoise_params* p) {
    if (!p) return RT_ERR_INVALID;
    *p = DENOISE_DEFAULTS;
    return RT_OK;
}

// rt_denoise: validation, the three record images of scratch, then rt_denoise.hip's launches
// between the context's two events.  Nothing is launched or written before every check has passed.
int rt_denoise(rt_ctx* c, int width, int height, const void* sums, const void* sumsq, const uint32_t* counts,
               int samples, const rt_aov_buffers* guides, int guide_samples, const rt_denoise_params* params, void* out,
               void* out_variance, void* stream) {
    if (!c) return RT_ERR_INVALID;
    if (!sums || !out) return fail(c, RT_ERR_INVALID, "rt_denoise: sums %p, out %p", sums, out);
    if (width < 1 || height < 1 || (long long)width * height > 0x7fffffffll)
        return fail(c, RT_ERR_INVALID, "rt_denoise: image size %dx%d (1 <= width height <= 2^31 - 1)", width, height);
    if (!counts && samples < 1)
        return fail(c, RT_ERR_INVALID, "rt_denoise: counts is NULL and samples is %d (>= 1)", samples);
    const rt_aov_buffers g = guides ? *guides : rt_aov_buffers{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (g.albedo && (!g.hits || guide_samples < 1))
        return fail(c, RT_ERR_INVALID, "rt_denoise: an albedo guide needs hits (%p) and guide_samples %d >= 1",
                    (void*)g.hits, guide_samples);
    const rt_denoise_params dp = params ? *params : DENOISE_DEFAULTS;
    if (dp.iterations < 0 || dp.iterations > 8 || dp.normal_log2_power < 0 || dp.normal_log2_power > 10)
        return fail(c, RT_ERR_INVALID, "rt_denoise: 0 <= iterations %d <= 8, 0 <= normal_log2_power %d <= 10",
                    dp.iterations, dp.normal_log2_power);
    if (!(std::isfinite(dp.sigma_depth) && dp.sigma_depth > 0.0 && std::isfinite(dp.sigma_lum) && dp.sigma_lum >= 0.0 &&
          std::isfinite(dp.lum_eps) && dp.lum_eps > 0.0))
        return fail(c, RT_ERR_INVALID, "rt_denoise: sigma_depth %g > 0, sigma_lum %g >= 0 and lum_eps %g > 0 must be finite",
                    dp.sigma_depth, dp.sigma_lum, dp.lum_eps);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t image = (size_t)width * (size_t)height * 4 * elem_bytes(c);
    int rc;
    if ((rc = reserve(c, c->d_dn_a, image)) || (rc = reserve(c, c->d_dn_b, dp.iterations ? image : 0)) ||
        (rc = reserve(c, c->d_dn_guide, image)))
        return rc;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    DenoiseLaunch D;
    D.elem_bytes = (int)elem_bytes(c), D.width = width, D.height = height;
    D.samples = samples, D.guide_samples = guide_samples;
    D.iterations = dp.iterations, D.normal_log2_power = dp.normal_log2_power;
    D.sigma_depth = dp.sigma_depth, D.sigma_lum = dp.sigma_lum, D.lum_eps = dp.lum_eps;
    D.sums = sums, D.sumsq = sumsq, D.counts = counts;
    D.albedo = g.albedo, D.normal = g.normal, D.depth = g.depth, D.hits = g.albedo ? g.hits : nullptr;
    D.col_a = c->d_dn_a.p, D.col_b = c->d_dn_b.p, D.guide = c->d_dn_guide.p;
    D.out = out, D.out_variance = out_variance;
    return timed_end(c, st, launch_denoise(D, st), "denoise launch");
}

int rt_trace_rays_diag(rt_ctx* c, const void* rays, int n, rt_hit* hits, uint64_t counters[4]) {
    if (!c || !counters) return RT_ERR_INVALID;
    if (c->precision != RT_PREC_F32 || c->scene.n_mnodes > 0)
        return fail(c, RT_ERR_INVALID, "rt_trace_rays_diag instruments the fp32 sphere-scene kernel");
    DevBuf counts;
    HIPCHK(c, counts.reserve(DIAG_SLOTS * sizeof(unsigned long long)));
    unsigned long long* d = counts.as<unsigned long long>();
    hipError_t e = hipMemsetAsync(d, 0, DIAG_SLOTS * sizeof(unsigned long long), c->stream);
    int rc = e == hipSuccess ? trace_rays(c, rays, n, nullptr, hits, c->stream, d) : RT_OK;
    unsigned long long h[DIAG_SLOTS] = {};
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == RT_OK) e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, RT_ERR_HIP, "trace diag: %s", hipGetErrorString(e));
    for (int k = 0; k < 4; ++k) counters[k] = h[2 + k];   // inner_it, inner_act, leaf_it, leaf_act
    return RT_OK;
}

static_assert(DIAG_SLOTS == RT_DIAG_SLOTS, "diag slots");
int rt_render_diag(rt_ctx* c, const rt_camera* cam, int spp, int max_depth, uint64_t counters[16]) {
    return rt_render_diag_ex(c, cam, spp, max_depth, counters, 16);
}

int rt_render_diag_ex(rt_ctx* c, const rt_camera* cam, int spp, int max_depth, uint64_t* counters, int n) {
    if (!c || !counters || n < 1 || n > DIAG_SLOTS)
        return c ? fail(c, RT_ERR_INVALID, "rt_render_diag_ex: counters and 1 <= n <= %d", DIAG_SLOTS) : RT_ERR_INVALID;
    if (c->precision != RT_PREC_F32) return fail(c, RT_ERR_INVALID, "rt_render_diag instruments the fp32 kernel");
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "no scene");
    if (spp > FIX_LAUNCH_SAMPLES) return fail(c, RT_ERR_INVALID, "rt_render_diag: spp <= %d", FIX_LAUNCH_SAMPLES);
    int rc = check_camera(c, cam);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rt_shard_info si;
    rt_shard_layout(cam->image_width, cam->image_height, 0, 1, &si);
    if ((rc = reserve(c, c->d_shard, (size_t)si.num_tiles * 64 * 3 * 4))) return rc;
    DevBuf counts;
    HIPCHK(c, counts.reserve(DIAG_SLOTS * sizeof(unsigned long long)));
    unsigned long long* d = counts.as<unsigned long long>();
    hipError_t e = hipMemsetAsync(d, 0, DIAG_SLOTS * sizeof(unsigned long long), c->stream);
    // the persistent kernel of rt_render, instrumented (block 512, <= 64 VGPRs; the
    // coherent-primary kernel at the context's block, 512 or 1024; the ray pool at 512)
    // exactly the kernel rt_render runs for this tuning, instrumented (RT_DIAG_VARIANTS);
    // a tuning with no instrumented build is refused (RT_ERR_INVALID), never substituted
    c->diag_buf = d;
    if (e == hipSuccess) rc = rt_render(c, cam, spp, max_depth, 0, 1, c->d_shard.p, nullptr, nullptr);
    c->diag_buf = nullptr;
    if (e == hipSuccess && rc == RT_OK)
        e = hipMemcpyAsync(counters, d, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == RT_OK) e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, RT_ERR_HIP, "diag render: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_trace_tape(rt_ctx* c, const double ray[7], int depth, const double* tape, int tape_len, double out[3],
                  int* used) {
    if (!c || !ray || !out || !used || tape_len < 0 || (tape_len > 0 && !tape)) return RT_ERR_INVALID;
    if (!c->scene.has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_trace_tape before rt_upload_scene");
    if (c->precision != RT_PREC_F64) return fail(c, RT_ERR_INVALID, "rt_trace_tape needs an RT_PREC_F64 context");
    if (depth > 64) return fail(c, RT_ERR_LIMIT, "depth %d > 64", depth);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = reserve(c, c->d_tape, (size_t)(tape_len > 0 ? tape_len : 1) * sizeof(double))))
        return rc;
    if (tape_len)
        HIPCHK(c, hipMemcpyAsync(c->d_tape.p, tape, (size_t)tape_len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_small.p, ray, 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rt_camera dummy{};
    dummy.image_width = dummy.image_height = 1;
    RenderParams P;
    fill_params(c, &dummy, 1, depth, plan_launch(c, true).mesh_stack, P);
    double* small = c->d_small.as<double>();
    HIPCHK(c, launch_tape_f64(P, depth, small, c->d_tape.as<double>(), tape_len, small + 8, c->d_used.as<int>(), c->stream));
    HIPCHK(c, hipMemcpyAsync(out, small + 8, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(used, c->d_used.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

}  // extern "C"
