/*
 * rt_hip.h -- C ABI of the MI355X path tracer (librt_hip.so).
 *
 * The reference has no FFI: its boundary is the C++ header API.  The
 * entry points below are what that API needs from a device backend; each cites the
 * reference interface it replaces.  include/rt/camera.h (C++ mirror of the reference
 * headers) is the drop-in caller; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every int-returning call
 * returns RT_OK (0) or a negative RT_ERR_* code; rt_last_error() has the message.
 * Device pointers are hipMalloc'd (or torch CUDA tensors); `stream` is a hipStream_t or
 * NULL for the context's own stream.  One context per process and GPU (the multi-GPU
 * path runs one process per GPU).
 */
#ifndef RT_HIP_H
#define RT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 12

enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,   /* bad argument                                  */
    RT_ERR_HIP = -2,       /* a HIP runtime call failed                     */
    RT_ERR_NO_SCENE = -3,  /* rt_render before rt_upload_scene              */
    RT_ERR_LIMIT = -4,     /* scene/BVH/depth beyond what the kernel holds */
    RT_ERR_COMM = -5       /* an RCCL call failed (message: ncclGetErrorString) */
};

enum { RT_LAMBERTIAN = 0, RT_METAL = 1, RT_DIELECTRIC = 2 };  /* material.h:15,31,48 */
enum { RT_PREC_F32 = 0, RT_PREC_F64 = 1 };

/* sphere.h:9-28.  center_vec = center2 - center1 exactly as sphere.h:27 computes it;
 * zero (and moving = 0) for a stationary sphere.  64 bytes. */
typedef struct {
    double center[3];
    double radius;
    double center_vec[3];
    int32_t mat;      /* index into the material array */
    int32_t moving;
} rt_sphere;

/* lambertian(albedo) material.h:17, metal(albedo, fuzz) :33 (fuzz clamped to 1 here
 * as there), dielectric(ir) :50.  48 bytes. */
typedef struct {
    int32_t type;
    int32_t pad;
    double albedo[3];
    double fuzz;
    double ir;
} rt_material;

/* A triangle (mesh path; the reference has no triangle primitive):
 * vertices in counter-clockwise order as seen from the outward side, material index.
 * 80 bytes. */
typedef struct {
    double v0[3], v1[3], v2[3];
    int32_t mat;
    int32_t pad;
} rt_triangle;

/* OBJ geometry as loaded by rt_obj_load: num_vertices xyz doubles and num_triangles
 * index triples (0-based) after fan triangulation of num_faces faces. */
typedef struct {
    int32_t num_vertices, num_faces, num_triangles, pad;
    double* vertices;
    int32_t* indices;
} rt_obj_mesh;

/* The camera AFTER camera::initialize() (camera.h:52-85): the derived members of
 * camera.h:117-125 plus defocus_angle (camera.h:25, tested in get_ray :94). */
typedef struct {
    int32_t image_width, image_height;
    double center[3];
    double pixel00_loc[3];
    double pixel_delta_u[3];
    double pixel_delta_v[3];
    double defocus_disk_u[3];
    double defocus_disk_v[3];
    double defocus_angle;
} rt_camera;

/* camera.h:15-26: the public fields a caller sets before render(). */
typedef struct {
    double aspect_ratio;
    int32_t image_width, samples_per_pixel, max_depth, pad;
    double vfov;
    double lookfrom[3], lookat[3], vup[3];
    double defocus_angle, focus_dist;
} rt_camera_desc;

/* Framebuffer tiling for the multi-GPU split: 8x8-pixel tiles in
 * row-major tile order; tile t belongs to shard t % num_shards.  A shard buffer holds
 * its tiles back to back, 64 pixels x 3 channels each, pixel (x%8, y%8) at lane
 * (y%8)*8 + x%8. */
typedef struct {
    int32_t tile_w, tile_h;
    int32_t tiles_x, tiles_y, num_tiles;
    int32_t shard, num_shards, shard_tiles, max_shard_tiles;
} rt_shard_info;

typedef struct {
    int32_t num_spheres, num_materials;
    int32_t bvh_nodes, bvh_depth, bvh_leaves, big_spheres;
    int32_t lds_bytes;
    int32_t precision;
    int32_t num_triangles, mesh_nodes, mesh_depth, mesh_leaves;   /* mesh BVH: 4-wide nodes, their depth */
    int32_t render_block;   /* threads per workgroup the render kernel uses for this scene */
    int32_t render_traversal;   /* traversal flags of the fp32 kernel this scene runs (the tuning's, with 128
                                   added where the LDS sums would cost occupancy, 8192 added for fp32 mesh
                                   scenes unless 16384 was asked for, 131072 added to 65536 on a grid one
                                   cell tall in y unless 262144 was asked for) */
    int32_t render_waves_per_eu;    /* register-budget key of that fp32 kernel (waves_per_eu, or for meshes the
                                       resolved mesh_waves_per_eu: 0 or 6); 0 for fp64 (ABI 7) */
    int32_t render_mesh_lds_stack;  /* mesh traversal stack entries per lane it keeps in LDS (the resolved
                                       mesh_lds_stack); 0 without a mesh (ABI 7) */
    int32_t grid_res[3];    /* the uniform sphere grid's cells per axis (0 0 0: none built; ABI 8) */
    int32_t grid_entries;   /* sphere references listed over its cells */
    /* ABI 10: what the current grid was built with (the tuning's sphere_grid_density and
       sphere_grid_time_slabs at the last rt_upload_scene; 0 without a grid), and its walk's reach:
       the walk is exact and ends for ray origins within +-grid_far_o on every axis (its fp32 plane
       distances lose precision beyond); a launch whose camera or scene could start a ray beyond
       it renders with the sphere tree instead, the same frame (rt_grid_reach).  render_* above
       describe a launch within reach. */
    int32_t grid_time_slabs;
    float grid_far_o;
    double grid_density;
} rt_scene_info;

/* Kernel/BVH tuning (defaults are the measured best).  block: threads
 * per workgroup of the render kernel (fp64 always 256); max_leaf, the SAH costs and the
 * mesh_* build fields shape the BVHs built by the next rt_upload_scene[_ex].  Only the
 * (block, waves_per_eu, traversal) combinations instantiated in rt_render_f32.hip render
 * (rt_set_tuning checks the requested one, rt_render_range the one the scene runs -- the
 * library may add 128 -- with a clear RT_ERR_INVALID); meshes have their own smaller
 * set.  Every combination renders the same pixels bit for bit (the fp32 kernels fuse
 * multiply-adds only within one expression, -ffp-contract=on, so every inlined copy
 * rounds alike); the fp64 path ignores the kernel fields. */
typedef struct {
    int32_t block;
    int32_t max_leaf;
    double cost_traverse, cost_intersect;
    int32_t waves_per_eu;   /* fp32 register budget: 0 = compiler's choice, 4 / 6 / 8 = <= 128 / 80 / 64 VGPRs */
    int32_t traversal;      /* flags: 8 select root, 16 whole-record (b128) LDS reads of nodes and spheres,
                               64 coherent primaries (camera rays traced in per-tile batches), 128 with 64:
                               no LDS pixel sums (set automatically where they would cost occupancy), 512
                               pop culling (a popped stack top whose box starts beyond the closest hit so
                               far is dropped unvisited), 8192 (fp32 mesh scenes; added by the library
                               wherever instantiated) the if-if mesh loop -- each iteration a lane visits
                               one node or tests one leaf, node and triangle loads issued together -- and
                               16384 (mesh scenes) the while-while mesh loop of rounds 1-3 instead,
                               65536 (ABI 8) the uniform sphere grid instead of the sphere BVH -- dropped
                               where rt_upload_scene built no grid (sphere_grid_density 0, or no sphere
                               outside the front list and the ground class); mixed scenes get it in their
                               mesh kernels where instantiated, fp64 through f64_kernel 5 (C3 fp32 48.2 ->
                               38.3 ms, fp64 97.1 -> 81.7 ms; C5 geometry -9.5 %; r05).
                               131072 (ABI 11; added by the library with 65536 wherever the grid is one
                               cell tall in y -- main.cpp's field on its ground -- and the kernel exists:
                               the walk steps in x and z only; C3 -6 %, the same frame) unless 262144
                               (never in a kernel key) asks to keep the 3-D walk; fp64 likewise.
                               32768 (quantised 64-B mesh nodes) was measured slower in r05 and is refused.
                               256 (time-binned sphere trees) and 4096 (an LDS copy of the mesh tree top)
                               were measured slower, removed in ABI 6 and are refused.
                               Default RT_TRAV_DEFAULT with block 1024; the
                               one-path-per-lane kernel is traversal 8 with block 512.  Every combination
                               gives the same frame bit for bit */
    int32_t mesh_max_leaf;  /* triangle BVH: at most this many triangles per leaf (1..8; default 2) */
    int32_t mesh_lds_nodes; /* reserved (-1..4096 accepted, no effect): the LDS tree-top kernels it sized
                               (traversal 4096) were removed in ABI 6 */
    double mesh_cost_traverse;  /* triangle BVH SAH: node cost relative to one triangle test */
    int32_t chunk_waves;    /* reserved (>= 0 accepted, no effect): the one-wave-per-tile F64 kernels 1 / 2
                               whose samples it split were removed in ABI 6; every kernel now runs
                               persistent lanes over the work queue (item_* below) */
    int32_t sample_buffer_mb;  /* F64: cap of the per-sample radiance buffer (MiB) of kernels 3 / 4; longer
                               sample ranges run in passes, each of at most 65535 samples (the coherent
                               kernel's FIFO keeps a sample's index within its pass in 16 bits) and at
                               least one; >= 1 (>= 16 before rt_render_pixels_moments) */
    int32_t mesh_builder;   /* RT_MESH_BUILD_HOST: binned SAH on the host (best trees); RT_MESH_BUILD_GPU:
                               built on the device -- Morton-code LBVH, then two rounds of treelet
                               restructuring by SAH (r06, ABI 10; fast builds for large or changing
                               meshes); RT_MESH_BUILD_GPU_LBVH: the plain Morton-code LBVH (r03-r05) */
    int32_t mesh_waves_per_eu;  /* register budget of the mesh kernels: -1 = auto (the default: of the
                                   instantiated kernels, the one keeping more waves resident per CU, equal
                                   occupancy keeping the unspilled one), 0 = the compiler's budget (5 waves
                                   per SIMD; with mesh_block 512 only the while-while kernel exists there, so
                                   that pair renders only with traversal | 16384), 6 = <= 80 VGPRs (6 waves per SIMD; the path throughput spills
                                   once per bounce, none in the traversal loop; C4 -5 %, C5 geometry -12 %) */
    int32_t mesh_lds_stack;     /* mesh traversal stack entries per lane kept in LDS (0..64; deeper entries go
                                   to scratch memory); -1 = auto (the default): the most entries, up to 12,
                                   that cost no workgroup per CU -- none for the mixed-scene kernels over the
                                   sphere grid (r06: C5 geometry -2.7 %) */
    int32_t mesh_block;         /* threads per workgroup for scenes with a mesh: 256, 512, or 0 = auto (the
                                   one keeping more waves per CU given registers and LDS) */
    int32_t item_samples;       /* F32 work queue: samples per work item at most (1..32; items shrink to 1 */
    double item_balance;        /* sample towards the end: a chunk of c samples is handed out only while
                                   what is left keeps every resident lane busy for item_balance chunks;
                                   default 8 since r05 -- 4 before; C3 -0.6 %, its 8-GPU shard -1 %) */
    double mesh_item_balance;   /* item_balance for scenes with a mesh (their per-pixel cost varies more);
                                   fp32 doubles it on shards with fewer pixels than resident lanes */
    int32_t coh_refill;         /* coherent kernel: another shade round runs while at least this many lanes of
                                   a wave hold no ray (1..64; default 48) */
    int32_t f64_kernel;         /* fp64 render kernel: 0 = default (5 where the scene has a sphere grid and
                                   traversal carries RT_TRAV_GRID, else 4; 5 is kernel 4 walking the grid,
                                   ABI 8); 3 = conservative fp32 slab tests
                                   (each slab widened by a bound of its rounding: no box the exact ray
                                   enters is rejected) on persistent lanes over the work queue (item_*),
                                   each sample stored for the ordered reduction (sample_buffer_mb bounds
                                   the buffer); 4 = 3 with coherent primaries (camera rays traced in
                                   per-tile batches).  Both render the same frame bit for bit (kernels 1 /
                                   2, one wave per tile, were removed in ABI 6 and are refused) */
    int32_t grid_workgroups;    /* fp32 persistent kernels: workgroups per launch; 0 = what the device keeps
                                   resident (the default); more only queue behind them (tests) */
    int32_t front_spheres;      /* the N largest spheres (below the R >= 64 ground class) are tested by every
                                   ray before the BVH, outside it (0..16; 0 = all in the BVH; -1 = auto, the
                                   default: those with radius >= 4x the median, at most 8) */
    double sphere_grid_density; /* cells per sphere of the uniform sphere grid that traversal flag
                                   RT_TRAV_GRID traverses instead of the sphere BVH -- fp32 sphere and
                                   mixed scenes, and fp64 through f64_kernel 5 (built by rt_upload_scene
                                   over the spheres outside the front list, when the scene suits one: see
                                   build_sphere_grid); 0 = no grid (the BVH).  Read at rt_upload_scene: a
                                   later change takes effect at the next upload (rt_scene_info reports the
                                   values the current grid was built with) */
    int32_t sphere_grid_time_slabs; /* the grid's time slabs (1..64; default 32; ABI 9): a ray walks only the
                                   cells within the box of the spheres at its time's slab of [0, 1] (moving
                                   spheres fill less of their swept box at one time); 1 = the spheres'
                                   box over the whole shutter (C3 37.8 -> 36.2 ms, r05ao).  Read at
                                   rt_upload_scene, as sphere_grid_density */
} rt_tuning;
enum { RT_MESH_BUILD_HOST = 0, RT_MESH_BUILD_GPU = 1, RT_MESH_BUILD_GPU_LBVH = 2 };
enum { RT_TRAV_SELROOT = 8, RT_TRAV_B128 = 16, RT_TRAV_COH = 64, RT_TRAV_NOSUM = 128, RT_TRAV_TBIN = 256,
       RT_TRAV_CULL = 512, RT_TRAV_MTOP = 4096, RT_TRAV_MIFIF = 8192, RT_TRAV_MWHILE = 16384, RT_TRAV_MQ = 32768,
       RT_TRAV_GRID = 65536, RT_TRAV_GFLAT = 131072, RT_TRAV_G3D = 262144,
       RT_TRAV_DEFAULT = RT_TRAV_COH | RT_TRAV_SELROOT | RT_TRAV_B128 | RT_TRAV_CULL | RT_TRAV_GRID };

typedef struct rt_ctx rt_ctx;

/* ---- context ------------------------------------------------------------------ */
int rt_abi_version(void);
int rt_device_count(void);
/* precision: RT_PREC_F32 (fast path) or RT_PREC_F64 (reference-exact arithmetic).
 * seed keys the per-(pixel, sample) RNG streams (replaces rtweekend.h:25-29's global
 * mt19937, which no parallel renderer can share). */
rt_ctx* rt_create(int device, uint64_t seed, int precision);
void rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);
const char* rt_error_string(int code);
int rt_set_seed(rt_ctx* ctx, uint64_t seed);
void* rt_stream(rt_ctx* ctx);
int rt_get_tuning(rt_ctx* ctx, rt_tuning* t);
int rt_set_tuning(rt_ctx* ctx, const rt_tuning* t);

/* camera::initialize (camera.h:52-85) in fp64, operation for operation. */
int rt_camera_initialize(const rt_camera_desc* desc, rt_camera* cam);

/* ---- scene: replaces hittable_list::add (hittable_list.h:20-23) + bvh_node(list)
 * (bvh.h:10-14).  The host builds an SAH BVH over the spheres, keeps the very large
 * ones (the R=1000 ground, main.cpp:15) in a separate list tested in fp64, and uploads
 * the flattened arrays.  Arrays are copied; the caller keeps ownership. */
int rt_upload_scene(rt_ctx* ctx, const rt_sphere* spheres, int num_spheres, const rt_material* materials,
                    int num_materials);
/* ABI 10: 1 in *walks when a launch with this camera walks the sphere grid, 0 when it renders
 * with the sphere tree (no grid built, or a ray could start beyond the grid's reach,
 * rt_scene_info.grid_far_o: the camera itself, or hit points on the scene -- anywhere on its
 * spheres, triangles and the big spheres that refract or move, and the parts of static opaque
 * big spheres visible from those).  Either way the same frame. */
int rt_grid_reach(rt_ctx* ctx, const rt_camera* cam, int32_t* walks);
/* What a job-list query runs for this camera on the current scene and tuning: rt_pixels_plan for
 * rt_render_pixels, rt_pixels_plan_call for the call named by `call` (RT_QUERY_PIXELS
 * rt_render_pixels, RT_QUERY_MOMENTS rt_render_pixels_moments, RT_QUERY_AOV rt_render_pixels_aov).
 * The plan is per call family because the measurement was: a call walks the sphere grid only
 * where the grid beat the tree by more than the two runs' spreads at every sample count measured
 * (DESIGN.md §5 "Queries over the sphere grid") -- rt_render_pixels in both precisions and
 * rt_render_pixels_moments in fp64 contexts.  rt_render_pixels_moments in fp32 contexts and
 * rt_render_pixels_aov always walk the sphere tree (walks_grid 0).  A call that may walk the grid
 * does so if and only if all of these hold: the scene has no triangle mesh; rt_upload_scene built a grid
 * (rt_scene_info.grid_res != 0 0 0); rt_tuning.traversal carries 65536 (RT_TRAV_GRID), read at the
 * call as rt_render reads it; in fp64 contexts rt_tuning.f64_kernel resolves to a grid kernel (0
 * or 5; 3 and 4 force the tree, as for frames); the camera is within the walk's reach
 * (rt_grid_reach); and the grid's layout fits 160 KiB of LDS at the queries' workgroup size.
 * Otherwise they walk the sphere tree -- also where only the grid's layout does not fit.  The walk
 * is the flat one (131072, x and z steps only) iff the grid is one cell tall in y and the
 * traversal does not carry 262144 (RT_TRAV_G3D).  Either way the same outputs, bit for bit: the
 * grid and the tree find the same hit.
 * The per-ray queries (rt_trace_rays, rt_trace_rays_from, rt_occluded, rt_radiance_rays) take
 * the caller's rays, for which there is no reach to prove, and always walk the tree.
 * Launches nothing.  Errors: RT_ERR_INVALID for a NULL argument, a bad camera or an unknown call, RT_ERR_NO_SCENE
 * before an upload, RT_ERR_LIMIT where the query itself would return it (neither layout fits the
 * LDS, an image too large).  Added to ABI 12 without a version bump, as rt_occluded was. */
typedef struct {
    int32_t walks_grid;   /* 1: the sphere grid; 0: the sphere tree */
    int32_t traversal;    /* the kernel's traversal flags (RT_TRAV_*: 536 for fp32 sphere trees, 8712 with
                             a mesh, + 65536 [+ 131072] over the grid; fp64: 32 + the grid's flags, or 0
                             for the tree) */
    int32_t block;        /* threads per workgroup */
    int32_t lds_bytes;    /* dynamic LDS per workgroup */
} rt_pixels_plan_info;
enum { RT_QUERY_PIXELS = 0, RT_QUERY_MOMENTS = 1, RT_QUERY_AOV = 2 };
int rt_pixels_plan(rt_ctx* ctx, const rt_camera* cam, rt_pixels_plan_info* info);
int rt_pixels_plan_call(rt_ctx* ctx, const rt_camera* cam, int call, rt_pixels_plan_info* info);
int rt_scene_info_get(rt_ctx* ctx, rt_scene_info* info);
/* Spheres plus triangles (configs 4/5: mesh, mixed).  Triangles get their own 4-wide BVH,
 * HBM-resident (nodes and triangles are read through L2/Infinity Cache with global loads;
 * the traversal stack is an LDS column per lane, deeper entries in scratch), built on the
 * host (binned SAH) or on the device (LBVH) per rt_tuning.mesh_builder.  Triangles are
 * two-sided with the sphere path's (0.001, inf) interval: fp64 Moller-Trumbore (the oracle's
 * operation order), fp32 a watertight edge-function test (r05); rt_render_diag
 * instruments the default mesh kernels too (slots 27-30).  Coordinates (centres, motion,
 * radii, vertices) must be finite and within +-1e30 (RT_ERR_LIMIT otherwise). */
int rt_upload_scene_ex(rt_ctx* ctx, const rt_sphere* spheres, int num_spheres, const rt_material* materials,
                       int num_materials, const rt_triangle* triangles, int num_triangles);

/* ---- OBJ: replaces ModelLoader::load (src/vulkan/model_loader.h:17-19, an empty stub)
 * over the vendored, never-called tinyobjloader (tiny_obj_loader.h:605).  Returns RT_OK
 * and malloc'd arrays (release with rt_obj_free); RT_ERR_INVALID on a parse error (an
 * unreadable path, a face index naming no vertex, a coordinate that overflows to +-inf);
 * RT_ERR_LIMIT for a face with more than RT_OBJ_MAX_FACE_VERTICES corners or when memory
 * runs out.  Coordinates follow tinyobjloader's number grammar (a missing or non-numeric
 * token is 0); lines end at \n, \r\n or \r. */
#define RT_OBJ_MAX_FACE_VERTICES 4096
int rt_obj_load(const char* path, rt_obj_mesh* out);
void rt_obj_free(rt_obj_mesh* mesh);

/* ---- render: replaces camera::render's pixel x sample loop + ray_color recursion
 * (camera.h:37-47, camera_cpu.h:8-26).  Renders the tiles of `shard` of
 * `num_shards` into out_sums (device, shard_tiles*64*3 values of the context
 * precision: float for F32, double for F64), each the SUM over spp samples of the
 * linear colour (the `pixel_color` of camera.h:40-44).  out_segments (device,
 * shard_tiles*64 uint32, may be NULL) receives per-pixel world.hit counts.  F64 sums are
 * the reference's: sequential fp64 additions in sample order.  F32 sums are exact sums of
 * the samples' fp32 radiance rounded to the grid 2^-28 (64-bit fixed point), rounded once
 * to float -- independent of how samples are split over waves, launches or GPUs, exact
 * while a pixel's sample radiances stay below 2^13 (non-finite sums give NaN / +-inf as
 * the reference's additions would).  Asynchronous
 * on `stream` (NULL: the context's own stream, created hipStreamNonBlocking, so it does
 * NOT wait for work on the legacy null stream: the caller orders the producers of
 * out_sums/out_segments before the call, or passes its own stream); rt_last_kernel_ms()
 * gives its kernel time once it has finished. */
int rt_shard_layout(int width, int height, int shard, int num_shards, rt_shard_info* info);
int rt_render(rt_ctx* ctx, const rt_camera* cam, int samples_per_pixel, int max_depth, int shard, int num_shards,
              void* out_sums, uint32_t* out_segments, void* stream);
int rt_last_kernel_ms(rt_ctx* ctx, float* ms);
/* Progressive / split rendering: samples [sample_begin, sample_begin + sample_count) of
 * every pixel of the shard.  accumulate = 1 continues the per-pixel sums (and world.hit
 * counts) already in out_sums / out_segments, so a frame rendered as several ranges is
 * bit-identical to one rt_render of all its samples.  F64 continues the values in
 * out_sums.  F32 continues the context's fixed-point sums of the last launches into this
 * same buffer (same shard layout; the context remembers the last 4 buffers) wherever
 * out_sums still holds what the last launch wrote there; for a buffer it holds no sums
 * for, or where the contents changed (e.g. freed and reallocated at the same address),
 * it starts from out_sums' float values.  spp > 8191 runs as consecutive launches
 * (rt_last_kernel_ms covers all of them).  (The role the
 * reference's interactive Vulkan frame loop would play, graphical_environment_vulkan.cpp
 * :208-225, as plain device accumulation.) */
int rt_render_range(rt_ctx* ctx, const rt_camera* cam, int sample_begin, int sample_count, int max_depth,
                    int shard, int num_shards, int accumulate, void* out_sums, uint32_t* out_segments, void* stream);

/* Scatter num_shards stacked shard buffers (shard s at s*max_shard_tiles*64*3) into a
 * row-major W*H*3 frame (device, context precision). */
int rt_unshard(rt_ctx* ctx, const void* gathered, int width, int height, int num_shards, void* frame,
               void* stream);
/* write_color (color.h:14-35) on the device: sums -> /spp -> sqrt -> clamp(0,0.999) ->
 * int(256 x).  rgb: W*H*3 int32 (device) -- int32 because the reference prints
 * static_cast<int> and a NaN sum prints INT_MIN. */
int rt_quantize(rt_ctx* ctx, const void* frame, int width, int height, int samples_per_pixel, int32_t* rgb,
                void* stream);

/* write_color straight to bytes, fused with the un-interleave: num_shards stacked shard
 * buffers (as rt_unshard) -> row-major W*H*3 uint8 (device).  A quarter of rt_quantize's
 * int32 frame, so the device->host copy of a frame is 6.2 MB at 1080p.  A NaN sum
 * (which the reference prints as static_cast<int>(NaN)) gives 0. */
int rt_finish_frame_u8(rt_ctx* ctx, const void* gathered, int width, int height, int num_shards,
                       int samples_per_pixel, uint8_t* rgb8, void* stream);
/* Page-locked host memory (hipHostMalloc): device->host copies into it run at the full
 * link rate and asynchronously.  rt_host_free releases it. */
void* rt_host_alloc(size_t bytes);
void rt_host_free(void* p);

/* Whole frame on this context's GPU, 8-bit host out (the camera::render output path):
 * render, rt_finish_frame_u8 and the copy into rgb8_host (W*H*3 bytes; copied directly
 * when it is rt_host_alloc memory, else through the context's pinned staging buffer).
 * Synchronous. */
int rt_render_frame_u8(rt_ctx* ctx, const rt_camera* cam, int samples_per_pixel, int max_depth, uint8_t* rgb8_host);

/* ---- RCCL: the gather of finished shards to rank 0 over xGMI.
 * One process per GPU: rank 0 makes an id with rt_comm_unique_id, every rank receives it
 * by any channel (a file, a socket, torch.distributed's store) and calls
 * rt_comm_init_rank (non-blocking ncclCommInitRankConfig, polled): a rank whose peers do
 * not all join within the timeout (RT_COMM_INIT_TIMEOUT_MS, or the _timeout variant's)
 * gets RT_ERR_COMM and the half-built communicator is aborted, so a failure on one rank
 * cannot leave the others blocked.  One process driving several GPUs:
 * rt_comm_init_all (ncclCommInitAll) gives context r rank r.  RCCL errors come back as
 * RT_ERR_COMM with ncclGetErrorString in rt_last_error (e.g. two ranks on one GPU). */
#define RT_COMM_ID_BYTES 128
#define RT_COMM_INIT_TIMEOUT_MS 120000
int rt_comm_unique_id(char id[RT_COMM_ID_BYTES]);
int rt_comm_init_rank(rt_ctx* ctx, int nranks, int rank, const char id[RT_COMM_ID_BYTES]);
int rt_comm_init_rank_timeout(rt_ctx* ctx, int nranks, int rank, const char id[RT_COMM_ID_BYTES], int timeout_ms);
int rt_comm_init_all(rt_ctx** ctxs, int num_ctxs);
int rt_comm_rank(rt_ctx* ctx, int* rank, int* nranks);   /* RT_ERR_INVALID without a communicator */
int rt_comm_destroy(rt_ctx* ctx);
/* ncclGather of this rank's shard buffer (max_shard_tiles*64*3 values of the context
 * precision for a W x H frame split over nranks) into `gathered` on rank 0 (nranks times
 * that, shard r at offset r; may be NULL on other ranks), enqueued on `stream` after the
 * work already there (the render).  Asynchronous. */
int rt_gather_shards(rt_ctx* ctx, const void* shard, void* gathered, int width, int height, void* stream);

/* Whole frame across several contexts in ONE process (e.g. one per GPU of the node, each
 * with the same scene uploaded): context r renders shard r of n on its own stream; the
 * shards are copied to ctxs[0]'s device (peer copies over xGMI when the devices differ),
 * un-interleaved and quantised there.  Same pixels as rt_render_frame on one context.
 * With communicators from rt_comm_init_all the shards travel by one grouped ncclGather;
 * otherwise by peer copies (hipMemcpyPeerAsync).  Synchronous; outputs as rt_render_frame.  (The per-process alternative for clusters of
 * ranks is rt_render + an RCCL gather, raytracingproject_amd/distributed.py.) */
int rt_render_frame_multi(rt_ctx** ctxs, int num_ctxs, const rt_camera* cam, int samples_per_pixel, int max_depth,
                          void* sums_host, int32_t* rgb_host);

/* Whole frame on this context's GPU, host in / host out (the drop-in camera::render
 * path).  sums_host: W*H*3 of the context precision (may be NULL); rgb_host: W*H*3 int32
 * (may be NULL); segments_host: W*H uint32 (may be NULL).  Synchronous. */
int rt_render_frame(rt_ctx* ctx, const rt_camera* cam, int samples_per_pixel, int max_depth, void* sums_host,
                    int32_t* rgb_host, uint32_t* segments_host);

/* One ray on an explicit tape of uniforms, fp64, reference order: the drop-in for a
 * direct ray_color(r, depth, world) call (camera_cpu.h:8, tests.cpp:42) that must keep
 * consuming the caller's sequential random stream.  ray = {orig[3], dir[3], time}.
 * *used = uniforms consumed (the caller advances its stream by that much); if *used
 * exceeds tape_len the result is invalid and the caller retries with a longer tape. */
int rt_trace_tape(rt_ctx* ctx, const double ray[7], int depth, const double* tape, int tape_len, double out[3],
                  int* used);

/* Batched world.hit: hittable::hit (hittable.h:28) of the uploaded world -- the closest
 * hit in (0.001, inf), hittable_list.h:25-39 / bvh.h:16-24 -- for n rays in one launch,
 * with each closest hit's hit_record (hittable.h:7-22).  rays: device memory, n records
 * of 7 values of the context precision {origin xyz, direction xyz, time}; hits: device
 * memory, n rt_hit.  id: the input index of the sphere hit (as given to
 * rt_upload_scene[_ex]), num_spheres + the triangle's input index, or -1 (miss: the other
 * fields are 0); mat: its material index.  fp64 contexts compute with the reference's
 * operations (sphere.h:30-57) and order.  Asynchronous on `stream` (NULL: the context's);
 * rt_last_kernel_ms times it. */
typedef struct {
    double t;
    double p[3], normal[3];
    int32_t id, front_face, mat, pad;
} rt_hit;
int rt_trace_rays(rt_ctx* ctx, const void* rays, int num_rays, rt_hit* hits, void* stream);
/* ABI 12: rt_trace_rays for rays that may name the primitive they start on.  origin_ids:
 * device memory, num_rays values in rt_hit.id's numbering (the input index of a sphere,
 * num_spheres + the input index of a triangle) or -1 for none; any other value counts as -1;
 * NULL: all -1, which is rt_trace_rays.
 * fp32 contexts treat primitive origin_ids[i] as the render kernels treat a scattered ray's
 * previous hit.  The contract: the origin is taken to lie ON that primitive (a hit point of
 * it, rounded to fp32).  One root of a sphere it starts on is then the origin itself, which
 * fp32 cannot tell from a hit just above tmin = 0.001 when the direction is short; so that
 * sphere offers only its other root, t = -2 (o - c).d / d.d -- a hit where it lies in
 * (0.001, inf): the far side of a sphere the ray enters, nothing for a ray that leaves it --
 * and that triangle is skipped.  An origin that is not on the named primitive gets that
 * same treatment, which is then not the closest hit.
 * fp64 contexts ignore the ids: the reference has no such notion (sphere.h:41-46 tests both
 * roots against tmin), and the records equal rt_trace_rays' bit for bit. */
int rt_trace_rays_from(rt_ctx* ctx, const void* rays, int num_rays, const int32_t* origin_ids, rt_hit* hits,
                       void* stream);
/* Batched any-hit visibility: hittable::hit's return value (hittable.h:28) for num_rays rays,
 * each over its own interval: occluded[i] = 1 where some primitive of the uploaded world has a
 * root t with tmin_i < t < tmax_i (interval::surrounds, interval.h:33-35), else 0.  No record:
 * shadow rays, ambient occlusion, line of sight, "anything within distance L".
 * rays: as for rt_trace_rays.  intervals: device memory, num_rays records {tmin, tmax} of the
 * context precision; NULL: (0.001, +inf) for every ray.  occluded: device memory, num_rays
 * bytes, each written 0 or 1.  tmax = +inf is valid; so is a negative or -inf tmin (the
 * reference's interval has no sign rule: roots behind the origin count where the interval
 * admits them).  tmin >= tmax, or a NaN end, gives 0 and is no error.  A ray that starts on a
 * surface passes a tmin; there are no origin ids here.
 * fp64 contexts return the reference's boolean exactly (sphere.h:30-48's roots, both tested);
 * fp32 contexts run the primitive tests of rt_trace_rays, so with intervals = NULL the answer
 * is (rt_hit.id != -1) ray for ray.  The traversal stops at a ray's first hit, orders nothing
 * and writes one byte, where rt_trace_rays finds the closest hit and writes 72.
 * Errors as rt_trace_rays (RT_ERR_NO_SCENE before an upload, RT_ERR_INVALID for num_rays < 0
 * or a NULL rays / occluded with num_rays > 0, RT_ERR_LIMIT past 160 KiB of LDS); num_rays ==
 * 0 is a no-op.  Asynchronous on `stream` (NULL: the context's); rt_last_kernel_ms times it.
 * Added to ABI 12 without a version bump: a new entry point changes no existing one, so every
 * caller built against 12 keeps working, and one that needs rt_occluded looks the symbol up. */
int rt_occluded(rt_ctx* ctx, const void* rays, int num_rays, const void* intervals, uint8_t* occluded,
                void* stream);
/* Batched ray_color (camera_cpu.h:8-26) over caller-supplied rays: radiance[i] =
 * ray_color(rays[i], max_depth, world), one value per ray.  Nothing is summed and nothing is
 * rounded to the frame's fixed-point grid: the caller reduces.  A custom camera (orthographic,
 * fisheye, a light probe, a sampler of the caller's own, a subset of pixels) is the caller's
 * rays + the caller's (pixel, sample) keys + a sum.
 * rays: as for rt_trace_rays.  keys: device memory, one rt_path_key per ray, or NULL for
 * {i, 0, 0, 0} on ray i.  Ray i draws from the RT-CRNG-1 stream key(seed, pixel, sample)
 * (oracle/rt_rng_spec.h rtspec_path_key, seed: rt_set_seed's), starting at draw number
 * first_draw -- the draws a camera spent on the ray before ray_color, e.g. rt_camera's 2 for the
 * pixel square, 2 per defocus-disk candidate and 1 for the time.  pad is ignored.  The key is the only per-ray
 * state: two rays with equal key and equal values get equal results, and the output is the
 * same bit for bit for any order, grid size or split of the batch.
 * radiance: device memory, num_rays x 3 values of the context precision.  segments: NULL, or
 * device memory for num_rays counts of that ray's world.hit calls (what rt_render's
 * out_segments sums per pixel).  max_depth <= 0: every radiance and count is 0, no path is
 * traced (camera_cpu.h:9-10).
 * fp64 contexts return the reference's ray_color bit for bit: its sphere and triangle
 * arithmetic, attenuations multiplied innermost-first (camera_cpu.h:19), no self-primitive
 * rule; max_depth > 64 is RT_ERR_LIMIT as in rt_render_range.  fp32 contexts keep the fp32
 * render kernels' arithmetic: the throughput is multiplied bounce by bounce, and every
 * scattered segment treats the primitive it starts on as rt_trace_rays_from does; the caller's
 * first segment names none (there are no origin ids here).
 * Errors as rt_trace_rays (RT_ERR_NO_SCENE before an upload, RT_ERR_INVALID for num_rays < 0
 * or a NULL rays / radiance with num_rays > 0, RT_ERR_LIMIT past 160 KiB of LDS); num_rays ==
 * 0 is a no-op.  A non-finite ray component gives an unspecified value for that ray only; every
 * path ends (at most max_depth segments).  Asynchronous on `stream` (NULL: the context's);
 * rt_last_kernel_ms times it.  Calls on one context share a device counter: enqueue them on
 * one stream, or order them.  Added to ABI 12 without a version bump, as rt_occluded was. */
typedef struct {
    uint32_t pixel, sample, first_draw, pad;
} rt_path_key;
int rt_radiance_rays(rt_ctx* ctx, const void* rays, int num_rays, const rt_path_key* keys, int max_depth,
                     void* radiance, uint32_t* segments, void* stream);
/* Sparse rendering: the sums rt_render / rt_render_range write, for a device list of pixel
 * sample jobs instead of a whole shard of tiles with one sample range -- adaptive sampling, crop
 * windows, re-rendering a dirty region, sparse previews, per-pixel budgets.
 * jobs: device memory, num_jobs records.  pixel = j * image_width + i (row j, column i: the key
 * rt_render gives that pixel's RNG streams); the job's samples are [sample_begin, sample_begin +
 * sample_count); pad is ignored.  Jobs are independent: a pixel may appear in several, with
 * overlapping ranges.  A job with sample_count == 0 or pixel >= width * height contributes
 * nothing -- its outputs are 0, or untouched when accumulate is 1 -- and is no error.  The flat
 * sample list is job 0's samples in order, then job 1's, ...; T is the valid jobs' total count.
 * out_sums: device memory, num_jobs x 3 values of the context precision; out_segments: NULL, or
 * device memory for num_jobs world.hit counts of that job's samples.
 * fp64 contexts: out = start + L(s0) + L(s0 + 1) + ..., sequential fp64 additions in sample
 * order, start = 0.0 or (accumulate = 1) the value already in out_sums[job]; L is the
 * reference's ray_color of get_ray(i, j) on the RT-CRNG-1 stream key(seed, pixel, sample).  A
 * job {p, 0, spp} is rt_render's sum of pixel p bit for bit, and {p, 0, a} followed by {p, a, b}
 * with accumulate equals {p, 0, a + b}.
 * fp32 contexts: the fp32 render kernels' rule.  Each sample channel is rounded to
 * rintf(L 2^19), the roundings are summed exactly as integers S, and out =
 * (float)((double)(S 2^9) 2^-28) -- the same bits for any order or split; a non-finite or
 * overflowing sample makes the channel NaN or +-inf as in rt_render.  accumulate = 1 starts from
 * rint((double)out 2^28) (non-finite values as NaN / +-inf), which is what rt_render_range does
 * for a buffer the context holds no sums for; the context's memory of rt_render_range's output
 * buffers is neither used nor disturbed.  L is the fp32 render kernels' arithmetic (the camera
 * vectors rounded once, the throughput multiplied bounce by bounce, the self-primitive rule on
 * scattered segments only).  Out-of-range radiance aside, a job {p, s, n} is
 * rt_render_range(s, n) at pixel p bit for bit.
 * out_segments is overwritten, or added to with accumulate = 1.
 * The sphere grid is walked where rt_render would walk it for this camera, else the sphere tree
 * (rt_pixels_plan says which, and when; rt_render_pixels_moments: rt_pixels_plan_call, the grid in
 * fp64 contexts only); the sums are the same bits either way.  fp64 passes: each sample is
 * stored as a 28-byte record (3 doubles and one uint32) before the ordered reduction, and one
 * pass holds floor(rt_tuning.sample_buffer_mb 2^20 / 28) samples of the flat list; a job that
 * straddles a pass boundary continues in the next pass.
 * Errors: RT_ERR_NO_SCENE before an upload; RT_ERR_INVALID for a bad camera, num_jobs < 0, or a
 * NULL jobs / out_sums with num_jobs > 0; RT_ERR_LIMIT for fp64 max_depth > 64, past 160 KiB of
 * LDS, or T > 2^31 - 1 (the scan is 64-bit).  num_jobs == 0 is a no-op.  max_depth <= 0: sums and
 * counts are 0 (untouched with accumulate), no path kernel runs.
 * T lives on the device and the host needs it to size the passes and check the limit: the call
 * SYNCHRONISES on the stream once, after the scan of the jobs' counts, with an 8-byte copy;
 * everything after that is asynchronous on `stream` (NULL: the context's).  rt_last_kernel_ms
 * covers the whole call, scan included.  Calls on one context share device scratch: enqueue
 * them on one stream, or order them.  Cost: one search of the job list per sample; in fp32 all
 * samples of a job add to the same three words with atomics, and in fp64 one thread adds a job's
 * samples in order, so split a job of 10^5 samples or more into several jobs of that pixel.
 * Added to ABI 12 without a version bump, as rt_occluded. */
typedef struct {
    uint32_t pixel, sample_begin, sample_count, pad;
} rt_pixel_job;
int rt_render_pixels(rt_ctx* ctx, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, int max_depth,
                     int accumulate, void* out_sums, uint32_t* out_segments, void* stream);
/* rt_render_pixels with a second output, the per-job second moment -- what an adaptive sampler
 * needs to estimate a pixel's variance on the device.  The contract is rt_render_pixels': jobs,
 * flat sample list, T, the fp64 passes, the single synchronisation, the errors, max_depth <= 0,
 * invalid and empty jobs; out_sums and out_segments are bit for bit what rt_render_pixels writes
 * for the same arguments.
 * out_sumsq: device memory, num_jobs x 3 values of the context precision: per channel the sum of
 * squares of the job's per-sample radiance.  Required: NULL with num_jobs > 0 is RT_ERR_INVALID.
 * A job without samples gets 0, or is left untouched with accumulate = 1.
 * fp64 contexts: sumsq = start + L0 L0 + L1 L1 + ..., in sample order; each product is rounded to
 * double on its own (never fused into the addition), the additions are sequential; start = 0.0,
 * or (accumulate = 1) the value already in out_sumsq.  A job that straddles a pass continues
 * out_sumsq as it continues out_sums, so {p, 0, a} then {p, a, b} with accumulate equals
 * {p, 0, a + b} in both outputs.
 * fp32 contexts: per sample channel r = rintf(L 2^19), the integer-valued float the sum rule
 * rounds to.  r == 0 adds nothing; a NaN r makes the channel's sumsq NaN; |r| >= 2^32 (a sample
 * at or beyond the documented exact range 2^13, or an infinity) makes it +inf (NaN wins over
 * +inf); otherwise r r is an exact integer below 2^64 and is added exactly, in any order: two
 * 64-bit words per channel, S_lo += r r & 0xffffffff and S_hi += r r >> 32, neither of which can
 * overflow within 2^31 samples, and out_sumsq = (float)(((double)S_hi 2^32 + (double)S_lo) 2^-38),
 * IEEE operations in that order.  accumulate = 1 starts from X = rint((double)out_sumsq 2^38)
 * for 0 <= out_sumsq < 2^57 (S_hi = X >> 32, S_lo = X & 0xffffffff); a negative or NaN start gives
 * NaN, one >= 2^57 or +inf gives +inf.  The sums' own rule and flags are untouched.
 * Cost: fp32 adds up to six atomics per sample to rt_render_pixels' three; fp64 adds three
 * multiplications per sample to the ordered reduction.  rt_tuning.grid_workgroups > 0 caps the
 * path kernel's grid here (rt_render_pixels ignores it); the outputs do not depend on it.
 * Added to ABI 12 without a version bump. */
int rt_render_pixels_moments(rt_ctx* ctx, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, int max_depth,
                             int accumulate, void* out_sums, void* out_sumsq, uint32_t* out_segments, void* stream);
/* One round of an adaptive sampler, on the device: rewrites jobs[k] in place for the next
 * rt_render_pixels_moments call from the sums and second moments the list has accumulated.  The
 * list keeps its length and slot order, so out_sums, out_sumsq and out_segments stay valid as
 * accumulators (accumulate = 1); a converged slot gets sample_count = 0, which rt_render_pixels*
 * leaves alone.  sums, sumsq: num_jobs x 3 values of the context precision (device).
 * All arithmetic is fp64 whatever the context precision (floats convert exactly); every
 * operation is rounded once, in the written order, nothing is fused.  With n = sample_begin +
 * sample_count (64-bit), s_c = sums[k][c], q_c = sumsq[k][c]:
 *   n >= max_samples: next = 0;  else n < min_samples: next = min_samples - n;
 *   else any s_c or q_c non-finite: not converged;
 *   else m_c = s_c / n, d_c = q_c - s_c m_c, v_c = d_c > 0 ? d_c / (n - 1) : 0,
 *        e2 = ((v_0 + v_1) + v_2) / (3 n), m = ((m_0 + m_1) + m_2) / 3, a = max(|m|, abs_floor),
 *        t = rel_error a; converged iff e2 <= t t  (the squared standard error of the mean of the
 *        channel average against a relative tolerance);
 *   not converged: next = min(n, max_step, max_samples - n) (doubling, capped); converged: 0.
 *   jobs[k] = {pixel, (uint32)n, next, 0}.
 * stats: two device uint64, overwritten: {jobs with next > 0, the sum of next}.
 * Errors: RT_ERR_INVALID for a NULL pointer with num_jobs > 0, num_jobs < 0, min_samples < 2,
 * min_samples > max_samples, max_samples > 2^31 - 1, max_step == 0, a negative or non-finite
 * rel_error or abs_floor.  num_jobs == 0 is a no-op that zeroes stats.  Needs no scene;
 * asynchronous on `stream` (NULL: the context's); rt_last_kernel_ms times it.
 * Not done here: compacting the job list (converged slots stay, at 16 bytes and one scan element
 * each), a fused finish kernel for a non-uniform n (divide sums by n yourself; rt_quantize(mean,
 * spp = 1) quantises), any use from rt_render.
 * Added to ABI 12 without a version bump. */
typedef struct {
    double rel_error, abs_floor;
    uint32_t min_samples, max_samples, max_step, pad;
} rt_adaptive_params;
int rt_refine_jobs(rt_ctx* ctx, rt_pixel_job* jobs, int num_jobs, const void* sums, const void* sumsq,
                   const rt_adaptive_params* params, uint64_t* stats, void* stream);
/* The camera's rays on the device: camera::get_ray (camera.h:87-113) for every sample of a job
 * list (jobs, flat sample list and T as for rt_render_pixels).  For flat sample q: rays[q] = the
 * ray, 7 values of the context precision {origin xyz, direction xyz, time}, in the render
 * kernels' arithmetic of that precision; keys[q] = {pixel, sample, first_draw, 0} with
 * first_draw the draws get_ray spent (2 for the pixel square, 2 per defocus-disk candidate
 * including the accepted one when defocus_angle > 0, 1 for the time) -- ready for
 * rt_radiance_rays, rt_trace_rays or rt_occluded; ray_job[q] = the job's index (ray_job may be
 * NULL).  rt_radiance_rays(rays, keys), summed per job by rt_render_pixels' rules, equals
 * rt_render_pixels.  Needs no scene: only the camera and the context's seed.
 * rays, keys, ray_job: device memory for max_rays records.  *num_rays (host memory, may be NULL)
 * receives T; T > max_rays is RT_ERR_INVALID with nothing written beyond *num_rays (call with
 * max_rays = 0 to size the buffers).  Other errors: RT_ERR_INVALID for a bad camera, num_jobs <
 * 0, or a NULL jobs / rays / keys with num_jobs > 0; RT_ERR_LIMIT for T > 2^31 - 1.  num_jobs ==
 * 0 sets *num_rays = 0 and does nothing else.  Synchronises once after the scan, as
 * rt_render_pixels; the rays are written asynchronously on `stream`; rt_last_kernel_ms covers
 * the call. */
int rt_camera_rays(rt_ctx* ctx, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs, void* rays,
                   rt_path_key* keys, int32_t* ray_job, int64_t max_rays, int64_t* num_rays, void* stream);
/* First-hit auxiliary outputs (AOVs) per job -- the guide images a denoiser asks for: albedo,
 * normal, depth, primitive id and sky coverage -- reduced on the device without writing a ray or a
 * hit record to memory.  jobs, valid and invalid jobs, the flat sample list, T, the scan and its
 * single 8-byte synchronisation, the stream rules and rt_last_kernel_ms are rt_render_pixels'.
 * Only the first segment is traced (there is no max_depth), and no RNG draw is spent beyond
 * get_ray's.
 * Per sample, r is the camera ray rt_camera_rays writes for it and h the rt_hit rt_trace_rays
 * returns for r: the tree, the same traversal flags, no origin id -- the same bits.  (Over the
 * sphere grid the record is the same too -- tests/test_query_grid.py held a grid build of this
 * call to it -- but the grid was not faster here, so the call keeps the tree:
 * rt_pixels_plan_call(RT_QUERY_AOV).)
 * out: host struct of device pointers, each num_jobs records; a NULL member is skipped.
 *   hits    the number of the job's samples with h.id != -1; overwritten, or added to with
 *           accumulate = 1.  hits / sample_count is the coverage (1 - sky).
 *   albedo  x 3, context precision: per sample the material's albedo in the context precision
 *           (fp32: (float)rt_material.albedo) for Lambertian and metal, (1, 1, 1) -- its scatter
 *           attenuation -- for a dielectric, 0 for a miss; summed over the job's samples.
 *   normal  x 3, context precision: per sample h.normal, the face-oriented normal of the record
 *           (not renormalised), 0 for a miss; summed over the job's samples.
 *   depth, id  the nearest hit of the job: the sample with the smallest h.t, among equal t the
 *           smallest h.id; depth = its h.t (context precision), id = its h.id (rt_hit.id's
 *           numbering).  h.t is the ray parameter, and the camera's direction reaches the focus
 *           plane at t = 1, so depth * focus_dist is the planar depth for a pinhole camera.  A job
 *           with no hit gets depth = +inf, id = -1.  If only one of the two is given the other is
 *           simply not written.
 * Sum rule (albedo, normal): exactly rt_render_pixels', with the per-sample value in place of L.
 * fp64 adds sequentially in sample order from 0, or from the buffer with accumulate = 1 (a miss
 * adds 0.0); fp32 takes rintf(v 2^19), sums exactly as integers in units of 2^-28 and rounds once,
 * with the same NaN / +-inf flags, and accumulate = 1 starts from rint((double)out 2^28) -- the
 * exact earlier sum wherever out, a float, holds it: a sum of multiples of 2^-19 below 32 in
 * magnitude, so {p, 0, a} then {p, a, b} equals {p, 0, a + b} bit for bit for a <= 31.
 * Nearest hit: fp32 keeps one 64-bit word per job, (float bits of t) << 32 | (uint32_t)id, combined
 * by unsigned minimum (t > 0.001, so bit order is numeric order); fp64 keeps (t, id) under the same
 * comparison in the ordered reduction.  accumulate = 1 continues from what depth and id hold -- the
 * caller's contract is that they hold an earlier call's output or (+inf, -1) -- and a missing one
 * counts as +inf / -1.
 * A job without samples (sample_count == 0 or pixel >= width * height) gets (0, 0, +inf, -1, 0),
 * or is left untouched with accumulate = 1.
 * fp64 passes: each sample is stored as a 60-byte record (7 doubles and one int32) before the
 * ordered reduction; a pass holds floor(rt_tuning.sample_buffer_mb 2^20 / 60) samples, and a job
 * that straddles a pass boundary continues in the next.
 * fp32: a wave's lanes hold consecutive samples, and the lanes of one job are combined within the
 * wave before one lane issues that job's atomics.  The environment's RT_AOV_COMBINE=0 at rt_create
 * issues one set of atomics per sample instead; the outputs are the same bits.
 * Errors: rt_render_pixels' (RT_ERR_NO_SCENE before an upload; RT_ERR_INVALID for a bad camera,
 * num_jobs < 0 or a NULL jobs with num_jobs > 0; RT_ERR_LIMIT past 160 KiB of LDS or T > 2^31 - 1),
 * and RT_ERR_INVALID for a NULL out with num_jobs > 0 or an out whose five members are all NULL.
 * num_jobs == 0 is a no-op.  Shares rt_render_pixels' device scratch: same stream, or ordered.
 * Not done here: coherent per-tile batches of the camera rays; the sphere grid (built and
 * measured: 1.09x the tree's time in fp32, within the spreads in fp64 at 2 spp, so not kept); a
 * sky-coloured albedo for misses (blend with the coverage yourself).
 * Added to ABI 12 without a version bump, as rt_occluded. */
typedef struct {
    void*     albedo;   /* num_jobs x 3, context precision, or NULL */
    void*     normal;   /* num_jobs x 3, context precision, or NULL */
    void*     depth;    /* num_jobs,     context precision, or NULL */
    int32_t*  id;       /* num_jobs, or NULL */
    uint32_t* hits;     /* num_jobs, or NULL */
} rt_aov_buffers;
int rt_render_pixels_aov(rt_ctx* ctx, const rt_camera* cam, const rt_pixel_job* jobs, int num_jobs,
                         int accumulate, const rt_aov_buffers* out, void* stream);
/* The consumer of the calls above: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010;
 * the spatial half of SVGF, Schied et al. 2017) over per-pixel sums, second moments and first-hit
 * guides, on the device, in the context precision.  A 5x5 B3-spline kernel dilated by 1, 2, 4, ...
 * whose taps are stopped by normal, depth and a variance-scaled luminance difference.  With
 * iterations = 0 and no guides it is the finish of a non-uniform sample count: out = sums / n.
 * The rule uses IEEE + - x / sqrt and comparisons only -- no exp, no pow, nothing fused -- so it is
 * bit for bit reproducible in both precisions (tests/denoise_ref.py restates it in numpy).
 *
 * Layout and arguments.  All images are row-major width x height, pixel p = y width + x: the order
 * of a full-frame job list (jobs[k].pixel = k), so the outputs of rt_render_pixels[_moments] and
 * rt_render_pixels_aov plug in unchanged, and rt_unshard's frame does too.  T is the context
 * precision; every operation below is done in T and rounded once, in the written order, nothing
 * contracted; the double parameters are converted to T once.  max(a, b) is a > b ? a : b and
 * min(a, b) is a < b ? a : b.
 *   sums (x 3, required), sumsq (x 3, may be NULL): what rt_render_pixels_moments writes.
 *   counts: the per-pixel n (uint32); NULL: every n = samples.
 *   guides: may be NULL, and so may each member; id is ignored; albedo needs hits and
 *     guide_samples >= 1.  albedo, normal and hits are the per-job SUMS of guide_samples samples,
 *     exactly as rt_render_pixels_aov writes them.
 *   params: NULL means rt_denoise_default_params'.
 *   out (x 3, required; may be the sums buffer itself), out_variance (x 1, may be NULL).
 * Prepare, per pixel:
 *   nT = (T)n;  m_c = n > 0 ? s_c / nT : 0.
 *   With albedo a_c = max((albedo_c + (T)(guide_samples - hits)) / (T)guide_samples, 1/64) -- a miss
 *   counts as white; without, a_c = 1.  c_c = m_c / a_c;  L = ((c_0 + c_1) + c_2) / 3.
 *   Variance V with sumsq and n >= 2: d_c = q_c - s_c m_c, v_c = d_c > 0 ? d_c / (T)(n - 1) : 0,
 *   v'_c = v_c / (a_c a_c), V = ((v'_0 + v'_1) + v'_2) / ((T)3 nT) -- rt_refine_jobs' e2; n < 2: V = 0.
 *   Without sumsq: over the in-image cells of the 3x3 window around p (k cells, row-major order, sums
 *   from 0) mu = (sum of L) / k, mu2 = (sum of L L) / k, V = max(mu2 - mu mu, 0).
 *   Normal: d = (N_0 N_0 + N_1 N_1) + N_2 N_2, n^ = d > 0 ? N / sqrt(d) : 0; no normal guide: n^ = 0.
 *   Depth: z as given, +inf for sky; no depth guide: z = 0.
 * Pass i = 0 .. iterations - 1, s = 2^i, per pixel p = (x, y), reading pass i - 1's c, V and L:
 *   V~ = (sum of (g(dx) g(dy)) V_q) / (sum of g(dx) g(dy)) over the in-image cells of the undilated
 *   3x3 window in row-major order, g = (1/4, 1/2, 1/4);  den = sigma_lum sqrt(V~) + lum_eps.
 *   Taps dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner), q = (x + dx s, y + dy s); a tap outside
 *   the image is skipped.  k = h(dx) h(dy), h = (1/16, 1/4, 3/8, 1/4, 1/16): exact in binary.
 *   Centre tap: w = k.  Other taps: w = (k w_n) e8(x_z + x_l), where
 *     w_n: 1 if n^_p and n^_q are both zero (so always without a normal guide); else
 *          t = max((n^_p.x n^_q.x + n^_p.y n^_q.y) + n^_p.z n^_q.z, 0), squared normal_log2_power times;
 *     x_z: 0 if z_p == z_q; otherwise, if either is infinite, the tap's w = 0; otherwise
 *          |z_p - z_q| / (sigma_depth min(z_p, z_q));
 *     x_l: |L_p - L_q| / den;
 *     e8(x) = u^8 by three squarings of u = max(1 - x 0.125, 0): a compactly supported stand-in
 *          for exp(-x) that needs only exact operations.
 *   Accumulators start from 0 and add in tap order: Sw += w, Sc_c += w c_q,c, Sv += (w w) V_q.
 *   Then c'_p = Sc / Sw, V'_p = Sv / (Sw Sw), and L is recomputed from c'.  Sw >= 9/64 always.
 * Finish: out_c = c_c a_c; out_variance = V, the variance of the demodulated channel average.
 *
 * A non-finite input makes the outputs within its taps' reach unspecified; it is never a fault.
 * Needs no scene.  Asynchronous on `stream` (NULL: the context's); no synchronisation of its own;
 * rt_last_kernel_ms covers the whole call.  Scratch -- two ping-pong record images and one guide
 * image, 4 T per pixel each -- is owned by the context and grown on demand: calls on one context
 * must use one stream or be ordered.
 * Errors: RT_ERR_INVALID for a NULL ctx, sums or out; width or height < 1 or width height > 2^31 -
 * 1; counts NULL with samples < 1; albedo without hits or with guide_samples < 1; a parameter
 * outside the ranges below -- nothing is written.  A failed allocation is RT_ERR_HIP.
 * Not done here: temporal accumulation, firefly clamping, inpainting of n = 0 pixels, denoising
 * rt_render's sharded buffers without rt_unshard.
 * Added to ABI 12 without a version bump, as rt_occluded was. */
typedef struct {
    int32_t iterations;          /* 0..8; a-trous passes, step 2^i in pass i */
    int32_t normal_log2_power;   /* 0..10; the normal weight is (n_p.n_q)^(2^k) by k squarings */
    double  sigma_depth;         /* > 0, finite: relative depth difference that counts as 1 */
    double  sigma_lum;           /* >= 0, finite: luminance difference in standard deviations */
    double  lum_eps;             /* > 0, finite */
} rt_denoise_params;
/* The defaults: iterations 5, normal_log2_power 7, sigma_depth 0.05, sigma_lum 4, lum_eps 1e-6. */
int rt_denoise_default_params(rt_denoise_params* p);
int rt_denoise(rt_ctx* ctx, int width, int height,
               const void* sums, const void* sumsq, const uint32_t* counts, int samples,
               const rt_aov_buffers* guides, int guide_samples,
               const rt_denoise_params* params, void* out, void* out_variance, void* stream);
/* rt_trace_rays, instrumented (fp32 sphere scenes; synchronous): counters = {node-loop wave
 * iterations, their active lanes, sphere-loop wave iterations, their active lanes}. */
int rt_trace_rays_diag(rt_ctx* ctx, const void* rays, int num_rays, rt_hit* hits, uint64_t counters[4]);

/* ---- diagnostics (not on the render path) ---------------------------------------
 * Whole frame with the instrumented build of the persistent fp32 kernel (block 512, the
 * context's traversal flags 0, 1 or 8; spp <= 8191): counters[16] receives
 *  0 bounce-loop wave iterations, 1 active lanes summed over them,
 *  2 inner-node-loop wave iterations, 3 their active lanes, 4 leaf-sphere-loop wave
 *  iterations, 5 their active lanes, 6/7 shader cycles (s_memtime) summed over bounce
 *  iterations in closest-hit / shade+scatter, 8 cycles in the pixel-chunk hand-out and
 *  flush loop, 9 whole-kernel cycles, both summed over waves, 10 world.hit calls,
 *  11 pixel-chunk flushes, 12-14 the K-rays-per-lane model: wave step iterations (node
 *  visits + sphere tests of the slowest active lane) summed per closest_hit call (K=1),
 *  per pair (K=2) and per four consecutive calls (K=4). */
int rt_render_diag(rt_ctx* ctx, const rt_camera* cam, int samples_per_pixel, int max_depth, uint64_t counters[16]);
/* The same with n <= RT_DIAG_SLOTS counters.  The coherent-primary kernel (RT_TRAV_COH)
 * fills 0-15 as {0 bounce-loop wave iterations, 1 their active lanes, 2-5 as above,
 * 6 cycles in closest-hit (secondaries), 7 shade rounds, 8 camera-ray batches, 9 whole
 * kernel, 10 world.hit calls (secondaries), 11 finished paths, 12 batches, 13 batch
 * traversal wave iterations, 14 their active lanes, 15 primary hits popped} and 16-23
 * with each wave's timeline in s_memrealtime ticks (100 MHz): 16 latest wave end,
 * 17 ~earliest wave start (bitwise NOT), 18 sum over waves of (end - queue found dry),
 * 19 sum of (queue found dry - start), 20 ~earliest dry (NOT), 21 latest dry, 22 waves,
 * 23 bounce-loop wave iterations after the queue ran dry (the drain), and 24-27 with the
 * framebuffer traffic: 24 samples finished into their item's LDS sums, 25 samples
 * flushed straight to HBM (their item was no longer the wave's current one, or a value
 * outside [0, 1]), 26 item flushes (per pixel); mesh scenes add 27-30: 27 mesh-BVH node
 * wave iterations, 28 their active lanes, 29 triangle-test wave iterations, 30 their active
 * lanes.  The fp32 sphere-only kernels over the sphere grid, which have no mesh loops, fill
 * 27-29 with the primary-hit hand-over instead: 27 pop passes (shade rounds of a wave in which
 * at least one lane popped a FIFO entry), 28 the lanes that popped in them (equal to slot 15),
 * 29 primary hits adopted (kept by the waiting lane that traced them in the batch, see
 * RT_BATCH_ADOPT in INTEGRATION.md; never queued, so not in slot 15).  31: grid walks
 * suspended (the sphere-only kernel over the flat grid walk, see RT_GRID_SUSPEND in
 * INTEGRATION.md; 0 for every other kernel); a resumed walk counts no new world.hit call in
 * slot 10, though its trace counts in slots 0 and 1.  32-39 (the same sphere-only grid kernels;
 * 0 for every other kernel): the pop passes of slot 27 by the number of lanes that popped in
 * the pass -- 32: 1-2 lanes, 33: 3-6, 34: 7-16, 35: more than 16, for passes that do not
 * directly follow a batch in which a lane adopted its hit; 36-39: the same four buckets for
 * passes that directly follow such a batch in the same shade round.  The eight sum to slot 27.
 * The same kernels, per shade pass of a wave (one trip of the shade loop: sky finishes, pops,
 * one scatter pass): 30 shade passes, 40 those in which at least one lane flushed a finished
 * sample straight to HBM (slot 25's samples), 41 those whose scatter pass held both a metal and a
 * dielectric lane. */
enum { RT_DIAG_SLOTS = 42 };
int rt_render_diag_ex(rt_ctx* ctx, const rt_camera* cam, int samples_per_pixel, int max_depth, uint64_t* counters,
                      int n);

#ifdef __cplusplus
}
#endif
#endif
