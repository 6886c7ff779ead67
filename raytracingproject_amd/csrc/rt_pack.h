// rt_pack.h -- a scene's host-side packing: everything rt_upload_scene_ex computes before it
// touches the device (argument checks, the trees, the per-precision records, the sphere grid,
// rt_trace_rays' id map and its inverse, the walk's reach), and the reach test each launch makes against it.
// Host only, no HIP types: built with g++ under the sanitizers by tests/cpp/pack_driver.cpp.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_bvh.h"
#include "rt_scene.h"

namespace rtx {

// r06: where a launch's rays can start (grid_reach_ok): the box of the geometry a ray can
// leave from anywhere on it -- spheres outside the big class, triangles, and big spheres that
// refract or move -- and the static opaque big spheres (centre, radius), which a ray only
// reaches within its tangent distance
struct SceneReach {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    std::vector<std::array<double, 4>> big;
};

// No ray a launch from `cam` can produce starts beyond +-far_o (GridHdr::far_o) on any axis:
// the sphere grid's walk serves the launch.  (A scene without a grid: the caller's case.)
bool grid_reach_ok(const SceneReach& reach, float far_o, const rt_camera& cam);

struct PackedScene {
    bool f64 = false;
    bool gpu_build = false;            // the mesh tree is built on the device: mbvh, tf, td, tmeta stay empty
    BuiltBvh bvh;
    MeshBvh mbvh;
    std::vector<SphereF> sf;           // fp32: the tree's spheres, record k = input sphere bvh.order[k]
    std::vector<SphereD> sd;           // fp64: the same
    std::vector<MatF> mf;
    std::vector<MatD> md;
    std::vector<SphereD> big;          // the big spheres (bvh.big), both precisions
    std::vector<BigF> bigf;            // ...relative to their near points (fp32 kernels)
    std::vector<TriF> tf;              // fp32: leaf order, then zero records covering TRIF_SLACK bytes
    std::vector<uint32_t> tmeta;       // fp32: per-triangle meta words, leaf order
    std::vector<TriD> td;              // fp64: leaf order
    std::vector<unsigned char> grid;   // the sphere grid's buffer (empty: the scene has none)
    GridHdr grid_hdr{};
    int grid_entries = 0;              // sphere references over its cells
    std::vector<int> remap;            // kernel id slot -> input index: spheres | big | host-built triangles (+ n)
    std::vector<int> unmap;            // remap's inverse (invert_remap); with gpu_build: the caller, once remap is whole
    SceneReach reach;
    float box_extent = 0.f;            // bound of |coordinate| over the node boxes and vertices
    double clo[3] = {0, 0, 0}, chi[3] = {0, 0, 0};   // gpu_build: the triangle centroids' bounds (Morton grid)
};

// rt_trace_rays_from's id map, remap's inverse: input index (spheres, then n + triangle) -> Hit::id
// (kernel_id_of_slot of the slot that holds it), NO_SELF for an index remap does not hold.
// remap: n_spheres tree positions | n_big big spheres | triangles; `total` input primitives.
void invert_remap(const std::vector<int>& remap, int n_spheres, int n_big, int total, std::vector<int>& unmap);

// Checks the arrays and packs them for a context of the given precision and tuning (the tree,
// grid and mesh-builder fields).  RT_OK, or the status rt_upload_scene_ex returns with its
// message in err; `out` is then unspecified.
int pack_scene(const rt_sphere* s, int n, const rt_material* m, int nm, const rt_triangle* tri, int ntri,
               const rt_tuning& tuning, bool f64, PackedScene& out, std::string& err);

}  // namespace rtx
