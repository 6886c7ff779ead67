// bvh_boxes_driver.cpp -- the sphere tree and the sphere grid over scenes with negative radii
// (the reference's hollow spheres: sphere.h's roots use radius * radius, its box orders the
// corners), built with -fsanitize=address,undefined (build.py build_bvh_boxes, run by
// tests/test_bvh_boxes.py).  No GPU code.
//
//   bvh_boxes_driver SPHERES.f64
//
// SPHERES.f64: n x 8 doubles (centre, centre motion, radius, moving flag).  For max_leaf in
// {1, 4} x front in {0, -1, 3}, build_bvh over the scene as given, over the scene with every
// radius made positive and over the scene with every radius made negative:
//   * every sphere that is neither big nor in the front list occurs exactly once in `order`
//     behind the front list, the front spheres once in it, the big ones never, and the leaves
//     reached from the root cover the tree's positions exactly once;
//   * every child box has lo <= hi on each axis and contains [min(c0, c1) - |r|, max(c0, c1) +
//     |r|] of every sphere beneath it (so does sphere_box of every sphere);
//   * the three trees are byte-identical (nodes, order, front, big, depth, leaves): the boxes
//     may depend on |r| only;
//   * build_sphere_grid over the fp32 records (made as rt_upload_scene makes them) returns the
//     same verdict, header and bytes for the three sign patterns.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingproject_amd/csrc/rt_bvh.h"
#include "../../raytracingproject_amd/csrc/rt_scene.h"

using namespace rtx;

static long long checks_failed = 0;
static void check(bool ok, const char* what, int a = -1, int b = -1) {
    if (!ok && ++checks_failed <= 20) std::printf("CHECK FAILED: %s (%d, %d)\n", what, a, b);
}

// the sphere's swept box over the shutter, from |r|
static void swept(const rt_sphere& s, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) {
        const double c0 = s.center[a], c1 = s.center[a] + (s.moving ? s.center_vec[a] : 0.0);
        lo[a] = std::fmin(c0, c1) - std::fabs(s.radius);
        hi[a] = std::fmax(c0, c1) + std::fabs(s.radius);
    }
}

static bool box_holds(const float blo[3], const float bhi[3], const rt_sphere& s) {
    double lo[3], hi[3];
    swept(s, lo, hi);
    for (int a = 0; a < 3; ++a)
        if (!((double)blo[a] <= lo[a] && (double)bhi[a] >= hi[a])) return false;
    return true;
}

struct Walk {
    const std::vector<rt_sphere>& s;
    const BuiltBvh& b;
    std::vector<int> covered;   // per position of `order`: leaves that hold it
    int depth = 0;

    // the input spheres beneath `ref`
    std::vector<int> beneath(uint32_t ref, int d) {
        std::vector<int> out;
        if (ref & REF_LEAF) {
            const int count = (int)((ref >> 11) & 0xfu) + 1, first = (int)(ref & 0x7ffu);
            for (int k = first; k < first + count; ++k) {
                const bool inside = k >= b.front && k < (int)b.order.size();
                check(inside, "a leaf's positions lie behind the front list, within order", k, (int)b.order.size());
                if (!inside) continue;
                ++covered[k];
                out.push_back(b.order[k]);
            }
            return out;
        }
        const bool known = ref < b.nodes.size() && d <= STACK_MAX;
        check(known, "an inner ref names a node, no deeper than the stack", (int)ref, d);
        if (!known) return out;
        depth = d > depth ? d : depth;
        const Node& nd = b.nodes[ref];
        const bool twice = b.nodes.size() == 1 && nd.ref0 == nd.ref1 && (nd.ref0 & REF_LEAF);   // single-leaf root
        for (int c = 0; c < (twice ? 1 : 2); ++c) {
            const float* lo = c ? nd.lo1 : nd.lo0;
            const float* hi = c ? nd.hi1 : nd.hi0;
            for (int a = 0; a < 3; ++a) check(lo[a] <= hi[a], "a child box has lo <= hi", (int)ref, a);
            const std::vector<int> sub = beneath(c ? nd.ref1 : nd.ref0, d + 1);
            for (int k : sub) check(box_holds(lo, hi, s[k]), "a child box contains every sphere beneath it", (int)ref, k);
            out.insert(out.end(), sub.begin(), sub.end());
        }
        if (twice) {
            for (int a = 0; a < 3; ++a) check(nd.lo1[a] <= nd.hi1[a], "a child box has lo <= hi", (int)ref, a);
            for (int k : out) check(box_holds(nd.lo1, nd.hi1, s[k]), "a child box contains every sphere beneath it", (int)ref, k);
        }
        return out;
    }
};

static void check_tree(const std::vector<rt_sphere>& s, const BuiltBvh& b) {
    const int n = (int)s.size();
    std::vector<int> seen(n, 0), where(n, -1);
    for (int k = 0; k < (int)b.order.size(); ++k) {
        const int id = b.order[k];
        const bool ok = id >= 0 && id < n;
        check(ok, "order holds input indices", k, id);
        if (!ok) return;
        ++seen[id];
        where[id] = k;
    }
    std::vector<char> big(n, 0);
    for (int k : b.big) {
        check(k >= 0 && k < n && std::fabs(s[k].radius) >= BIG_RADIUS, "big holds the spheres of |r| >= BIG_RADIUS", k);
        if (k >= 0 && k < n) big[k] = 1;
    }
    check(b.front >= 0 && b.front <= (int)b.order.size(), "front within order", b.front);
    for (int k = 0; k < n; ++k) {
        if (std::fabs(s[k].radius) >= BIG_RADIUS) check(big[k] && seen[k] == 0, "a big sphere is in big and not in order", k);
        else check(!big[k] && seen[k] == 1, "a sphere that is not big occurs exactly once in order", k, seen[k]);
    }
    Walk w{s, b, std::vector<int>(b.order.size(), 0)};
    if (!b.nodes.empty()) w.beneath(0u, 1);
    for (int k = 0; k < (int)b.order.size(); ++k)
        check(w.covered[k] == (k < b.front ? 0 : 1), "the leaves cover each tree position once, no front position", k,
              w.covered[k]);
    check(b.nodes.empty() == ((int)b.order.size() == b.front), "a tree exactly where spheres are left for it");
    check(w.depth == b.depth, "depth is the deepest inner node", w.depth, b.depth);
}

static bool same_tree(const BuiltBvh& x, const BuiltBvh& y) {
    return x.nodes.size() == y.nodes.size() &&
           (x.nodes.empty() || !std::memcmp(x.nodes.data(), y.nodes.data(), x.nodes.size() * sizeof(Node))) &&
           x.order == y.order && x.big == y.big && x.front == y.front && x.depth == y.depth && x.leaves == y.leaves;
}

// the fp32 records of the tree's spheres in `order`, as rt_upload_scene makes them
static std::vector<SphereF> records(const std::vector<rt_sphere>& s, const BuiltBvh& b) {
    std::vector<SphereF> sf;
    for (int k : b.order) {
        const rt_sphere& q = s[k];
        SphereF r{};
        for (int a = 0; a < 3; ++a) {
            r.c[a] = (float)q.center[a];
            r.cv[a] = q.moving ? (float)q.center_vec[a] : 0.0f;
        }
        r.r = (float)q.radius;
        sf.push_back(r);
    }
    return sf;
}

struct BuiltGrid {
    bool ok = false;
    GridHdr hdr;
    std::vector<unsigned char> buf;
};

static BuiltGrid grid_of(const std::vector<rt_sphere>& s, const BuiltBvh& b, double density) {
    BuiltGrid g;
    std::memset(&g.hdr, 0, sizeof g.hdr);
    const std::vector<SphereF> sf = records(s, b);
    g.ok = build_sphere_grid(sf.data(), b.front, (int)sf.size(), density, 32, (int)sizeof(SphereF), g.hdr, g.buf);
    return g;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<rt_sphere> given;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        double v[8];
        while (std::fread(v, sizeof(double), 8, f) == 8) {
            rt_sphere s{};
            for (int a = 0; a < 3; ++a) s.center[a] = v[a], s.center_vec[a] = v[3 + a];
            s.radius = v[6];
            s.moving = v[7] != 0.0;
            given.push_back(s);
        }
        std::fclose(f);
    }
    if (given.empty()) return 2;
    int negative = 0;
    std::vector<rt_sphere> scenes[3] = {given, given, given};   // as given, every radius > 0, every radius < 0
    for (size_t k = 0; k < given.size(); ++k) {
        negative += given[k].radius < 0;
        scenes[1][k].radius = std::fabs(given[k].radius);
        scenes[2][k].radius = -std::fabs(given[k].radius);
    }
    for (const rt_sphere& s : given) {
        float lo[3], hi[3];
        sphere_box(s, lo, hi);
        for (int a = 0; a < 3; ++a) check(lo[a] <= hi[a], "sphere_box has lo <= hi", a);
        check(box_holds(lo, hi, s), "sphere_box contains the sphere's swept box");
    }
    int trees = 0, grids = 0;
    for (int max_leaf : {1, 4})
        for (int front : {0, -1, 3}) {
            BvhParams p;
            p.max_leaf = max_leaf;
            p.front = front;
            BuiltBvh b[3];
            bool built = true;
            for (int v = 0; v < 3; ++v) {
                std::string err;
                const bool ok = build_bvh(scenes[v].data(), (int)scenes[v].size(), p, b[v], err);
                check(ok, err.c_str(), max_leaf, front);
                built = built && ok;
                if (ok) check_tree(scenes[v], b[v]);
            }
            if (!built) continue;
            ++trees;
            check(same_tree(b[0], b[1]), "the tree of the scene as given equals the tree of |r|", max_leaf, front);
            check(same_tree(b[2], b[1]), "the tree of -|r| equals the tree of |r|", max_leaf, front);
            for (double density : {2.0, 8.0}) {
                BuiltGrid g[3];
                for (int v = 0; v < 3; ++v) g[v] = grid_of(scenes[v], b[v], density);
                for (int v : {0, 2}) {
                    check(g[v].ok == g[1].ok, "the grid builder's verdict does not depend on the radius signs", v);
                    check(!std::memcmp(&g[v].hdr, &g[1].hdr, sizeof(GridHdr)), "the grid header depends on |r| only", v);
                    check(g[v].buf == g[1].buf, "the grid's bytes depend on |r| only", v);
                }
                grids += g[1].ok;
            }
        }
    std::printf("bvh_boxes spheres %zu negative %d trees %d grids %d checks failed %lld\n", given.size(), negative, trees,
                grids, checks_failed);
    return checks_failed ? 1 : 0;
}
