// rt_pack.cpp -- the host-side packing of a scene (rt_pack.h).  Host only, no HIP.
#include "rt_pack.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>

namespace rtx {

// The sphere grid's walk is exact and ends only for ray origins within +-GridHdr::far_o
// (rt_bvh.cpp build_sphere_grid); the kernel has no check for it (any such code in the walk
// cost C3 1.4 .. 9 %, r06), so each launch checks here, on the host, that no ray it can
// produce starts beyond it -- else it renders with the tree.  Rays start at the camera (its
// centre, within the defocus disk) or at hit points: on the geometry a ray can reach anywhere
// (reach.lo / reach.hi: small spheres swept over the shutter, triangles, big spheres that
// refract or move), or on a static opaque big sphere B, which a ray from O reaches only
// within the tangent distance sqrt(|O - C|^2 - R^2) of O (a point of B seen from O), and
// whose surface starts no ray that meets B again.  Hit regions on the big spheres are grown
// from each other to a fixed point (a ground sphere alone: one step).  The margin covers the
// fp32 rounding of hit points.
bool grid_reach_ok(const SceneReach& reach, float far_o, const rt_camera& cam) {
    using Box = std::array<double, 6>;
    auto empty = []() {
        const double inf = std::numeric_limits<double>::infinity();
        return Box{inf, inf, inf, -inf, -inf, -inf};
    };
    auto join = [](Box& a, const Box& b) {
        for (int k = 0; k < 3; ++k) {
            a[k] = std::min(a[k], b[k]);
            a[3 + k] = std::max(a[3 + k], b[3 + k]);
        }
    };
    Box u0 = empty();
    for (int k = 0; k < 3; ++k) {
        const double r = cam.defocus_angle > 0 ? std::fabs(cam.defocus_disk_u[k]) + std::fabs(cam.defocus_disk_v[k]) : 0;
        // (std::min and std::max below would drop a NaN operand: such a camera proves nothing)
        if (std::isnan(cam.center[k]) || std::isnan(r)) return false;
        u0[k] =std::min(reach.lo[k], cam.center[k] - r);
        u0[3 + k] = std::max(reach.hi[k], cam.center[k] + r);
    }
    const size_t nb = reach.big.size();
    std::vector<Box> hit(nb, empty());
    bool changed = true;
    for (int it = 0; it < 16 && changed; ++it) {
        changed = false;
        for (size_t j = 0; j < nb; ++j) {
            Box from = u0;   // where a ray that meets B_j can start: anywhere but on B_j
            for (size_t k = 0; k < nb; ++k)
                if (k != j) join(from, hit[k]);
            const auto& b = reach.big[j];
            double d2 = 0, d2n = 0;   // the farthest corner of `from` from B_j's centre, and its nearest point
            for (int k = 0; k < 3; ++k) {
                const double e = std::max(std::fabs(from[k] - b[k]), std::fabs(from[3 + k] - b[k]));
                const double n = std::max({from[k] - b[k], b[k] - from[3 + k], 0.0});
                d2 += e * e;
                d2n += n * n;
            }
            // (a ray could start inside B_j -- geometry embedded in it, or a box too loose to
            // tell: then all of B_j)
            const double t = d2n < b[3] * b[3] ? std::numeric_limits<double>::infinity()
                                               : std::sqrt(std::max(d2 - b[3] * b[3], 0.0));
            Box h;
            for (int k = 0; k < 3; ++k) {
                h[k] = std::max(from[k] - t, b[k] - b[3]);
                h[3 + k] = std::min(from[3 + k] + t, b[k] + b[3]);
            }
            if (!(h[0] <= h[3] && h[1] <= h[4] && h[2] <= h[5])) continue;
            Box g = hit[j];
            join(g, h);
            if (g != hit[j]) {
                hit[j] = g;
                changed = true;
            }
        }
    }
    if (changed) return false;   // (no fixed point within 16 rounds: the tree)
    Box all = u0;
    for (const Box& h : hit) join(all, h);
    double m = 0;
    for (int k = 0; k < 6; ++k) m = std::max(m, std::fabs(all[k]));
    return m * (1.0 + 0x1p-10) <= (double)far_o;   // (false for NaN)
}

namespace {

int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// the record (SphereF / SphereD) of an input sphere, each value converted once
template <class R>
R sphere_record(const rt_sphere& q, uint32_t meta) {
    using F = decltype(R::r);
    R r{};
    for (int a = 0; a < 3; ++a) {
        r.c[a] = (F)q.center[a];
        r.cv[a] = q.moving ? (F)q.center_vec[a] : (F)0;
    }
    r.r = (F)q.radius;
    r.meta = meta;
    return r;
}

}  // namespace

int pack_scene(const rt_sphere* s, int n, const rt_material* m, int nm, const rt_triangle* tri, int ntri,
               const rt_tuning& tuning, bool f64, PackedScene& out, std::string& err) {
    if (n < 0 || nm < 0 || ntri < 0 || (n > 0 && !s) || (nm > 0 && !m) || (ntri > 0 && !tri))
        return fail(err, RT_ERR_INVALID, "bad scene arrays (n=%d, nm=%d, ntri=%d)", n, nm, ntri);
    if (nm > (int)META_MAT_MASK) return fail(err, RT_ERR_LIMIT, "too many materials");
    for (int k = 0; k < nm; ++k)
        if (m[k].type < RT_LAMBERTIAN || m[k].type > RT_DIELECTRIC)
            return fail(err, RT_ERR_INVALID, "material %d has type %d", k, m[k].type);
    for (int k = 0; k < n; ++k) {
        if (s[k].mat < 0 || s[k].mat >= nm)
            return fail(err, RT_ERR_INVALID, "sphere %d references material %d of %d", k, s[k].mat, nm);
        if (!std::isfinite(s[k].radius)) return fail(err, RT_ERR_INVALID, "sphere %d radius not finite", k);
        bool ok = coord_ok(s[k].radius);
        for (int a = 0; a < 3; ++a) ok = ok && coord_ok(s[k].center[a]) && coord_ok(s[k].center_vec[a]);
        if (!ok) return fail(err, RT_ERR_LIMIT, "sphere %d: a coordinate is not finite or beyond +-1e30", k);
    }
    for (int k = 0; k < ntri; ++k) {
        if (tri[k].mat < 0 || tri[k].mat >= nm)
            return fail(err, RT_ERR_INVALID, "triangle %d references material %d of %d", k, tri[k].mat, nm);
        bool ok = true;
        for (int a = 0; a < 3; ++a) ok = ok && coord_ok(tri[k].v0[a]) && coord_ok(tri[k].v1[a]) && coord_ok(tri[k].v2[a]);
        if (!ok) return fail(err, RT_ERR_LIMIT, "triangle %d: a vertex coordinate is not finite or beyond +-1e30", k);
    }

    out = PackedScene{};
    out.f64 = f64;
    BuiltBvh& bvh = out.bvh;
    MeshBvh& mbvh = out.mbvh;
    std::string berr;
    BvhParams bp;
    bp.max_leaf = tuning.max_leaf;
    bp.cost_traverse = tuning.cost_traverse;
    bp.cost_intersect = tuning.cost_intersect;
    bp.front = tuning.front_spheres;
    bp.big = relatively_big_spheres(s, n, tri, ntri);
    if (!build_bvh(s, n, bp, bvh, berr)) return fail(err, RT_ERR_LIMIT, "%s", berr.c_str());
    out.gpu_build = ntri > 0 && tuning.mesh_builder != RT_MESH_BUILD_HOST;
    if (out.gpu_build) {
        // validation + centroid bounds for the Morton grid; the tree is built on the device
        if (ntri > MESH_MAX_TRIS) return fail(err, RT_ERR_LIMIT, "mesh holds at most 2^24 triangles");
        for (int a = 0; a < 3; ++a) {
            out.clo[a] = std::numeric_limits<double>::infinity();
            out.chi[a] = -std::numeric_limits<double>::infinity();
        }
        for (int k = 0; k < ntri; ++k)
            for (int a = 0; a < 3; ++a) {
                const double x0 = tri[k].v0[a], x1 = tri[k].v1[a], x2 = tri[k].v2[a];
                if (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(x2))
                    return fail(err, RT_ERR_LIMIT, "triangle %d has a non-finite vertex", k);
                const double cm = 0.5 * (std::fmin(x0, std::fmin(x1, x2)) + std::fmax(x0, std::fmax(x1, x2)));
                out.clo[a] = std::fmin(out.clo[a], cm);
                out.chi[a] = std::fmax(out.chi[a], cm);
            }
    } else if (!build_mesh_bvh(tri, ntri, tuning.mesh_max_leaf, tuning.mesh_cost_traverse, mbvh, berr)) {
        return fail(err, RT_ERR_LIMIT, "%s", berr.c_str());
    }

    const int nb = (int)bvh.order.size();
    auto meta_of = [&](const rt_sphere& q) {
        return make_meta((uint32_t)q.mat, (uint32_t)m[q.mat].type, q.moving ? 1u : 0u);
    };
    // the fp32 records: an fp32 scene's own, and what the grid lists in either precision
    std::vector<SphereF> sf;
    for (int k = 0; k < nb; ++k) {
        const rt_sphere& q = s[bvh.order[k]];
        sf.push_back(sphere_record<SphereF>(q, meta_of(q)));
        if (f64) out.sd.push_back(sphere_record<SphereD>(q, meta_of(q)));
    }
    // the big spheres' near points (BigF): on each, the point nearest the centre of the
    // other spheres' bounding box (the origin without others), and the outward normal there
    double sc_lo[3] = {0, 0, 0}, sc_hi[3] = {0, 0, 0};
    {
        bool any = false;
        for (int k = 0; k < n; ++k) {
            if (std::find(bvh.big.begin(), bvh.big.end(), k) != bvh.big.end()) continue;
            for (int a = 0; a < 3; ++a) {
                const double lo = s[k].center[a] - std::fabs(s[k].radius), hi = s[k].center[a] + std::fabs(s[k].radius);
                sc_lo[a] = any ? std::min(sc_lo[a], lo) : lo;
                sc_hi[a] = any ? std::max(sc_hi[a], hi) : hi;
            }
            any = true;
        }
    }
    // where rays can start (r06, grid_reach_ok): everything but the static opaque big spheres
    // as boxes, those as (centre, radius)
    {
        SceneReach& reach = out.reach;
        const double inf = std::numeric_limits<double>::infinity();
        for (int a = 0; a < 3; ++a) {
            reach.lo[a] = inf;
            reach.hi[a] = -inf;
        }
        auto add = [&](const double* p, double r) {
            for (int a = 0; a < 3; ++a) {
                reach.lo[a] = std::min(reach.lo[a], p[a] - r);
                reach.hi[a] = std::max(reach.hi[a], p[a] + r);
            }
        };
        for (int k = 0; k < n; ++k) {
            const rt_sphere& q = s[k];
            const bool is_big = std::find(bvh.big.begin(), bvh.big.end(), k) != bvh.big.end();
            if (is_big && !q.moving && m[q.mat].type != RT_DIELECTRIC) {
                reach.big.push_back({q.center[0], q.center[1], q.center[2], std::fabs(q.radius)});
                continue;
            }
            double p1[3];
            for (int a = 0; a < 3; ++a) p1[a] = q.center[a] + (q.moving ? q.center_vec[a] : 0.0);
            add(q.center, std::fabs(q.radius));
            add(p1, std::fabs(q.radius));
        }
        for (int k = 0; k < ntri; ++k) {
            add(tri[k].v0, 0.0);
            add(tri[k].v1, 0.0);
            add(tri[k].v2, 0.0);
        }
    }
    for (int k : bvh.big) {
        const rt_sphere& q = s[k];
        SphereD r = sphere_record<SphereD>(q, meta_of(q));
        r.inv_r = (float)(1.0 / q.radius);
        out.big.push_back(r);
        BigF f{};
        double nv[3], len = 0;
        for (int a = 0; a < 3; ++a) {
            nv[a] = 0.5 * (sc_lo[a] + sc_hi[a]) - q.center[a];
            len += nv[a] * nv[a];
        }
        len = std::sqrt(len);
        // (a negative radius -- the reference's inside-out sphere: the near point is still
        // centre + |r| na; n = (p0 - centre) / r and inv_r keep the radius' sign, so that
        // f = q + r n and (p - c) / r = (p - p0) / r + n hold as they are in the kernels)
        const double sgn = q.radius < 0 ? -1.0 : 1.0;
        for (int a = 0; a < 3; ++a) {
            const double na = len > 0 ? nv[a] / len : (a == 1 ? 1.0 : 0.0);
            f.n[a] = (float)(sgn * na);
            f.p0[a] = (float)(q.center[a] + std::fabs(q.radius) * na);
            f.cv[a] = q.moving ? (float)q.center_vec[a] : 0.0f;
        }
        f.r = (float)q.radius;
        f.inv_r = (float)(1.0 / q.radius);
        f.meta = r.meta;
        out.bigf.push_back(f);
    }
    for (int k : mbvh.order) {
        const rt_triangle& q = tri[k];
        const uint32_t meta = make_meta((uint32_t)q.mat, (uint32_t)m[q.mat].type, 0u);
        if (f64) {
            TriD r{};
            for (int a = 0; a < 3; ++a) {
                r.v0[a] = q.v0[a];
                r.e1[a] = q.v1[a] - q.v0[a];
                r.e2[a] = q.v2[a] - q.v0[a];
            }
            r.meta = meta;
            out.td.push_back(r);
        } else {
            TriF r{};   // each vertex rounded once: shared vertices stay identical (watertight test)
            double e1[3], e2[3];
            for (int a = 0; a < 3; ++a) {
                r.v0[a] = (float)q.v0[a];
                r.v1[a] = (float)q.v1[a];
                r.v2[a] = (float)q.v2[a];
                e1[a] = q.v1[a] - q.v0[a];
                e2[a] = q.v2[a] - q.v0[a];
            }
            r.n[0] = (float)(e1[1] * e2[2] - e1[2] * e2[1]);   // the facet normal, fp64
            r.n[1] = (float)(e1[2] * e2[0] - e1[0] * e2[2]);
            r.n[2] = (float)(e1[0] * e2[1] - e1[1] * e2[0]);
            out.tf.push_back(r);
            out.tmeta.push_back(meta);
        }
    }
    // the records plus TRIF_SLACK zero bytes (the if-if loop's 80-B leaf reads)
    if (!f64 && !out.tf.empty()) out.tf.resize(out.tf.size() + (TRIF_SLACK + sizeof(TriF) - 1) / sizeof(TriF), TriF{});
    for (int k = 0; k < nm; ++k) {
        double p[4] = {m[k].albedo[0], m[k].albedo[1], m[k].albedo[2], 0.0};
        if (m[k].type == RT_METAL) p[3] = m[k].fuzz < 1 ? m[k].fuzz : 1;  // material.h:33
        if (m[k].type == RT_DIELECTRIC) p[3] = m[k].ir;
        if (f64) {
            MatD r;
            for (int a = 0; a < 4; ++a) r.p[a] = p[a];
            out.md.push_back(r);
        } else {
            MatF r;
            for (int a = 0; a < 4; ++a) r.p[a] = (float)p[a];
            out.mf.push_back(r);
        }
    }
    // the uniform grid over the tree's spheres, where the scene suits one (TRAV_GRID);
    // fp64 scenes list their spheres from the records rounded to fp32 (the padding
    // covers the rounding: the cells only choose which spheres are tested)
    if (tuning.sphere_grid_density > 0 &&
        build_sphere_grid(sf.data(), bvh.front, nb, tuning.sphere_grid_density, tuning.sphere_grid_time_slabs,
                          f64 ? (int)sizeof(SphereD) : (int)sizeof(SphereF), out.grid_hdr, out.grid)) {
        const GridHdr& h = out.grid_hdr;
        const uint32_t last = ((const uint32_t*)out.grid.data())[h.n_cells - 1 + (uint32_t)(h.res[0] * h.res[1])];
        // (the last cell's end position, in bytes, less the pad layers and the cells)
        out.grid_entries = (int)((last >> GRID_POS_BITS) / 4u - h.n_cells - 2u * (uint32_t)(h.res[0] * h.res[1]));
    } else {
        out.grid.clear();
    }
    if (!f64) out.sf = std::move(sf);
    {
        // TRAV_F32BOX (fp64 kernels): a bound of |coordinate| over the sphere-tree boxes and
        // the triangles (the mesh boxes enclose them, rounded outward by an ulp)
        double ext = 0.0;
        for (const Node& nd : bvh.nodes)
            for (int a = 0; a < 3; ++a)
                ext = std::max({ext, (double)std::fabs(nd.lo0[a]), (double)std::fabs(nd.hi0[a]),
                                (double)std::fabs(nd.lo1[a]), (double)std::fabs(nd.hi1[a])});
        for (int k = 0; k < ntri; ++k)
            for (int a = 0; a < 3; ++a)
                ext = std::max({ext, std::fabs(tri[k].v0[a]), std::fabs(tri[k].v1[a]), std::fabs(tri[k].v2[a])});
        out.box_extent = std::isfinite(ext) ? (float)(ext * (1.0 + 0x1p-20)) : 3e38f;
    }
    // rt_trace_rays' id map: BVH sphere position -> input index, then the big spheres, then
    // the triangles in leaf order (input index + n; a device-built tree's: the caller)
    out.remap.reserve((size_t)nb + out.big.size() + (size_t)ntri);
    for (int k = 0; k < nb; ++k) out.remap.push_back(bvh.order[k]);
    for (int k : bvh.big) out.remap.push_back(k);
    for (int k : mbvh.order) out.remap.push_back(n + k);
    if (!out.gpu_build) invert_remap(out.remap, nb, (int)out.big.size(), n + ntri, out.unmap);
    return RT_OK;
}

void invert_remap(const std::vector<int>& remap, int n_spheres, int n_big, int total, std::vector<int>& unmap) {
    unmap.assign((size_t)std::max(total, 0), NO_SELF);
    for (size_t slot = 0; slot < remap.size(); ++slot)
        if (remap[slot] >= 0 && remap[slot] < total) unmap[(size_t)remap[slot]] = kernel_id_of_slot((int)slot, n_spheres, n_big);
}

}  // namespace rtx
