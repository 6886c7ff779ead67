// rt_occluded.h -- batched any-hit visibility (rt_occluded): hittable::hit's return value
// (hittable.h:28) for many rays, each over its own interval ray_t = (tmin, tmax).
//
// any_hit answers "has some primitive a root t with tmin < t < tmax" (interval::surrounds,
// interval.h:33-35) and nothing else: a lane leaves at its first hit, hit children are pushed
// in the order they are stored (no sorting network, no pop culling), and (tmin, tmax) stays
// what the caller gave for the whole traversal.  The primitive tests, the slab arithmetic and
// the stacks are closest_hit's (rt_device.h), so that
//   * fp32 with the default interval (0.001, inf) agrees with closest_hit's id != -1 ray for
//     ray: both run the same test functions on the same operands, a box that closest_hit
//     enters any_hit enters too (its tmax is never smaller), and a primitive any_hit reports
//     is one closest_hit either reaches or has culled behind an earlier hit;
//   * fp64 is the reference's boolean exactly: the spheres and triangles are tested in the
//     reference's fp64 operation order, the conservative fp32 boxes only prune.
// The sphere tree is walked, never the grid (whose reach proof is made per launch camera).
#pragma once
#include "rt_render_impl.h"

namespace rtx {

// fp32 bounds of an fp64 interval for box_hit_cons (TRAV_F32BOX): at or below tmin, at or
// above tmax, for either sign.  (float)x is within 2^-24 |x| of x (or within 2^-126 where the
// result is subnormal or flushed), the margin 2^-22 |x| + 2^-100 exceeds both; an infinite end
// stays infinite, an end beyond the fp32 range is clamped to it first and moves outwards from
// there.  (cons_tmax / CONS_TMIN of closest_hit hold for the positive interval (0.001, tmax) only.)
__device__ __forceinline__ float cons_lower(double tmin) {
    const float x = fminf((float)tmin, 0x1.fffffep127f);
    return x - __builtin_fmaf(fabsf(x), 0x1p-22f, 0x1p-100f);
}
__device__ __forceinline__ float cons_upper(double tmax) {
    const float x = fmaxf((float)tmax, -0x1.fffffep127f);
    return x + __builtin_fmaf(fabsf(x), 0x1p-22f, 0x1p-100f);
}

template <class R, bool EXACT, int TRAV = 0, bool MESH = false>
__device__ __forceinline__ bool any_hit(const SceneView<R>& sc, const Ray<R>& ray, const R tmin, const R tmax,
                                        uint16_t* stack, int stride) {
    const V3<R> o = ray.o, d = ray.d;
    const R a = len2(d);
    const R inv_a = rcp(a);

    // big spheres (rt_scene.h BIG_RADIUS)
    if (EXACT) {
        // reference arithmetic, fp64 (sphere.h:30-48)
        const V3<double> od = cvt<double>(o), dd = cvt<double>(d);
        for (int k = 0; k < sc.n_big; ++k) {
            const SphereD& s = sc.big[k];
            double t;
            if (sphere_root<double, true>(mk(s.c[0], s.c[1], s.c[2]), s.r, mk(s.cv[0], s.cv[1], s.cv[2]),
                                          (s.meta >> 30) & 1u, od, dd, (double)a, 0.0, (double)ray.time, (double)tmin,
                                          (double)tmax, false, t))
                return true;
        }
    } else {
        // fp32: relative to the sphere's near point (BigF), closest_hit's expressions
        for (int k = 0; k < sc.n_big; ++k) {
            const BigF& s = sc.bigf[k];
            V3<R> p0 = mk((R)s.p0[0], (R)s.p0[1], (R)s.p0[2]);
            if ((s.meta >> 30) & 1u) p0 = madd((R)ray.time, mk((R)s.cv[0], (R)s.cv[1], (R)s.cv[2]), p0);
            const V3<R> q = o - p0, nn = mk((R)s.n[0], (R)s.n[1], (R)s.n[2]);
            const R b = -fma((R)s.r, dot(nn, d), dot(q, d));
            const R cc = fma((R)2 * (R)s.r, dot(nn, q), dot(q, q));
            const R disc = b * b - a * cc;
            if (disc < 0) continue;
            const R qq = b + copysign((R)sqrt(disc), b);
            const R ta = cc * rcp(qq), tb = qq * inv_a;
            const R t0 = fmin(ta, tb), t1 = fmax(ta, tb);
            if ((tmin < t0 && t0 < tmax) || (tmin < t1 && t1 < tmax)) return true;
        }
    }

    // one sphere of the LDS array (the tree's leaves and the front list share it)
    using Sph = typename Prec<R>::Sph;
    auto test_one = [&](int k) -> bool {
        const Sph* rec = sc.sph + k;
        R tk;
        if constexpr (!EXACT && (TRAV & TRAV_B128) != 0) {
            const float4* q = (const float4*)rec;
            const float4 s0 = q[0], s1 = q[1];   // c, r | cv, meta
            keep_live(__float_as_uint(s0.w));
            keep_live(__float_as_uint(s1.w));
            return sphere_root<R, false, (TRAV & TRAV_SELROOT) != 0>(
                mk((R)s0.x, (R)s0.y, (R)s0.z), (R)s0.w, mk((R)s1.x, (R)s1.y, (R)s1.z), false, o, d, a, inv_a,
                ray.time, tmin, tmax, false, tk);
        }
        const auto& s = *rec;
        return sphere_root<R, EXACT, (TRAV & TRAV_SELROOT) != 0>(mk((R)s.c[0], (R)s.c[1], (R)s.c[2]), (R)s.r,
                                     mk((R)s.cv[0], (R)s.cv[1], (R)s.cv[2]), (s.meta >> 30) & 1u, o, d, a, inv_a,
                                     ray.time, tmin, tmax, false, tk);
    };
    // front list (rt_tuning.front_spheres)
    for (int k = 0; k < sc.n_front; ++k)
        if (test_one(k)) return true;

    constexpr bool CONS = EXACT && (TRAV & TRAV_F32BOX) != 0;
    using BT = std::conditional_t<CONS, float, R>;   // box-test distances
    // the boxes' interval: fp64 with fp32 boxes widens it outwards (boxes only prune)
    BT blo, bhi;
    if constexpr (CONS) {
        blo = cons_lower((double)tmin);
        bhi = cons_upper((double)tmax);
    } else {
        blo = tmin;
        bhi = tmax;
    }
    const V3<R> inv = mk(slab_rcp(d.x), slab_rcp(d.y), slab_rcp(d.z));
    const V3<R> oi = EXACT ? o : o * inv;   // fp32: t = lo*inv - o*inv as one FMA
    ConsSlabs cs;
    if constexpr (CONS) cs = cons_slabs(cvt<double>(o), cvt<double>(d), sc.box_extent);

    // sphere tree (LDS): closest_hit's stack -- the latest push in a register, older ones in
    // this lane's LDS column (stack_entries() counts on the register) -- without the ordering
    if (sc.n_nodes > 0) {
        const Node* nodes = sc.nodes;
        uint32_t ref = 0, top = REF_NONE;
        int sp = 0;
        auto pop = [&]() -> uint32_t {
            if (top != REF_NONE) {
                const uint32_t r = top;
                top = REF_NONE;
                return r;
            }
            if (sp > 0) {
                --sp;
                return stack[sp * stride];
            }
            return REF_NONE;
        };
        for (;;) {
            while (!(ref & REF_LEAF)) {
                const uint4* q = (const uint4*)(nodes + ref);
                const uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];   // one 64-B node
                const float lo0[3] = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z)};
                const float hi0[3] = {__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z)};
                const float lo1[3] = {__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w2.z)};
                const float hi1[3] = {__uint_as_float(w3.x), __uint_as_float(w3.y), __uint_as_float(w3.z)};
                const uint32_t r0 = w0.w, r1 = w1.w;
                if (TRAV & TRAV_B128) {
                    keep_live(w2.w);
                    keep_live(w3.w);
                }
                BT tn0, tn1;
                bool h0, h1;
                if constexpr (CONS) {
                    h0 = box_hit_cons(lo0, hi0, cs, blo, bhi, tn0);
                    h1 = box_hit_cons(lo1, hi1, cs, blo, bhi, tn1);
                } else {
                    h0 = box_hit(lo0, hi0, inv, oi, blo, bhi, tn0);
                    h1 = box_hit(lo1, hi1, inv, oi, blo, bhi, tn1);
                }
                if (h0 && h1) {
                    if (top != REF_NONE) {
                        stack[sp * stride] = (uint16_t)top;
                        ++sp;
                    }
                    top = r1;
                    ref = r0;
                } else if (h0 || h1) {
                    ref = h0 ? r0 : r1;
                } else {
                    ref = pop();
                }
            }
            if (ref == REF_NONE) break;
            const int first = (int)(ref & 0x7ffu);
            const int last = first + (int)((ref >> 11) & 0xfu);
            for (int k = first; k <= last; ++k)
                if (test_one(k)) return true;
            ref = pop();
            if (ref == REF_NONE) break;
        }
    }

    if (MESH && sc.n_mnodes > 0) {
        // Mesh BVH (4-wide, HBM): closest_hit's stack -- a register, then the LDS column, then
        // scratch -- with the first hit child continued and the others pushed as stored.
        uint32_t mstk[MESH_STACK_MAX];
        int sp = 0;
        uint32_t ref = 0, top = MREF_EMPTY;
        typedef __attribute__((address_space(3))) uint32_t lds_u32;
        lds_u32* const mlds = (lds_u32*)sc.mstack;
        auto mpop = [&]() -> uint32_t {
            if (top != MREF_EMPTY) {
                const uint32_t r = top;
                top = MREF_EMPTY;
                return r;
            }
            if (sp <= 0) return MREF_EMPTY;
            --sp;
            if (sp < sc.n_mstack) return mlds[sp * stride];
            return mstk[sp - sc.n_mstack];
        };
        auto mpush = [&](uint32_t r) {
            if (top != MREF_EMPTY) {
                if (sp < sc.n_mstack)
                    mlds[sp * stride] = top;
                else
                    mstk[sp - sc.n_mstack] = top;
                ++sp;
            }
            top = r;
        };
        typedef float nf4 __attribute__((ext_vector_type(4)));
        typedef uint32_t nu4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) const nu4 glb_u4;
        // One 4-wide node from its 7 loaded words: the first hit child is returned, the other
        // hit children pushed (or a pop).
        auto mnode = [&](const nf4 lx, const nf4 ly, const nf4 lz, const nf4 hx, const nf4 hy, const nf4 hz,
                         const nu4 rr) -> uint32_t {
            const uint32_t r[4] = {rr.x, rr.y, rr.z, rr.w};
            const float LX[4] = {lx.x, lx.y, lx.z, lx.w}, LY[4] = {ly.x, ly.y, ly.z, ly.w};
            const float LZ[4] = {lz.x, lz.y, lz.z, lz.w}, HX[4] = {hx.x, hx.y, hx.z, hx.w};
            const float HY[4] = {hy.x, hy.y, hy.z, hy.w}, HZ[4] = {hz.x, hz.y, hz.z, hz.w};
            uint32_t next = MREF_EMPTY;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                bool hc;
                if constexpr (!EXACT) {
                    const float t0x = __builtin_fmaf(LX[c], inv.x, -oi.x), t1x = __builtin_fmaf(HX[c], inv.x, -oi.x);
                    const float t0y = __builtin_fmaf(LY[c], inv.y, -oi.y), t1y = __builtin_fmaf(HY[c], inv.y, -oi.y);
                    const float t0z = __builtin_fmaf(LZ[c], inv.z, -oi.z), t1z = __builtin_fmaf(HZ[c], inv.z, -oi.z);
                    const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), (float)tmin));
                    const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), (float)tmax));
                    hc = tn <= tf;
                } else {
                    const float lo[3] = {LX[c], LY[c], LZ[c]}, hi[3] = {HX[c], HY[c], HZ[c]};
                    BT tn;
                    if constexpr (CONS)
                        hc = box_hit_cons(lo, hi, cs, blo, bhi, tn);
                    else
                        hc = box_hit(lo, hi, inv, oi, blo, bhi, tn);
                }
                if (hc && r[c] != MREF_EMPTY) {
                    if (next == MREF_EMPTY)
                        next = r[c];
                    else
                        mpush(r[c]);
                }
            }
            return next != MREF_EMPTY ? next : mpop();
        };
        if constexpr (!EXACT && (TRAV & TRAV_MIFIF) != 0) {
            // closest_hit's if-if loop: a lane visits one node or tests one leaf per iteration,
            // node and triangle loads leaving through the same instructions
            const TriF* tris = (const TriF*)sc.tris;
            {
                // a ray that misses the mesh's box within its interval skips the mesh
                const float mlo[3] = {sc.mbox[0], sc.mbox[1], sc.mbox[2]};
                const float mhi[3] = {sc.mbox[3], sc.mbox[4], sc.mbox[5]};
                R tb;
                if (!box_hit(mlo, mhi, inv, oi, tmin, tmax, tb)) ref = MREF_EMPTY;
            }
            auto mtri = [&](const V3<float> p0, const V3<float> p1, const V3<float> p2, const V3<float> nn) -> bool {
                float t;
                return tri_wt(p0, p1, p2, nn, o, d, tmin, tmax, t);
            };
            auto fw = [](uint32_t u) { return __uint_as_float(u); };
            for (;;) {
                if (ref == MREF_EMPTY) break;
                const bool leaf = (ref & MREF_LEAF) != 0;
                const int first = (int)(ref & 0xffffffu);
                const int last = first + (int)((ref >> 24) & 0x7fu);
                // node: its 7 words of 16 B; leaf: its first two 48-B records (6 words: the
                // triangle array carries TRIF_SLACK bytes past its end), the 7th load repeating
                // the leaf's first address
                const glb_u4* q = leaf ? (const glb_u4*)(tris + first) : (const glb_u4*)(sc.mnodes + ref);
                const glb_u4* q6 = leaf ? q : q + 6;
                const nu4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4], w5 = q[5], w6 = q6[0];
                if (!leaf) {
                    ref = mnode(__builtin_bit_cast(nf4, w0), __builtin_bit_cast(nf4, w1), __builtin_bit_cast(nf4, w2),
                                __builtin_bit_cast(nf4, w3), __builtin_bit_cast(nf4, w4), __builtin_bit_cast(nf4, w5), w6);
                    continue;
                }
                // words: tri A v0.xyz v1.x | v1.yz v2.xy | v2.z n.xyz, tri B in w3..w5 likewise
                if (mtri(mk(fw(w0.x), fw(w0.y), fw(w0.z)), mk(fw(w0.w), fw(w1.x), fw(w1.y)),
                         mk(fw(w1.z), fw(w1.w), fw(w2.x)), mk(fw(w2.y), fw(w2.z), fw(w2.w))))
                    return true;
                if (last > first) {
                    if (mtri(mk(fw(w3.x), fw(w3.y), fw(w3.z)), mk(fw(w3.w), fw(w4.x), fw(w4.y)),
                             mk(fw(w4.z), fw(w4.w), fw(w5.x)), mk(fw(w5.y), fw(w5.z), fw(w5.w))))
                        return true;
                    for (int k = first + 2; k <= last; ++k) {
                        const TriF& r = tris[k];
                        if (mtri(mk(r.v0[0], r.v0[1], r.v0[2]), mk(r.v1[0], r.v1[1], r.v1[2]),
                                 mk(r.v2[0], r.v2[1], r.v2[2]), mk(r.n[0], r.n[1], r.n[2])))
                            return true;
                    }
                }
                ref = mpop();
            }
        } else {
            for (;;) {
                while (!(ref & MREF_LEAF)) {
                    const glb_u4* q = (const glb_u4*)(sc.mnodes + ref);
                    const nu4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4], w5 = q[5], w6 = q[6];
                    ref = mnode(__builtin_bit_cast(nf4, w0), __builtin_bit_cast(nf4, w1), __builtin_bit_cast(nf4, w2),
                                __builtin_bit_cast(nf4, w3), __builtin_bit_cast(nf4, w4), __builtin_bit_cast(nf4, w5), w6);
                }
                if (ref == MREF_EMPTY) break;
                const int first = (int)(ref & 0xffffffu);
                const int last = first + (int)((ref >> 24) & 0x7fu);
                // the next triangle's load is issued before this one's test
                typename Prec<R>::Tri tr = sc.tris[first];
                for (int k = first; k <= last; ++k) {
                    const typename Prec<R>::Tri nx = sc.tris[k < last ? k + 1 : last];
                    R t;
                    if (tri_hit(tr, o, d, tmin, tmax, t)) return true;
                    tr = nx;
                }
                ref = mpop();
                if (ref == MREF_EMPTY) break;
            }
        }
    }
    return false;
}

// rt_occluded: one ray per lane (grid-stride), the scene in LDS as in trace_kernel, one byte
// per ray.  intervals: n records {tmin, tmax}, or null for (0.001, inf) on every ray.  An
// interval that surrounds nothing (tmin >= tmax, or a NaN end) answers 0 without a traversal.
template <class R, bool EXACT, int BLOCK, int TRAV, bool MESH>
__global__ __launch_bounds__(BLOCK) void occluded_kernel(RenderParams P, const R* __restrict__ rays, int n,
                                                         const R* __restrict__ intervals,
                                                         uint8_t* __restrict__ occluded) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* s_stack;
    uint32_t* s_mstack;
    const SceneView<R> sc = load_scene_lds<R, BLOCK, TRAV, MESH>(P, smem, s_stack, s_mstack);
    __syncthreads();
    uint16_t* stack = s_stack + threadIdx.x;
    for (int base = blockIdx.x * BLOCK; base < n; base += gridDim.x * BLOCK) {
        const int i = base + (int)threadIdx.x;
        if (i >= n) break;
        const R* q = rays + (size_t)i * 7;
        Ray<R> ray;
        ray.o = mk(q[0], q[1], q[2]);
        ray.d = mk(q[3], q[4], q[5]);
        ray.time = q[6];
        R tmin = (R)0.001, tmax = (R)__builtin_huge_valf();
        if (intervals) {
            tmin = intervals[(size_t)i * 2];
            tmax = intervals[(size_t)i * 2 + 1];
        }
        bool hit = false;
        if (tmin < tmax) hit = any_hit<R, EXACT, TRAV, MESH>(sc, ray, tmin, tmax, stack, BLOCK);
        occluded[i] = hit ? (uint8_t)1 : (uint8_t)0;
    }
}

}  // namespace rtx
