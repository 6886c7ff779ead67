// quant_range_driver.cpp -- render_coherent's finish (csrc/rt_render_impl.h) before and after
// r18's lean finish, restated for the CPU and compared sample by sample.  No GPU code; the
// predicate under test is the kernel's own (csrc/rt_quant.h).
//
// A finished sample is three channels q on the 2^-19 grid (q = rintf(L 2^19) 2^-19), a pixel and
// whether the wave's current item takes it into its LDS sums (in_item).  What it does to the
// frame is, per channel, exactly one of: a float added to the item sum (which reaches the packed
// word later as (u64)(sum 2^19)), an integer added to the launch's packed word, an integer added
// to the 64-bit running sum in units of 2^-28, a flag -- or nothing.
//   old: in01 = every channel >= 0.f and <= 1.f; in_item && in01 -> item sums (q != 0 only),
//        otherwise flush_sample(cnt = 1).
//   new: in01 = rtx::in01 (integer compare); in01 && in_item -> item sums; in01 && !in_item ->
//        u = (u32)(q 2^19), packed words R | G << 32 and B; !in01 -> flush_sample(cnt = 1).
// Checked: (1) all 2^32 bit patterns of channel 0 beside two fixed in-range channels, both
// values of in_item, and the other two positions over every 256th pattern: the two predicates
// differ for -0.0 alone, and the contribution (in units of 2^-28) and flags are equal for every
// pattern; (2) 10^6 random triples quantised as the kernel quantises them; (3) every triple over
// {0, -0, 1, 1 + ulp, 2^-19, NaN, +inf, -inf}, both in_item.
//
//   quant_range_driver [threads]        exit status 0: all equal
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "rt_quant.h"

namespace {

constexpr int FIX_SHIFT = 28, FIX_SAMPLE_SHIFT = 19;   // rt_device.h
constexpr uint32_t FIX_NAN = 1u, FIX_POS = 2u, FIX_NEG = 4u;
constexpr float SC = (float)(1 << FIX_SAMPLE_SHIFT), ISC = 1.f / SC;

float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

// What one sample adds: per channel an item-sum float, a packed integer, a 64-bit integer; flags.
struct Effect {
    float isum[3] = {0.f, 0.f, 0.f};
    bool isum_add[3] = {false, false, false};
    unsigned long long packed[3] = {0, 0, 0};
    long long accum[3] = {0, 0, 0};
    uint32_t flags = 0;
    // Is channel c's contribution to the pixel's sum the same in a and b?  The same kind of add
    // with the same operand; or an item-sum float v on one side and the packed integer u on the
    // other with v 2^19 == u (the item's sums reach the packed word as (u64)(sum 2^19), exact for
    // values on the grid); an add of integer 0 is no add.
    static bool same(const Effect& a, const Effect& b, int c) {
        if (a.isum_add[c] != b.isum_add[c]) {
            const Effect &f = a.isum_add[c] ? a : b, &u = a.isum_add[c] ? b : a;
            return u.accum[c] == 0 && u.packed[c] <= (1ull << FIX_SAMPLE_SHIFT) &&
                   f.isum[c] * (float)(1 << FIX_SAMPLE_SHIFT) == (float)u.packed[c];
        }
        uint32_t x, y;
        std::memcpy(&x, &a.isum[c], 4);
        std::memcpy(&y, &b.isum[c], 4);
        return x == y && a.packed[c] == b.packed[c] && a.accum[c] == b.accum[c];
    }
};

// flush_sample (rt_render_impl.h) with cnt = 1: the decisions, and what the atomics would add
void flush_sample(const float q[3], Effect& e) {
    for (int c = 0; c < 3; ++c) {
        const float v = q[c];
        if (v == 0.f) continue;
        if (v > 0.f && v <= 1.f) {
            e.packed[c] = (unsigned long long)(v * SC);
            continue;
        }
        const double d = (double)v * (double)(1ll << FIX_SHIFT);
        if (std::fabs(d) < 0x1p62)
            e.accum[c] = (long long)d;
        else
            e.flags |= (d != d ? FIX_NAN : d > 0 ? FIX_POS : FIX_NEG) << (3 * c);
    }
}

void item_sums(const float q[3], Effect& e) {
    for (int c = 0; c < 3; ++c)
        if (q[c] != 0.f) {
            e.isum[c] = q[c];
            e.isum_add[c] = true;
        }
}

bool in01_old(const float q[3]) {
    return q[0] >= 0.f && q[0] <= 1.f && q[1] >= 0.f && q[1] <= 1.f && q[2] >= 0.f && q[2] <= 1.f;
}

Effect finish_old(const float q[3], bool in_item) {
    Effect e;
    if (in_item && in01_old(q))
        item_sums(q, e);
    else
        flush_sample(q, e);
    return e;
}

Effect finish_new(const float q[3], bool in_item) {
    Effect e;
    if (rtx::in01(q[0], q[1], q[2])) {
        if (in_item) {
            item_sums(q, e);
        } else {
            for (int c = 0; c < 3; ++c) e.packed[c] = (uint32_t)(q[c] * SC);
        }
    } else {
        flush_sample(q, e);
    }
    return e;
}

struct Tally {
    unsigned long long checked = 0, pred_differs = 0, failed = 0;
};

bool has_minus_zero(const float q[3]) {
    for (int c = 0; c < 3; ++c)
        if (q[c] == 0.f && std::signbit(q[c])) return true;
    return false;
}

void check(const float q[3], bool in_item, Tally& t) {
    const Effect a = finish_old(q, in_item), b = finish_new(q, in_item);
    bool ok = a.flags == b.flags;
    for (int c = 0; c < 3; ++c) ok = ok && Effect::same(a, b, c);
    // the packed words hold 32 bits per channel
    for (int c = 0; c < 3; ++c) ok = ok && b.packed[c] <= 0xffffffffull;
    const bool pa = in01_old(q), pb = rtx::in01(q[0], q[1], q[2]);
    if (pa != pb) {
        ++t.pred_differs;
        // only -0.0 may tell the predicates apart, and only old-true / new-false
        ok = ok && pa && !pb && has_minus_zero(q);
    }
    ++t.checked;
    if (!ok) {
        if (t.failed++ < 8) {
            uint32_t u[3];
            std::memcpy(u, q, sizeof u);
            std::printf("MISMATCH q = %08x %08x %08x in_item %d: predicate %d -> %d, flags %x -> %x\n", u[0], u[1], u[2],
                        (int)in_item, (int)pa, (int)pb, a.flags, b.flags);
        }
    }
}

void merge(Tally& into, const Tally& t) {
    into.checked += t.checked;
    into.pred_differs += t.pred_differs;
    into.failed += t.failed;
}

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the kernel's rounding of a radiance channel onto the grid
float quantise(float l) { return std::nearbyintf(l * SC) * ISC; }

}   // namespace

int main(int argc, char** argv) {
    int nthreads = argc > 1 ? std::atoi(argv[1]) : (int)std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;

    // (1) every bit pattern of one channel
    Tally sweep;
    {
        std::vector<Tally> part((size_t)nthreads);
        std::vector<std::thread> pool;
        for (int k = 0; k < nthreads; ++k)
            pool.emplace_back([&, k]() {
                Tally t;
                const uint64_t lo = (1ull << 32) * (uint64_t)k / (uint64_t)nthreads,
                               hi = (1ull << 32) * (uint64_t)(k + 1) / (uint64_t)nthreads;
                for (uint64_t u = lo; u < hi; ++u) {
                    const float v = from_bits((uint32_t)u);
                    const float q0[3] = {v, 0.5f, 1.f};
                    check(q0, false, t);
                    check(q0, true, t);
                    if ((u & 0xffu) == 0) {   // (-0.0 is among them)
                        const float q1[3] = {ISC, v, 0.f}, q2[3] = {1.f, 0.25f, v};
                        check(q1, false, t);
                        check(q1, true, t);
                        check(q2, false, t);
                        check(q2, true, t);
                    }
                }
                part[(size_t)k] = t;
            });
        for (auto& th : pool) th.join();
        for (const Tally& t : part) merge(sweep, t);
    }
    std::printf("sweep checked %llu predicate-differs %llu failed %llu\n", sweep.checked, sweep.pred_differs, sweep.failed);

    // (2) random triples, quantised as the kernel does: in-range radiance mostly, then values
    // around the ends of the range, large ones, and raw bit patterns (NaN, inf, denormals)
    Tally rnd;
    uint64_t seed = 0x5EEDull;
    for (int n = 0; n < 1000000; ++n) {
        float q[3];
        for (int c = 0; c < 3; ++c) {
            const uint64_t r = splitmix(seed);
            const float unit = (float)((r >> 40) & 0xffffff) * 0x1p-24f;
            float l;
            switch (r & 15u) {
                case 0: l = 0.f; break;
                case 1: l = -unit * 0x1p-19f; break;              // rounds to -0.0 or -2^-19
                case 2: l = 1.f + (unit - 0.5f) * 0x1p-17f; break;   // around 1
                case 3: l = (unit - 0.5f) * 0x1p-17f; break;         // around 0
                case 4: l = (unit - 0.5f) * 8.f; break;
                case 5: l = (unit - 0.5f) * 0x1p40f; break;
                case 6: l = from_bits((uint32_t)(r >> 32)); break;
                default: l = unit; break;
            }
            q[c] = quantise(l);
        }
        check(q, (splitmix(seed) & 1u) != 0, rnd);
    }
    std::printf("random checked %llu predicate-differs %llu failed %llu\n", rnd.checked, rnd.pred_differs, rnd.failed);

    // (3) the boundary values in every position
    Tally edge;
    const float inf = std::numeric_limits<float>::infinity();
    const float edges[8] = {0.f, -0.f, 1.f, std::nextafterf(1.f, 2.f), ISC, std::numeric_limits<float>::quiet_NaN(), inf, -inf};
    for (float x : edges)
        for (float y : edges)
            for (float z : edges) {
                const float q[3] = {x, y, z};
                check(q, false, edge);
                check(q, true, edge);
            }
    std::printf("edges checked %llu predicate-differs %llu failed %llu\n", edge.checked, edge.pred_differs, edge.failed);

    // the sweep's three positions meet -0.0 once each, under both values of in_item
    const bool counts = sweep.pred_differs == 6 && edge.pred_differs > 0;
    if (!counts) std::printf("UNEXPECTED predicate-differs counts\n");
    const bool ok = counts && !sweep.failed && !rnd.failed && !edge.failed;
    std::printf("%s\n", ok ? "quant range ok" : "quant range FAILED");
    return ok ? 0 : 1;
}
