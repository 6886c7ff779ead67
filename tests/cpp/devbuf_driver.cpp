// devbuf_driver.cpp -- csrc/rt_devbuf.h on the CPU, under ASan + UBSan with leak detection
// (raytracingproject_amd.build.build_devbuf; run by tests/test_devbuf.py).
//
// The three HIP calls DevBuf makes are defined here as counting fakes over malloc: a set of
// the live blocks, the sizes asked for, a switch that fails the k-th allocation, and a count of
// frees of pointers the fake never handed out (or handed out and already took back).  No HIP
// library is linked.  Prints "devbuf checks N failed F"; exit status 1 where F > 0.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "rt_devbuf.h"

namespace {
std::map<void*, size_t> g_live;    // block -> bytes asked for
int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
int g_fail_at = 0;                 // the g_fail_at-th allocation from now fails (0: none)
int g_checks = 0, g_failed = 0;
}  // namespace

hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_at > 0 && --g_fail_at == 0) {
        *p = reinterpret_cast<void*>(0x1);   // (a failed call's output is not to be relied on)
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    g_live[*p] = bytes;
    ++g_mallocs;
    return hipSuccess;
}

hipError_t hipFree(void* p) {
    const auto it = g_live.find(p);
    if (it == g_live.end()) {
        ++g_bad_frees;
        return hipErrorInvalidValue;
    }
    g_live.erase(it);
    std::free(p);
    ++g_frees;
    return hipSuccess;
}

const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "ok" : "fake error"; }

#define CHECK(cond)                                                       \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            ++g_failed;                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                 \
    } while (0)

using rtx::DevBuf;

// the shape of rt_ctx::Scene: several buffers and plain facts, forgotten by assigning a new one
struct Record {
    DevBuf a, b, c;
    int n = 0;
    float box[6] = {};
};

static bool live(const void* p, size_t bytes) {
    const auto it = g_live.find(const_cast<void*>(p));
    return it != g_live.end() && it->second == bytes;
}

int main() {
    {   // reserve: kept for an equal or smaller request, replaced for a larger one
        DevBuf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(100) == hipSuccess && b.cap == 100 && live(b.p, 100));
        void* p = b.p;
        CHECK(b.reserve(100) == hipSuccess && b.p == p && b.cap == 100);
        CHECK(b.reserve(40) == hipSuccess && b.p == p && b.cap == 100);
        CHECK(g_mallocs == 1 && g_frees == 0);
        CHECK(b.reserve(101) == hipSuccess && b.cap == 101 && live(b.p, 101) && !live(p, 100));
        CHECK(g_mallocs == 2 && g_frees == 1 && g_live.size() == 1);
        CHECK(b.as<char>() == static_cast<char*>(b.p) && b.as<const double>() == static_cast<const double*>(b.p));
        CHECK(b.reset() == hipSuccess && b.p == nullptr && b.cap == 0 && g_live.empty());
        CHECK(b.reset() == hipSuccess && g_frees == 2 && g_bad_frees == 0);   // (nothing to free: no call)
    }
    CHECK(g_live.empty() && g_mallocs == 2 && g_frees == 2);
    {   // an empty request holds 16 bytes at cap 0, and the next empty request keeps them
        DevBuf b;
        CHECK(b.reserve(0) == hipSuccess && b.p != nullptr && b.cap == 0 && live(b.p, 16));
        void* p = b.p;
        const int m = g_mallocs;
        CHECK(b.reserve(0) == hipSuccess && b.p == p && b.cap == 0 && g_mallocs == m);
        CHECK(b.reserve(1) == hipSuccess && b.cap == 1 && live(b.p, 1) && g_mallocs == m + 1 && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // a failed allocation: empty, the error returned, the old block gone; the next one succeeds
        DevBuf b;
        CHECK(b.reserve(32) == hipSuccess);
        g_fail_at = 1;
        CHECK(b.reserve(64) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && g_live.empty());
        CHECK(b.reserve(64) == hipSuccess && b.cap == 64 && live(b.p, 64));
        DevBuf fresh;
        g_fail_at = 1;
        CHECK(fresh.reserve(8) == hipErrorOutOfMemory && fresh.p == nullptr && fresh.cap == 0);
        g_fail_at = 2;   // (the switch counts calls: the second from here)
        CHECK(fresh.reserve(8) == hipSuccess && live(fresh.p, 8));
        CHECK(fresh.reserve(9) == hipErrorOutOfMemory && fresh.p == nullptr && fresh.cap == 0);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
    {   // moves empty their source; move assignment frees what the target held, once
        DevBuf a;
        CHECK(a.reserve(24) == hipSuccess);
        void* pa = a.p;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 24 && g_live.size() == 1);
        DevBuf t;
        CHECK(t.reserve(48) == hipSuccess);
        void* pt = t.p;
        const int f = g_frees;
        t = std::move(b);
        CHECK(b.p == nullptr && b.cap == 0 && t.p == pa && t.cap == 24);
        CHECK(g_frees == f + 1 && !live(pt, 48) && live(pa, 24) && g_live.size() == 1);
        DevBuf& self = t;
        t = std::move(self);   // (self-assignment keeps the block)
        CHECK(t.p == pa && t.cap == 24 && g_frees == f + 1);
        DevBuf empty;
        t = std::move(empty);  // (from an empty one: freed, empty)
        CHECK(t.p == nullptr && t.cap == 0 && g_frees == f + 2 && g_live.empty());
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
    {   // a record of several, assigned from a default-constructed one: each block freed once
        Record r;
        CHECK(r.a.reserve(10) == hipSuccess && r.b.reserve(0) == hipSuccess && r.c.reserve(30) == hipSuccess);
        r.n = 7, r.box[5] = 1.f;
        CHECK(g_live.size() == 3);
        const int f = g_frees;
        r = Record{};
        CHECK(g_frees == f + 3 && g_live.empty() && g_bad_frees == 0);
        CHECK(r.a.p == nullptr && r.b.p == nullptr && r.c.p == nullptr && r.c.cap == 0 && r.n == 0 && r.box[5] == 0.f);
        // filled aside, then moved in: the record's old blocks go, the new ones are kept
        CHECK(r.a.reserve(5) == hipSuccess);
        Record up;
        CHECK(up.a.reserve(11) == hipSuccess && up.c.reserve(12) == hipSuccess);
        up.n = 3;
        void *ua = up.a.p, *uc = up.c.p;
        r = std::move(up);
        CHECK(r.a.p == ua && r.c.p == uc && r.b.p == nullptr && r.n == 3 && up.a.p == nullptr && up.c.p == nullptr);
        CHECK(g_live.size() == 2 && live(ua, 11) && live(uc, 12));
    }
    // at exit: nothing live, every free was of a block handed out, as many frees as allocations
    CHECK(g_live.empty());
    CHECK(g_bad_frees == 0);
    CHECK(g_mallocs == g_frees && g_mallocs > 0);
    std::printf("devbuf checks %d failed %d mallocs %d frees %d bad_frees %d live %zu\n", g_checks, g_failed, g_mallocs,
                g_frees, g_bad_frees, g_live.size());
    return g_failed ? 1 : 0;
}
