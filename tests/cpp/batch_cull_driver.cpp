// batch_cull_driver.cpp -- the tile / sphere cull of csrc/rt_batch_cull.h against brute force.
//
// Usage: batch_cull_driver CASES.bin    (written by tests/test_batch_cull.py)
//
// A case is a camera (the 18 fp32 words of CohConst::cam, the defocus flag, the image size)
// and a list of SphereF records.  For every 8x8 tile of the image (edge tiles included) the
// driver takes the tile's candidate set from the predicate exactly as the kernel does
// (cull_beam once per tile, cull_keep per record), generates the tile's camera rays in fp64
// from camera_ray_lds' formulas -- the uniforms at their extremes (jitter +-0.5, the lens rim,
// time 0 and 1 - 2^-24) and at random -- and tests every sphere that is NOT a candidate in
// fp64 (sphere.h:30-57, roots in (0.001, inf)): a hit there is a sphere the kernel would miss.
// Mode 1 cases only count candidates per tile (the benchmark view's condition on the cap).
//
// Exit status 0: no sphere missed and every condition met; 1 otherwise.  Built with
// -DRT_CULL_MUTATE=1..3 the predicate is wrong on purpose and the driver must exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_batch_cull.h"

using namespace rtx;

namespace {

struct CaseHdr {
    int32_t magic, W, H, defocus, n, mode, over_permille_max, pad;
    char name[32];
    float cam[18];
};
static_assert(sizeof(CaseHdr) == 32 + 32 + 72, "CaseHdr");
constexpr int32_t MAGIC = 0x4c4c5543;   // "CULL"

struct Rng {   // xorshift64*: the driver's own stream
    uint64_t s;
    double next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return (double)((s * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53;
    }
};

struct V {
    double x, y, z;
};
V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V operator*(double s, V a) { return {s * a.x, s * a.y, s * a.z}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V ld(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }

// sphere.h:30-57 in fp64: any root in (0.001, inf)
bool hits(const SphereF& s, V o, V d, double time) {
    const V center = ld(s.c) + time * ld(s.cv);
    const V oc = o - center;
    const double a = dot(d, d), hb = dot(oc, d), c = dot(oc, oc) - (double)s.r * (double)s.r;
    const double disc = hb * hb - a * c;
    if (!(disc >= 0)) return false;
    const double sq = std::sqrt(disc);
    return (-hb - sq) / a > 0.001 || (-hb + sq) / a > 0.001;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    int bad = 0, ncases = 0;
    CaseHdr h;
    while (fread(&h, sizeof(h), 1, f) == 1) {
        if (h.magic != MAGIC || h.n < 0 || h.n > (1 << 20) || h.W < 1 || h.H < 1) {
            fprintf(stderr, "bad case header\n");
            return 2;
        }
        h.name[31] = 0;
        std::vector<SphereF> sph((size_t)h.n);
        if (h.n && fread(sph.data(), sizeof(SphereF), (size_t)h.n, f) != (size_t)h.n) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        ++ncases;
        const V c = ld(h.cam), p00 = ld(h.cam + 3), du = ld(h.cam + 6), dv = ld(h.cam + 9), ddu = ld(h.cam + 12),
                ddv = ld(h.cam + 15);
        Rng rng{0x9E3779B97F4A7C15ull ^ (uint64_t)ncases};
        const int tiles_x = (h.W + 7) / 8, tiles_y = (h.H + 7) / 8;
        long ntiles = 0, nrays = 0, nmiss = 0, ncand_sum = 0, nover = 0, nempty = 0;
        int cand_max = 0;
        std::vector<char> keep((size_t)h.n);
        std::vector<int> rest;
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const int tx0 = tx * 8, ty0 = ty * 8;
                const CullBeam bm = cull_beam(h.cam, h.defocus, tx0, ty0);
                int nc = 0;
                rest.clear();
                for (int k = 0; k < h.n; ++k) {
                    keep[(size_t)k] = cull_keep(bm, sph[(size_t)k]);
                    if (keep[(size_t)k])
                        ++nc;
                    else
                        rest.push_back(k);
                }
                ++ntiles;
                ncand_sum += nc;
                cand_max = nc > cand_max ? nc : cand_max;
                nover += nc > BATCH_CAND_CAP;
                nempty += nc == 0;
                if (h.mode == 1 || rest.empty()) continue;
                for (int q = 0; q < 64; ++q) {
                    const int px = tx0 + (q & 7), py = ty0 + (q >> 3);
                    if (px >= h.W || py >= h.H) continue;
                    const V pc = p00 + (double)px * du + (double)py * dv;
                    // jitter: the four corners and a random one; lens: two opposite rim points
                    // (turned from pixel to pixel and corner to corner) and a random one; time: one
                    // of its two ends (alternating) and a random one
                    for (int ji = 0; ji < 5; ++ji) {
                        const double jx = ji < 4 ? ((ji & 1) ? 0.5 : -0.5) : rng.next() - 0.5;
                        const double jy = ji < 4 ? ((ji & 2) ? 0.5 : -0.5) : rng.next() - 0.5;
                        const V ps = pc + (jx * du + jy * dv);
                        const int nl = h.defocus ? 3 : 1;
                        for (int li = 0; li < nl; ++li) {
                            V o = c;
                            if (h.defocus) {
                                double lx, ly;
                                if (li < 2) {
                                    const double th = 6.283185307179586 * ((double)li / 2 + (double)q / 64 + (double)ji / 10);
                                    lx = std::cos(th);
                                    ly = std::sin(th);
                                } else {
                                    do {
                                        lx = 2 * rng.next() - 1;
                                        ly = 2 * rng.next() - 1;
                                    } while (!(lx * lx + ly * ly < 1));
                                }
                                o = c + lx * ddu + ly * ddv;
                            }
                            const V d = ps - o;
                            for (int ti = 0; ti < 2; ++ti) {
                                const double time = ti ? rng.next() : ((ji + li + q) & 1) ? 1.0 - 0x1p-24 : 0.0;
                                ++nrays;
                                for (int k : rest)
                                    if (hits(sph[(size_t)k], o, d, time)) {
                                        if (nmiss < 5)
                                            printf("  MISSING %s: tile (%d, %d) pixel %d sphere %d (r %g) time %g\n", h.name,
                                                   tx0, ty0, q, k, (double)sph[(size_t)k].r, time);
                                        ++nmiss;
                                    }
                            }
                        }
                    }
                }
            }
        const double over = ntiles ? 1000.0 * (double)nover / (double)ntiles : 0;
        printf("%-30s %dx%d n %d tiles %ld rays %ld cand mean %.2f max %d empty %.1f%% over-cap %.2f%% missing %ld\n", h.name,
               h.W, h.H, h.n, ntiles, nrays, ntiles ? (double)ncand_sum / (double)ntiles : 0.0, cand_max,
               ntiles ? 100.0 * (double)nempty / (double)ntiles : 0.0, over / 10, nmiss);
        if (nmiss) ++bad;
        if (h.over_permille_max >= 0 && over > (double)h.over_permille_max) {
            printf("  FAIL %s: %.2f%% of tiles over the cap of %d (at most %.1f%%)\n", h.name, over / 10, BATCH_CAND_CAP,
                   h.over_permille_max / 10.0);
            ++bad;
        }
    }
    fclose(f);
    printf("%d cases, %d failed (RT_CULL_MUTATE %d)\n", ncases, bad, RT_CULL_MUTATE);
    return bad || !ncases ? 1 : 0;
}
