// cand_depth_driver.cpp -- the near bound of csrc/rt_batch_cull.h (cull_near, the packed list
// word and its order) against brute force.
//
// Usage: cand_depth_driver CASES.bin    (written by tests/test_cand_depth.py; the case format
// is batch_cull_driver.cpp's)
//
// For every 8x8 tile of a case's image (edge tiles included) the driver takes the tile's
// candidates as the kernel does (cull_beam once, cull_keep per record) and each candidate's
// near bound, raw (cull_near) and as the list word carries it (cand_pack / cand_near).  It then
// generates the tile's camera rays from camera_ray_lds' formulas -- the uniforms at their
// extremes (jitter +-0.5, the lens rim, time 0 and 1 - 2^-24) and at random -- rounds origin
// and direction to the fp32 values the kernel traces, and computes the root the kernel's fp32
// sphere test reports (rt_device.h sphere_root, not self, tmin 0.001, no tmax) the ways the
// compiled kernel may: with and without fused multiply-adds, and with the reciprocals and the
// square root exact or moved two ulp either way (the device's approximate rcp / sqrt).  Every
// reported root must be at least both bounds.  Per tile whose list fits the cap the places
// cand_rank gives the words must be a permutation that orders them by (near, index).
//
// Exit status 0: no root below a bound, every list ordered; 1 otherwise.  Built with
// -DRT_CULL_MUTATE=1..4 (no margins, no lens radius, no motion half-length, the packed bound
// rounded up) the bound is wrong on purpose and the driver must exit 1.
#include <algorithm>
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
V ld(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }

float nudge(float x, int ulps) {
    for (int i = 0; i < std::abs(ulps); ++i) x = std::nextafterf(x, ulps > 0 ? INFINITY : -INFINITY);
    return x;
}

// sphere_root<float, false, SELECT> (rt_device.h), not self, over (0.001, inf): FMA: products
// fused into the sums that take them; ULPS: rcp and sqrt results moved by that many ulp
template <bool FMA>
bool root32(const SphereF& s, const float o[3], const float d[3], float time, int ulps, float& t) {
    auto mad = [](float a, float b, float c) { return FMA ? std::fmaf(a, b, c) : a * b + c; };
    auto dot = [&](const float* a, const float* b) { return mad(a[2], b[2], mad(a[1], b[1], a[0] * b[0])); };
    float f[3], l[3];
    for (int k = 0; k < 3; ++k) f[k] = o[k] - mad(time, s.cv[k], s.c[k]);
    const float a = dot(d, d), inv_a = nudge(1.f / a, ulps);
    const float b = -dot(f, d);
    const float u = b * inv_a;
    for (int k = 0; k < 3; ++k) l[k] = mad(u, d[k], f[k]);
    const float r2 = s.r * s.r;
    const float disc = r2 - dot(l, l);
    if (disc < 0) return false;
    const float cc = dot(f, f) - r2;
    const float q = b + std::copysign(nudge(std::sqrt(a * disc), ulps), b);
    const float ta = cc * nudge(1.f / q, ulps), tb = q * inv_a;
    const float t0 = std::fmin(ta, tb), t1 = std::fmax(ta, tb);
    t = 0.001f < t0 ? t0 : t1;
    return 0.001f < t && t < INFINITY;
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
        if (h.magic != MAGIC || h.n < 0 || h.n > (int)CAND_IDX_MASK + 1 || h.W < 1 || h.H < 1) {
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
        long ntiles = 0, nrays = 0, nroots = 0, nbelow = 0, npos = 0, ncand = 0, nsort = 0, nsort_bad = 0;
        double gap_min = INFINITY;   // the least root / bound - 1 seen
        std::vector<int> cand;
        std::vector<float> near_raw, near_word;
        std::vector<uint32_t> words, placed;
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const int tx0 = tx * 8, ty0 = ty * 8;
                const CullBeam bm = cull_beam(h.cam, h.defocus, tx0, ty0);
                cand.clear();
                near_raw.clear();
                near_word.clear();
                words.clear();
                for (int k = 0; k < h.n; ++k)
                    if (cull_keep(bm, sph[(size_t)k])) {
                        const float nr = cull_near(bm, sph[(size_t)k]);
                        const uint32_t w = cand_pack(nr, (uint32_t)k);
                        if (!(nr >= 0.f) || cand_index(w) != (uint32_t)k || (RT_CULL_MUTATE != 4 && !(cand_near(w) <= nr))) {
                            if (nbelow < 5) printf("  BAD WORD %s: sphere %d bound %g word %08x\n", h.name, k, (double)nr, w);
                            ++nbelow;
                        }
                        words.push_back(w);
                        if (cand_near(w) > 0.f || nr > 0.f) {   // (a bound of 0 holds for every root)
                            cand.push_back(k);
                            near_raw.push_back(nr);
                            near_word.push_back(cand_near(w));
                        }
                    }
                ++ntiles;
                ncand += (long)words.size();
                npos += (long)cand.size();
                if (!words.empty() && words.size() <= (size_t)BATCH_CAND_CAP) {
                    // the kernel's sort: word i goes to place cand_rank(i)
                    const uint32_t n = (uint32_t)words.size();
                    placed.assign(n, 0xffffffffu);
                    bool ok = true;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint32_t r = cand_rank(words.data(), n, words[i]);
                        if (r >= n || placed[r] != 0xffffffffu)
                            ok = false;
                        else
                            placed[r] = words[i];
                    }
                    for (uint32_t i = 0; ok && i + 1 < n; ++i) {
                        const float n0 = cand_near(placed[i]), n1 = cand_near(placed[i + 1]);
                        ok = n0 < n1 || (n0 == n1 && cand_index(placed[i]) < cand_index(placed[i + 1]));
                    }
                    std::vector<uint32_t> a(words), b(placed);
                    std::sort(a.begin(), a.end());
                    std::sort(b.begin(), b.end());
                    ok = ok && a == b;
                    ++nsort;
                    if (!ok) {
                        if (nsort_bad < 5) printf("  UNSORTED %s: tile (%d, %d), %u words\n", h.name, tx0, ty0, n);
                        ++nsort_bad;
                    }
                }
                if (cand.empty()) continue;
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
                            const float of[3] = {(float)o.x, (float)o.y, (float)o.z};
                            const float df[3] = {(float)d.x, (float)d.y, (float)d.z};
                            for (int ti = 0; ti < 2; ++ti) {
                                const float time = (float)(ti ? rng.next() * (1.0 - 0x1p-24)
                                                              : ((ji + li + q) & 1) ? 1.0 - 0x1p-24 : 0.0);
                                ++nrays;
                                for (size_t ci = 0; ci < cand.size(); ++ci) {
                                    const SphereF& s = sph[(size_t)cand[ci]];
                                    for (int var = 0; var < 6; ++var) {
                                        float t;
                                        const int ulps = (var >> 1) * 2 - 2;
                                        const bool hit = (var & 1) ? root32<true>(s, of, df, time, ulps, t)
                                                                   : root32<false>(s, of, df, time, ulps, t);
                                        if (!hit) continue;
                                        ++nroots;
                                        const float bound = std::fmax(near_raw[ci], near_word[ci]);
                                        if (bound > 0.f) gap_min = std::fmin(gap_min, (double)t / (double)bound - 1.0);
                                        if (!(near_raw[ci] <= t && near_word[ci] <= t)) {
                                            if (nbelow < 5)
                                                printf("  BELOW %s: tile (%d, %d) pixel %d sphere %d (r %g) time %g: root %.9g "
                                                       "bound %.9g word %.9g\n",
                                                       h.name, tx0, ty0, q, cand[ci], (double)s.r, (double)time, (double)t,
                                                       (double)near_raw[ci], (double)near_word[ci]);
                                            ++nbelow;
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        printf("%-30s %dx%d n %d tiles %ld rays %ld cand %ld bounded %ld roots %ld least gap %.3g lists %ld unsorted %ld "
               "below %ld\n",
               h.name, h.W, h.H, h.n, ntiles, nrays, ncand, npos, nroots, gap_min, nsort, nsort_bad, nbelow);
        if (nbelow || nsort_bad) ++bad;
    }
    fclose(f);
    printf("%d cases, %d failed (RT_CULL_MUTATE %d)\n", ncases, bad, RT_CULL_MUTATE);
    return bad || !ncases ? 1 : 0;
}
