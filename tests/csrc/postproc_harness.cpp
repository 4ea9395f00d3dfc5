// Host build of postproc and postproc_single (lightpycl_amd/csrc/lpc_math.hpp),
// for tests/test_postproc_single_host.py.  Built with g++ -ffp-contract=off.
#include <cstdint>
#include <cstring>
#include <vector>

#include "lpc_math.hpp"

namespace {

struct Sweep {
    int32_t K;
    float max_ray_len;
    const float *t0s;
    int nt;
    long long cases = 0, fired = 0, bad = 0;
    int32_t first_bad[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // K, j0, prev, c0, t0 index, materials (5 per digit, low
                                                           //   slot first, first 13), what: 1 fields, 2 predicate
};

bool same(const lpc::PostOut &a, const lpc::PostOut &b)
{
    return a.hit_mesh == b.hit_mesh && a.hit_idx == b.hit_idx && a.n1 == b.n1 && a.n2 == b.n2 &&
           a.entering == b.entering && std::memcmp(&a.t_min, &b.t_min, 4) == 0;
}

// every j0, prev, count and t0 for one material table
// (reduced: prev in {-2, 0} and counts 0, 1 only -- one of each kind, one of each parity)
void sweep_materials(Sweep &S, const int32_t *mat, bool reduced = false)
{
    const int32_t K = S.K;
    const uint32_t refr = lpc::refr_mask(K, mat);
    for (int32_t j0 = 0; j0 < K; ++j0)
        for (int32_t prev = -2; prev < (reduced ? 1 : K); prev += reduced ? 2 : 1)
            for (int32_t c0 = 0; c0 <= (reduced ? 1 : 3); ++c0)
                for (int it = 0; it < S.nt; ++it) {
                    const float t0 = S.t0s[it];
                    // (a slot at max_ray_len holds the clean key: no triangle index)
                    const int32_t i0 = t0 < S.max_ray_len ? 7 + j0 : -1;
                    auto slot = [&](int32_t j, float &t, int32_t &c, int32_t &i) {
                        if (j == j0) { t = t0; c = c0; i = i0; }
                        else { t = S.max_ray_len; c = 0; i = -1; }
                    };
                    const lpc::PostOut g = lpc::postproc(K, prev, mat, S.max_ray_len, slot);
                    bool generic = false;
                    const lpc::PostOut s = lpc::postproc_single(prev, refr, S.max_ray_len, j0, t0, c0, i0, generic);
                    ++S.cases;
                    S.fired += generic;
                    const bool eq = same(g, s);
                    // the predicate fires exactly where the two differ; where it does
                    // not, they are equal field for field
                    if (generic == eq) {
                        if (!S.bad) {
                            int32_t code = 0;
                            for (int32_t j = (K < 13 ? K : 13) - 1; j >= 0; --j) code = code * 5 + mat[j];
                            const int32_t fb[8] = {K, j0, prev, c0, it, code, eq ? 2 : 1, 0};
                            std::memcpy(S.first_bad, fb, sizeof(fb));
                        }
                        ++S.bad;
                    }
                }
}

}  // namespace

extern "C" {

// The sweep of one K.  exhaustive != 0: every material table in {0..4}^K;
// otherwise the structured tables (a background type everywhere, one slot of
// each other type: sweep_materials runs every j0 over each) and `nrand` tables
// from a fixed linear congruential stream.
// out[0..2]: cases, cases where the predicate fired, violations; bad[8]: the first
// violation (see Sweep::first_bad).
void postproc_single_sweep(int32_t K, float max_ray_len, const float *t0s, int nt, int exhaustive, int nrand,
                           long long *out, int32_t *bad)
{
    Sweep S;
    S.K = K; S.max_ray_len = max_ray_len; S.t0s = t0s; S.nt = nt;
    std::vector<int32_t> mat((size_t)K, 0);
    if (exhaustive) {
        long long total = 1;
        for (int32_t j = 0; j < K; ++j) total *= 5;
        for (long long code = 0; code < total; ++code) {
            long long c = code;
            for (int32_t j = 0; j < K; ++j) { mat[(size_t)j] = (int32_t)(c % 5); c /= 5; }
            sweep_materials(S, mat.data());
        }
    } else {
        for (int32_t bg = 0; bg < 5; ++bg)
            for (int32_t ja = 0; ja < K; ++ja)
                for (int32_t ta = 0; ta < 5; ++ta) {
                    if (ta == bg && ja > 0) continue;                  // (the plain background table once)
                    for (int32_t j = 0; j < K; ++j) mat[(size_t)j] = bg;
                    mat[(size_t)ja] = ta;
                    sweep_materials(S, mat.data());
                }
        uint64_t x = 0x9e3779b97f4a7c15ull + (uint64_t)K;
        for (int r = 0; r < nrand; ++r) {
            for (int32_t j = 0; j < K; ++j) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                mat[(size_t)j] = (int32_t)((x >> 33) % 5);
            }
            sweep_materials(S, mat.data());
        }
    }
    out[0] = S.cases; out[1] = S.fired; out[2] = S.bad;
    std::memcpy(bad, S.first_bad, sizeof(S.first_bad));
}

// Every refractive / non-refractive pattern of one K, all 2^K of them: what
// postproc can tell apart in a material table (it reads it through
// `mt == 0 || mt == 4` alone).  A refractive slot is of type 0 or 4 by its parity,
// another of type 1, 2 or 3 by its index; every j0 and t0, prev in {-2, 0},
// counts 0 and 1.  out / bad as above.
void postproc_single_sweep_patterns(int32_t K, float max_ray_len, const float *t0s, int nt, long long *out,
                                    int32_t *bad)
{
    Sweep S;
    S.K = K; S.max_ray_len = max_ray_len; S.t0s = t0s; S.nt = nt;
    std::vector<int32_t> mat((size_t)K, 0);
    for (uint32_t pat = 0; pat < (1u << K); ++pat) {
        for (int32_t j = 0; j < K; ++j) mat[(size_t)j] = ((pat >> j) & 1u) ? ((j & 1) ? 4 : 0) : 1 + j % 3;
        sweep_materials(S, mat.data(), true);
    }
    out[0] = S.cases; out[1] = S.fired; out[2] = S.bad;
    std::memcpy(bad, S.first_bad, sizeof(S.first_bad));
}

}  // extern "C"
