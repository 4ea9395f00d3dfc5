// The host build of the scene records (lpc_build.hpp) as the runtime calls it,
// and a per-ray model of the walk over the records it returns, shared by
// build_harness.cpp (loaded by tests/test_build_host.py) and build_san_main.cpp
// (the same code under the sanitizers, a stand-alone program).
//
// The model visits what k_roots / trav_packet / sliver_group visit, one ray at a
// time: the nodes of a piece cut tested with their node_self record, the children
// of every passing node with the node's own child tests, Moller-Trumbore
// (mt_accumulate) on the passing leaf children through xorder, and the run's
// slivers through their line filter.  Every filter expression is the one of
// lpc_math.hpp; filter_test is also evaluated with explicit FMAs (what the device
// compiler may contract it to).
#pragma once
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "lpc_build.hpp"

namespace bm {

using namespace lpc;

struct Built {
    SceneBuildOut out;
    std::vector<int32_t> run_lo, run_hi;
    std::string err;
};

// runs of equal mesh id, as lpc_scene_upload forms them
static inline void form_runs(int32_t M, const int32_t *mesh_id, std::vector<int32_t> &run_lo, std::vector<int32_t> &run_hi)
{
    for (int32_t i = 0; i < M; ++i) {
        if (i == 0 || mesh_id[i] != mesh_id[i - 1]) { run_lo.push_back(i); run_hi.push_back(i + 1); }
        else run_hi.back() = i + 1;
    }
}

// fn(0) .. fn(n - 1) on `threads` host threads taking the next index in turn
static inline void parfor_threads(int threads, int n, const std::function<void(int)> &fn)
{
    if (threads <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next(0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&] {
            for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
        });
    for (auto &th : pool) th.join();
}

static inline void build(Built &B, int32_t M, const float *v0, const float *v1, const float *v2, const int32_t *mesh_id,
                         double dcap, double scene_scale, double thin_k, int stack_max, int threads)
{
    form_runs(M, mesh_id, B.run_lo, B.run_hi);
    SceneBuildIn in;
    in.v0 = v0; in.v1 = v1; in.v2 = v2;
    in.run_lo = B.run_lo.data(); in.run_hi = B.run_hi.data(); in.nr = B.run_lo.size();
    in.dcap = dcap; in.scene_scale = scene_scale; in.thin_k = thin_k; in.stack_max = stack_max;
    B.err = build_scene_records(in, B.out, [threads](int n, const std::function<void(int)> &fn) {
        parfor_threads(threads, n, fn);
    });
}

// filter_test with explicit FMAs
static inline float filter_test_fma(float cx, float cy, float cz, float negB, float negA, float ox, float oy, float oz,
                                    float nx, float ny, float nz)
{
    const float wx = cx - ox, wy = cy - oy, wz = cz - oz;
    const float px = fmaf(wy, nz, -(wz * ny)), py = fmaf(wz, nx, -(wx * nz)), pz = fmaf(wx, ny, -(wy * nx));
    const float pp = fmaf(pz, pz, fmaf(py, py, px * px));
    const float ww = fmaf(wz, wz, fmaf(wy, wy, wx * wx));
    return pp + fmaf(negB, ww, negA);
}

struct Hit {
    float t;
    int32_t idx, cnt;
    bool same(const Hit &o) const { return memcmp(&t, &o.t, 4) == 0 && idx == o.idx && cnt == o.cnt; }
};

struct Ray {
    f3 O, D;
    float nx, ny, nz, dl;
};

static inline Ray make_ray(const float *o4, const float *d4)
{
    Ray r;
    r.O = mk3(o4[0], o4[1], o4[2]);
    r.D = mk3(d4[0], d4[1], d4[2]);
    r.dl = sqrtf(d4[0] * d4[0] + d4[1] * d4[1] + d4[2] * d4[2]);      // sliver_group's dl
    const float u = 1.0f / r.dl;                                        // the kernels' unit_dir
    r.nx = d4[0] * u; r.ny = d4[1] * u; r.nz = d4[2] * u;
    return r;
}

struct Tri {
    const float *v0, *v1, *v2;
    void acc(const Ray &r, int32_t t, float eps, Hit &h) const
    {
        const float *a = v0 + 4 * (size_t)t, *b = v1 + 4 * (size_t)t, *c = v2 + 4 * (size_t)t;
        mt_accumulate(r.O, r.D, mk3(a[0], a[1], a[2]), mk3(b[0] - a[0], b[1] - a[1], b[2] - a[2]),
                      mk3(c[0] - a[0], c[1] - a[1], c[2] - a[2]), t, eps, h.t, h.idx, h.cnt);
    }
};

// the reference: every triangle of the run in index order
static inline Hit brute(const Tri &T, const Ray &r, int32_t lo, int32_t hi, float eps, float max_ray_len)
{
    Hit h = {max_ray_len, -1, 0};
    for (int32_t t = lo; t < hi; ++t) T.acc(r, t, eps, h);
    return h;
}

static inline float sphere_test(bool fused, float cx, float cy, float cz, float negB, float negA, const Ray &r)
{
    return fused ? filter_test_fma(cx, cy, cz, negB, negA, r.O.x, r.O.y, r.O.z, r.nx, r.ny, r.nz)
                 : filter_test(cx, cy, cz, negB, negA, r.O.x, r.O.y, r.O.z, r.nx, r.ny, r.nz);
}

// One run from the nodes of level `lv` of its level table (a piece cut).
// cut_half: the cut's own tests in the half-line form (filter_testh).  dmax: the
// largest |D| of the launch (a sliver whose dmin exceeds it is skipped, as
// sliver_group skips it).
static inline Hit model_run(const Built &B, const Tri &T, const Ray &r, size_t run, size_t lv, bool fused, bool cut_half,
                            float dmax, float eps, float max_ray_len)
{
    const SceneBuildOut &S = B.out;
    Hit h = {max_ray_len, -1, 0};
    const std::vector<int32_t> &L = S.run_levels[run];
    std::vector<int32_t> stack;
    if (!L.empty())
        for (int32_t i = 0; i < L[2 * lv + 1]; ++i) {
            const int32_t node = L[2 * lv] + i;
            const FiltRec &q = S.node_self[(size_t)node];
            const float d = cut_half ? filter_testh(q.cx, q.cy, q.cz, q.negB, q.negA, r.O.x, r.O.y, r.O.z, r.nx, r.ny, r.nz)
                                     : sphere_test(fused, q.cx, q.cy, q.cz, q.negB, q.negA, r);
            if (d <= 0.0f) stack.push_back(node);
        }
    while (!stack.empty()) {
        const Node8 &N = S.nodes[(size_t)stack.back()];
        stack.pop_back();
        const bool internal = N.ref[0] >= 0;                    // trav_packet's rule
        for (int k = 0; k < 8; ++k) {
            if (!(sphere_test(fused, N.cx[k], N.cy[k], N.cz[k], N.negB[k], N.negA[k], r) <= 0.0f)) continue;
            if (internal) stack.push_back(N.ref[k]);
            else T.acc(r, S.xorder[(size_t)~N.ref[k]], eps, h);
        }
    }
    for (int32_t j = S.run_slo[run]; j < S.run_shi[run]; ++j) {
        const SliverRec &R = S.slivers[(size_t)j];
        if (!(R.dmin <= dmax)) continue;
        const float tx = r.O.x - R.v0x, ty = r.O.y - R.v0y, tz = r.O.z - R.v0z;
        const float d = sliver_line_test<float>(R.e2x, R.e2y, R.e2z, R.a, R.b, tx, ty, tz, r.D.x, r.D.y, r.D.z, r.dl);
        if (!(d <= 0.0f)) continue;
        // the exact record in the triangle's own E1 / E2 order (ax1: e2 holds E1)
        const f3 Ea = mk3(R.e2x, R.e2y, R.e2z), Eb = mk3(R.e1x, R.e1y, R.e1z);
        mt_accumulate(r.O, r.D, mk3(R.v0x, R.v0y, R.v0z), R.ax1 ? Ea : Eb, R.ax1 ? Eb : Ea, R.idx, eps, h.t, h.idx, h.cnt);
    }
    return h;
}

struct WalkStats {
    long long mismatches = 0;       // (ray, run, cut, variant) results that differ from brute force
    long long compared = 0;         // how many were compared
    long long first_ray = -1, first_run = -1, first_cut = -1, first_variant = -1;
};

// Every ray against every run: brute force into bt / bi / bc ([ray][run]), and
// the model from every cut level, plain and fused (variants 0, 1), with `half`
// also with the half-line test at the cut (variants 2, 3).
static inline WalkStats model_walk(const Built &B, const float *v0, const float *v1, const float *v2, long long n,
                                   const float *o4, const float *d4, float max_ray_len, bool half, float *bt,
                                   int32_t *bi, int32_t *bc)
{
    WalkStats W;
    const Tri T = {v0, v1, v2};
    const float eps = 0.000001f * max_ray_len;
    const size_t nr = B.run_lo.size();
    double dmax2 = 0.0;                                     // host_dmax2 / run_intersect's dmax
    for (long long i = 0; i < n; ++i) {
        const float *d = d4 + 4 * i;
        const double q = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
        if (!(q <= dmax2)) dmax2 = q;
    }
    if (!(dmax2 >= 0.0)) dmax2 = INFINITY;
    const float dmax = (float)std::min<double>(sqrt(dmax2 * (1.0 + 1e-5)), (double)INFINITY);
    // blocks of rays on a few host threads, merged in ray order
    const long long blk = 256, nblk = (n + blk - 1) / blk;
    std::vector<WalkStats> part((size_t)nblk);
    const int threads = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    parfor_threads(threads, (int)nblk, [&](int b) {
        WalkStats &P = part[(size_t)b];
        for (long long i = b * blk; i < std::min(n, (b + 1) * blk); ++i) {
            const Ray r = make_ray(o4 + 4 * i, d4 + 4 * i);
            for (size_t run = 0; run < nr; ++run) {
                const Hit want = brute(T, r, B.run_lo[run], B.run_hi[run], eps, max_ray_len);
                bt[(size_t)i * nr + run] = want.t; bi[(size_t)i * nr + run] = want.idx; bc[(size_t)i * nr + run] = want.cnt;
                const size_t nlv = std::max<size_t>(1, B.out.run_levels[run].size() / 2);
                for (size_t lv = 0; lv < nlv; ++lv)
                    for (int variant = 0; variant < (half ? 4 : 2); ++variant) {
                        const Hit got = model_run(B, T, r, run, lv, (variant & 1) != 0, (variant & 2) != 0, dmax, eps,
                                                  max_ray_len);
                        ++P.compared;
                        if (!got.same(want)) {
                            if (!P.mismatches) { P.first_ray = i; P.first_run = (long long)run; P.first_cut = (long long)lv; P.first_variant = variant; }
                            ++P.mismatches;
                        }
                    }
            }
        }
    });
    for (const WalkStats &P : part) {
        if (!W.mismatches && P.mismatches) { W.first_ray = P.first_ray; W.first_run = P.first_run; W.first_cut = P.first_cut; W.first_variant = P.first_variant; }
        W.mismatches += P.mismatches;
        W.compared += P.compared;
    }
    return W;
}

}  // namespace bm
