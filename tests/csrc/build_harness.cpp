// CPU harness for lpc_build.hpp: build_scene_records on the runs lpc_scene_upload
// forms, its records as arrays, and the model walk of build_model.hpp over them
// (tests/test_build_host.py).
#include "build_model.hpp"

using namespace bm;

// -> a handle (never NULL; bh_error tells whether the build was refused)
extern "C" void *bh_build(int M, const float *v0, const float *v1, const float *v2, const int32_t *mesh_id, double dcap,
                          double scene_scale, double thin_k, int stack_max, int threads)
{
    Built *B = new Built();
    build(*B, M, v0, v1, v2, mesh_id, dcap, scene_scale, thin_k, stack_max, threads);
    return B;
}

extern "C" void bh_free(void *h) { delete (Built *)h; }

extern "C" const char *bh_error(void *h) { return ((Built *)h)->err.c_str(); }

// [0] nodes [1] slivers [2] xorder entries [3] runs [4] level-table words over
// all runs [5] n_slivers [6] n_thin [7] sizeof(Node8) [8] sizeof(SliverRec)
// [9] sizeof(FiltRec)
extern "C" void bh_sizes(void *h, long long *out)
{
    const Built &B = *(Built *)h;
    size_t lw = 0;
    for (const auto &l : B.out.run_levels) lw += l.size();
    out[0] = (long long)B.out.nodes.size(); out[1] = (long long)B.out.slivers.size();
    out[2] = (long long)B.out.xorder.size(); out[3] = (long long)B.run_lo.size(); out[4] = (long long)lw;
    out[5] = B.out.n_slivers; out[6] = B.out.n_thin;
    out[7] = sizeof(Node8); out[8] = sizeof(SliverRec); out[9] = sizeof(FiltRec);
}

// The records, each into a buffer of the size bh_sizes gives.  level_off: per run
// the first word of its level table in `levels` (runs + 1 entries).
extern "C" void bh_records(void *h, void *nodes, void *node_self, void *slivers, int32_t *xorder, int32_t *run_lo,
                           int32_t *run_hi, int32_t *run_slo, int32_t *run_shi, int32_t *levels, int32_t *level_off)
{
    const Built &B = *(Built *)h;
    const SceneBuildOut &S = B.out;
    if (!S.nodes.empty()) memcpy(nodes, S.nodes.data(), S.nodes.size() * sizeof(Node8));
    if (!S.node_self.empty()) memcpy(node_self, S.node_self.data(), S.node_self.size() * sizeof(FiltRec));
    if (!S.slivers.empty()) memcpy(slivers, S.slivers.data(), S.slivers.size() * sizeof(SliverRec));
    if (!S.xorder.empty()) memcpy(xorder, S.xorder.data(), S.xorder.size() * 4);
    const size_t nr = B.run_lo.size();
    int32_t off = 0;
    for (size_t r = 0; r < nr; ++r) {
        run_lo[r] = B.run_lo[r]; run_hi[r] = B.run_hi[r];
        // a refused build returns before the later runs' tables exist
        run_slo[r] = r < S.run_slo.size() ? S.run_slo[r] : 0;
        run_shi[r] = r < S.run_shi.size() ? S.run_shi[r] : 0;
        level_off[r] = off;
        if (r < S.run_levels.size())
            for (int32_t w : S.run_levels[r]) levels[off++] = w;
    }
    level_off[nr] = off;
}

// Each triangle on its own, by the rules build_run applies: 0 hierarchy, 1 never,
// 2 sliver (a degenerate sphere test), 3 thin (the line filter bounds it better).
extern "C" void bh_classify(int M, const float *v0, const float *v1, const float *v2, double dcap, double scene_scale,
                            double thin_k, int32_t *cls)
{
    for (int t = 0; t < M; ++t) {
        const float *a = v0 + 4 * (size_t)t, *b = v1 + 4 * (size_t)t, *c = v2 + 4 * (size_t)t;
        const FiltRec f = filter_record(a, b, c, t, dcap, scene_scale);
        if (f.negA == INFINITY) cls[t] = 1;
        else if (f.negB < -1e29f) cls[t] = 2;
        else cls[t] = thin_axis(a, b, c, f.cx, f.cy, f.cz, scene_scale, thin_k) ? 3 : 0;
    }
}

// One record's test for rays (n,4): kind 0 filter_test, 1 with explicit FMAs,
// 2 filter_testh.  (The padded children of a node pass for no ray.)
extern "C" void bh_sphere_eval(int kind, float cx, float cy, float cz, float negB, float negA, long long n,
                               const float *o4, const float *d4, float *out)
{
    for (long long i = 0; i < n; ++i) {
        const Ray r = make_ray(o4 + 4 * i, d4 + 4 * i);
        out[i] = kind == 2 ? filter_testh(cx, cy, cz, negB, negA, r.O.x, r.O.y, r.O.z, r.nx, r.ny, r.nz)
                           : sphere_test(kind == 1, cx, cy, cz, negB, negA, r);
    }
}

// The model walk against brute force.  stats: [0] mismatches [1] compared
// [2..5] the first mismatch (ray, run, cut level, variant); bt / bi / bc: brute
// force per [ray][run].
extern "C" void bh_model_walk(void *h, const float *v0, const float *v1, const float *v2, long long n, const float *o4,
                              const float *d4, float max_ray_len, int half, long long *stats, float *bt, int32_t *bi,
                              int32_t *bc)
{
    const WalkStats W = model_walk(*(Built *)h, v0, v1, v2, n, o4, d4, max_ray_len, half != 0, bt, bi, bc);
    stats[0] = W.mismatches; stats[1] = W.compared; stats[2] = W.first_ray; stats[3] = W.first_run;
    stats[4] = W.first_cut; stats[5] = W.first_variant;
}
