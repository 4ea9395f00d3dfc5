// Host build of postproc<KU> and shade (lightpycl_amd/csrc/lpc_math.hpp) on rows
// the caller enumerates, for tests/test_postproc_tables_host.py and the host leg
// of tests/shade_rows.py.  Built with g++ -ffp-contract=off.
#include <cstdint>
#include <cstring>

#include "lpc_math.hpp"

namespace {

// One row's slots as the shading kernels hold them: slots j < K from the row,
// slots K <= j < KU in the clean state (shade_post, lpc_kernels.hip).
struct Row {
    int32_t K;
    float max_ray_len;
    const float *t;
    const int32_t *cnt, *idx;
    void operator()(int32_t j, float &tj, int32_t &cj, int32_t &ij) const
    {
        if (j < K) { tj = t[j]; cj = cnt[j]; ij = idx[j]; }
        else { tj = max_ray_len; cj = 0; ij = -1; }
    }
};

void put(int32_t *out, const lpc::PostOut &o)
{
    out[0] = o.hit_mesh; out[1] = o.hit_idx; out[2] = o.n1; out[3] = o.n2; out[4] = o.entering;
    std::memcpy(out + 5, &o.t_min, 4);
}

template <int KU>
void run_ku(int64_t n, int32_t K, float mrl, const int32_t *prev, const int32_t *mat, const float *t,
            const int32_t *cnt, const int32_t *idx, int32_t *out)
{
    for (int64_t r = 0; r < n; ++r) {
        const Row row{K, mrl, t + r * K, cnt + r * K, idx + r * K};
        put(out + 6 * r, lpc::postproc<KU>(K, prev[r], mat + r * K, mrl, row));
    }
}

}  // namespace

// The KU with_ku (lpc_runtime.hip) picks for K meshes.
extern "C" int32_t postproc_tables_ku(int32_t K) { return K <= 4 ? 4 : K <= 8 ? 8 : K <= 12 ? 12 : K <= 16 ? 16 : 0; }

// n rows of K slots each, [row][slot]; mat is per row.  out0: postproc<0>, outku:
// postproc<postproc_tables_ku(K)>; six int32 per row (hit_mesh, hit_idx, n1, n2,
// entering, the bits of t_min).
extern "C" void postproc_tables(int64_t n, int32_t K, float mrl, const int32_t *prev, const int32_t *mat,
                                const float *t, const int32_t *cnt, const int32_t *idx, int32_t *out0,
                                int32_t *outku)
{
    run_ku<0>(n, K, mrl, prev, mat, t, cnt, idx, out0);
    switch (postproc_tables_ku(K)) {
    case 4: run_ku<4>(n, K, mrl, prev, mat, t, cnt, idx, outku); break;
    case 8: run_ku<8>(n, K, mrl, prev, mat, t, cnt, idx, outku); break;
    case 12: run_ku<12>(n, K, mrl, prev, mat, t, cnt, idx, outku); break;
    case 16: run_ku<16>(n, K, mrl, prev, mat, t, cnt, idx, outku); break;
    default: run_ku<0>(n, K, mrl, prev, mat, t, cnt, idx, outku); break;
    }
}

// shade() on n rows in the drop-in kernels' layouts ((n,4) float rows; vertices
// as three (M,4) arrays).  pow and meas are updated in place; the children's
// directions go to r_dir / t_dir as (n,4) rows with w = 0.
extern "C" void shade_rows(int64_t n, const float *origin, const float *dest, const float *dir, float *pow,
                           int32_t *meas, const int32_t *n1, const int32_t *n2, const int32_t *imid,
                           const int32_t *iidx, const float *v0, const float *v1, const float *v2,
                           const int32_t *mat, const float *ior, const float *refl, const float *diss,
                           float ior_env, float *r_dir, float *r_pow, int32_t *r_meas, float *t_dir,
                           float *t_pow, int32_t *t_meas)
{
    using lpc::f3;
    auto ld = [](const float *p) { return lpc::mk3(p[0], p[1], p[2]); };
    auto tri = [&](int32_t i, f3 &a, f3 &b, f3 &c) {
        a = ld(v0 + 4 * (int64_t)i); b = ld(v1 + 4 * (int64_t)i); c = ld(v2 + 4 * (int64_t)i);
    };
    for (int64_t r = 0; r < n; ++r) {
        const lpc::ShadeOut s = lpc::shade(ld(origin + 4 * r), ld(dir + 4 * r), ld(dest + 4 * r), pow[r], meas[r],
                                           imid[r], iidx[r], n1[r], n2[r], mat, ior, refl, diss, ior_env, tri);
        pow[r] = s.pow; meas[r] = s.meas;
        r_dir[4 * r] = s.r_dir.x; r_dir[4 * r + 1] = s.r_dir.y; r_dir[4 * r + 2] = s.r_dir.z; r_dir[4 * r + 3] = 0.0f;
        t_dir[4 * r] = s.t_dir.x; t_dir[4 * r + 1] = s.t_dir.y; t_dir[4 * r + 2] = s.t_dir.z; t_dir[4 * r + 3] = 0.0f;
        r_pow[r] = s.r_pow; t_pow[r] = s.t_pow; r_meas[r] = s.r_meas; t_meas[r] = s.t_meas;
    }
}
