// Host build of the device-born light sources' arithmetic shared with the HIP
// kernels (lightpycl_amd/csrc/lpc_emit.hpp), for tests/test_emit_host.py.
// Built with g++ -ffp-contract=off.  The loops here stand in for the kernels'
// thread grids; the sums are plain sequential float64 sums.
#include "lpc_emit.hpp"

extern "C" {

// key[624], *pos: a RandomState state, advanced in place over n doubles; out: the
// doubles, or NULL to skip them (mt_stream with one thread).
void mt_fill(uint32_t *key, int *pos, long long n, double *out)
{
    uint32_t st[2 * LPC_MT_N];
    memcpy(st, key, LPC_MT_N * 4);
    int64_t last = 0;
    *pos = lpc::mt_stream(st, (int32_t)*pos, (int64_t)n, out, 0, 1, lpc::MtNoSync(), &last);
    memcpy(key, st + (last & 1) * LPC_MT_N, LPC_MT_N * 4);
}

// draws: u[n] | v[n].  Rays [first, first + count) into origin4 / dir4 (count,4), pow[count].
void emit_hemisphere(const double *draws, long long n, long long first, long long count, const float *center4,
                     const double *Rx, const double *Rz, double power, double m, float *origin4, float *dir4,
                     float *pow)
{
    double S = 0.0, ce;
    for (long long i = 0; i < n; ++i) {
        lpc::emit_hemi_dir(draws[i], draws[n + i], Rx, Rz, &ce);
        S += (double)lpc::emit_weight(ce, m);
    }
    for (long long i = 0; i < count; ++i) {
        const long long g = first + i;
        const lpc::d3 d = lpc::emit_hemi_dir(draws[g], draws[n + g], Rx, Rz, &ce);
        for (int k = 0; k < 4; ++k) origin4[4 * i + k] = center4[k];
        dir4[4 * i] = (float)d.x; dir4[4 * i + 1] = (float)d.y; dir4[4 * i + 2] = (float)d.z; dir4[4 * i + 3] = 0.0f;
        pow[i] = lpc::emit_power(lpc::emit_weight(ce, m), (float)power, (float)S);
    }
}

// draws: x[n] | y[n].
void emit_collimated(const double *draws, long long n, long long first, long long count, double diameter,
                     const float *center4, const double *Rx, const double *Rz, const float *dir_row3, double power,
                     float *origin4, float *dir4, float *pow)
{
    const float each = lpc::emit_power(1.0f, (float)power, (float)(double)n);
    for (long long i = 0; i < count; ++i) {
        const long long g = first + i;
        const lpc::d3 o = lpc::emit_colli_origin(draws[g], draws[n + g], diameter, Rx, Rz);
        origin4[4 * i] = lpc::add_f32((float)o.x, center4[0]);
        origin4[4 * i + 1] = lpc::add_f32((float)o.y, center4[1]);
        origin4[4 * i + 2] = lpc::add_f32((float)o.z, center4[2]);
        origin4[4 * i + 3] = lpc::add_f32(0.0f, center4[3]);
        for (int k = 0; k < 3; ++k) dir4[4 * i + k] = dir_row3[k];
        dir4[4 * i + 3] = 0.0f;
        pow[i] = each;
    }
}

// rotate_rays in place on (n,4) rows.
void rays_rotate(float *origin4, float *dir4, long long n, const double *R, const double *piv4)
{
    for (long long i = 0; i < n; ++i) {
        float *o = origin4 + 4 * i, *d = dir4 + 4 * i;
        const lpc::d3 ro = lpc::rotate_origin(o[0], o[1], o[2], R, piv4);
        const lpc::d3 rd = lpc::rotate_dir(d[0], d[1], d[2], R);
        o[0] = (float)ro.x; o[1] = (float)ro.y; o[2] = (float)ro.z; o[3] = (float)(0.0 + piv4[3]);
        d[0] = (float)rd.x; d[1] = (float)rd.y; d[2] = (float)rd.z; d[3] = 0.0f;
    }
}

}  // extern "C"
