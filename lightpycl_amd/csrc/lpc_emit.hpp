// lpc_emit.hpp -- light sources born on the device: numpy's legacy random stream
// (np.random.rand after np.random.seed) continued word for word, and the float64
// transforms of lightpycl_amd/light_source.py (random_rays, random_collimated_rays,
// rotate_rays) in their operation order.  Shared by the HIP kernels (lpc_emit.hip)
// and the CPU tests (tests/csrc/emit_harness.cpp, built with g++ -ffp-contract=off).
//
// The generator is pure integer arithmetic, so its doubles are numpy's bit for
// bit.  The transforms evaluate the same float64 expression tree as numpy on the
// same draws and matrices; the libm last bits (acos, sin, cos) and the order of a
// 3-term dot may differ, so a float32 result may differ by one rounding step
// (DESIGN.md section 10).
#pragma once
#include "lpc_math.hpp"

namespace lpc {

// ---------------------------------------------------------------------------
// MT19937 as numpy's RandomState keeps it: key[624] and pos in 0..624 (624: the
// next draw regenerates the block first).
#define LPC_MT_N 624
#define LPC_MT_M 397

LPC_HD uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far)
{
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
// Word k of the next block from the old block and the new block's earlier words.
// Three phases, each reading only what the phases before it wrote:
//   0: k in [0, 227)    old[k], old[k + 1], old[k + 397]
//   1: k in [227, 454)  old[k], old[k + 1], new[k - 227]   (phase 0)
//   2: k in [454, 624)  old[k], old[k + 1], new[k - 227]   (phase 1); k = 623 takes
//                       new[0] (phase 0) for old[k + 1] and new[396] (phase 1)
LPC_HD uint32_t mt_regen_word(int k, const uint32_t *old, const uint32_t *nw)
{
    const uint32_t nxt = k == LPC_MT_N - 1 ? nw[0] : old[k + 1];
    const uint32_t far = k < LPC_MT_N - LPC_MT_M ? old[k + LPC_MT_M] : nw[k - (LPC_MT_N - LPC_MT_M)];
    return mt_twist(old[k], nxt, far);
}
LPC_HD int mt_phase_begin(int p) { return p == 0 ? 0 : p == 1 ? 227 : 454; }
LPC_HD int mt_phase_end(int p) { return p == 0 ? 227 : p == 1 ? 454 : LPC_MT_N; }
LPC_HD uint32_t mt_temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// random_sample's double from two tempered outputs (exact: a 2^26 + b < 2^53).
LPC_HD double mt_double(uint32_t w0, uint32_t w1)
{
    LPC_EXACT
    const uint32_t a = w0 >> 5, b = w1 >> 6;
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

struct MtNoSync {
#if defined(__HIPCC__)
    __host__ __device__
#endif
    void operator()() const {}
};

// The next n doubles of the stream whose state is (st[0..624), pos), by `nt`
// cooperating threads (`tid` of them this one; `sync` is their barrier; the host
// runs it with one thread and MtNoSync).  st holds two blocks: block B of the
// stream lives in st + (B & 1) * 624, block 0 is the input key.  out == NULL
// only advances.  Double j takes stream words pos + 2 j and pos + 2 j + 1; 624 is
// even, so with an odd pos EVERY block ends on the first word of a double whose
// second word is word 0 of the next block (written by thread 0 once that block
// exists).  Returns the new pos (1..624); *last = the block holding the new key.
template <class Sync>
LPC_HD int32_t mt_stream(uint32_t *st, int32_t pos, int64_t n, double *out, int tid, int nt, Sync sync,
                         int64_t *last)
{
    const int64_t P = (int64_t)pos + 2 * n;
    const int64_t lastB = (P - 1) / LPC_MT_N;
    const int odd = pos & 1;
    for (int64_t B = 0; B <= lastB; ++B) {
        uint32_t *cur = st + (B & 1) * LPC_MT_N;
        const uint32_t *prv = st + ((B & 1) ^ 1) * LPC_MT_N;
        if (B > 0) {
            for (int p = 0; p < 3; ++p) {
                for (int k = mt_phase_begin(p) + tid; k < mt_phase_end(p); k += nt) cur[k] = mt_regen_word(k, prv, cur);
                sync();
            }
        }
        if (out) {
            const int lo = B == 0 ? pos : odd;
            for (int k = lo + 2 * tid; k + 1 < LPC_MT_N; k += 2 * nt) {
                const int64_t j = (LPC_MT_N * B + k - pos) / 2;
                if (j < n) out[j] = mt_double(mt_temper(cur[k]), mt_temper(cur[k + 1]));
            }
            if (odd && B > 0 && tid == 0) {
                const int64_t j = (LPC_MT_N * B - 1 - pos) / 2;
                if (j < n) out[j] = mt_double(mt_temper(prv[LPC_MT_N - 1]), mt_temper(cur[0]));
            }
            sync();                         // the next block overwrites prv
        }
    }
    *last = lastB;
    return (int32_t)(P - LPC_MT_N * lastB);
}

// ---------------------------------------------------------------------------
// The transforms.  numpy multiplies (n,4) rows by the 4x4 matrices of _Rx / _Rz
// (row and column 3 zero); M is their upper-left 3x3, row-major.
struct d3 { double x, y, z; };

LPC_HD d3 row_mul(d3 r, const double *M)
{
    LPC_EXACT
    d3 o;
    o.x = (r.x * M[0] + r.y * M[3]) + r.z * M[6];
    o.y = (r.x * M[1] + r.y * M[4]) + r.z * M[7];
    o.z = (r.x * M[2] + r.y * M[5]) + r.z * M[8];
    return o;
}

// random_rays: u -> elevation = arccos(u), v -> azimuth = (2 pi) v, the direction
// (sin el cos az, sin el sin az, cos el) . Rx(elev0) . Rz(az0).  *cos_el = cos(el),
// the directivity's argument.
LPC_HD d3 emit_hemi_dir(double u, double v, const double *Rx, const double *Rz, double *cos_el)
{
    LPC_EXACT
    const double el = acos(u);
    const double az = (2.0 * 3.141592653589793) * v;
    const double se = sin(el), ce = cos(el);
    d3 d;
    d.x = se * cos(az);
    d.y = se * sin(az);
    d.z = ce;
    *cos_el = ce;
    return row_mul(row_mul(d, Rx), Rz);
}
// float32(cos(el) ** m), m >= 0, with numpy's scalar-exponent shortcuts of power
// (0: ones, 0.5: sqrt, 1: copy, 2: square).
LPC_HD float emit_weight(double ce, double m)
{
    LPC_EXACT
    if (m == 1.0) return (float)ce;
    if (m == 0.0) return 1.0f;
    if (m == 2.0) return (float)(ce * ce);
    if (m == 0.5) return (float)sqrt(ce);
    return (float)pow(ce, m);
}
// pw * float32(power) / float32(sum pw), float32 IEEE arithmetic.
LPC_HD float emit_power(float pw, float power, float S)
{
    LPC_EXACT
    const float t = pw * power;
    return t / S;
}
// random_collimated_rays: ((x - 0.5) d, (y - 0.5) d, 0) . Rx . Rz; the caller casts
// to float32 and adds the float32 centre.
LPC_HD d3 emit_colli_origin(double x, double y, double diameter, const double *Rx, const double *Rz)
{
    LPC_EXACT
    d3 o;
    o.x = (x - 0.5) * diameter;
    o.y = (y - 0.5) * diameter;
    o.z = 0.0;
    return row_mul(row_mul(o, Rx), Rz);
}
LPC_HD float add_f32(float a, float b) { LPC_EXACT return a + b; }
// rotate_rays: (origin - pivot) . R + pivot and dir . R on float32 rows.
LPC_HD d3 rotate_origin(float x, float y, float z, const double *R, const double *piv)
{
    LPC_EXACT
    d3 d;
    d.x = (double)x - piv[0];
    d.y = (double)y - piv[1];
    d.z = (double)z - piv[2];
    d = row_mul(d, R);
    d.x = d.x + piv[0];
    d.y = d.y + piv[1];
    d.z = d.z + piv[2];
    return d;
}
LPC_HD d3 rotate_dir(float x, float y, float z, const double *R)
{
    d3 d;
    d.x = (double)x; d.y = (double)y; d.z = (double)z;
    return row_mul(d, R);
}

}  // namespace lpc
