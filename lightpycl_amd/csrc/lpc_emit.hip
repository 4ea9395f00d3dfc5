// lpc_emit.hip -- gfx950 kernels of the device-born light sources (lpc_emit.hpp):
//   k_mt19937          numpy's legacy generator continued on the device: one
//                      workgroup, both blocks of the state in LDS.
//   k_emit_weights     per-tile float64 sums of the directivity weights.
//   k_sum_tiles        the tiles' sums in a fixed order (one workgroup).
//   k_emit_hemisphere  random_rays' transform + power, rays [first, first + count).
//   k_emit_collimated  random_collimated_rays' transform.
//   k_rays_rotate      rotate_rays on a device source.
// Every sum is a fixed tree over a fixed tiling of the rays: no float atomics, so
// two runs give the same bits.  Included by lpc_runtime.hip after lpc_kernels.hip.
#include "lpc_emit.hpp"

namespace lpck {

#define LPC_MT_THREADS 320              // 5 waves: a block's 312 doubles in one pass
#define LPC_EMIT_TILE 1024              // rays per k_emit_weights tile

struct MtBlockSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// key[624] / *pos in and out (device memory); out: n doubles or NULL (skip).
__global__ __launch_bounds__(LPC_MT_THREADS) void k_mt19937(uint32_t *__restrict__ key, int32_t *__restrict__ pos,
                                                            int64_t n, double *__restrict__ out)
{
    __shared__ uint32_t st[2 * LPC_MT_N];
    const int tid = threadIdx.x;
    for (int k = tid; k < LPC_MT_N; k += LPC_MT_THREADS) st[k] = key[k];
    const int32_t p0 = *pos;
    __syncthreads();
    int64_t last = 0;
    const int32_t p1 = mt_stream(st, p0, n, out, tid, LPC_MT_THREADS, MtBlockSync(), &last);
    __syncthreads();
    const uint32_t *fin = st + (last & 1) * LPC_MT_N;
    for (int k = tid; k < LPC_MT_N; k += LPC_MT_THREADS) key[k] = fin[k];
    if (tid == 0) *pos = p1;
}

// Sum of a 256-thread block's values in a fixed order: the wave butterflies,
// then the four waves left to right.  Valid on thread 0.
static __device__ __forceinline__ double block_sum_fixed(double v, double *s4)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// tile[b] = sum over rays [1024 b, 1024 b + 1024) of (double)float32(cos(acos(u)) ** m)
__global__ __launch_bounds__(256) void k_emit_weights(const double *__restrict__ u, int64_t n, double m,
                                                      double *__restrict__ tile)
{
    __shared__ double s4[4];
    const int64_t lo = (int64_t)blockIdx.x * LPC_EMIT_TILE;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < LPC_EMIT_TILE / 256; ++r) {
        const int64_t i = lo + r * 256 + threadIdx.x;
        if (i < n) acc += (double)emit_weight(cos(acos(u[i])), m);
    }
    const double s = block_sum_fixed(acc, s4);
    if (threadIdx.x == 0) tile[blockIdx.x] = s;
}

// *out = the nt tile sums in a fixed order (thread t takes t, t + 256, ...).
__global__ __launch_bounds__(256) void k_sum_tiles(const double *__restrict__ tile, int64_t nt, double *__restrict__ out)
{
    __shared__ double s4[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < nt; i += 256) acc += tile[i];
    const double s = block_sum_fixed(acc, s4);
    if (threadIdx.x == 0) *out = s;
}

struct EmitArgs {
    const double *draws;        // 2 n doubles: u | v (hemisphere), x | y (collimated)
    int64_t n, first, count;
    double Rx[9], Rz[9];
    float center[4];
    float dir[3];               // collimated: the constant direction row
    float power;                // float32(power); collimated: each ray's power
    double m, diameter;
    const double *wsum;         // hemisphere: the float64 sum of the weights
    float4 *origin, *dirs;
    float *pow;
    double *tile;               // per 256-ray block: float64 sum of the powers written
};

__global__ __launch_bounds__(256) void k_emit_hemisphere(EmitArgs A)
{
    __shared__ double s4[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double mine = 0.0;
    if (i < A.count) {
        const int64_t g = A.first + i;
        double ce;
        const d3 d = emit_hemi_dir(A.draws[g], A.draws[A.n + g], A.Rx, A.Rz, &ce);
        const float pw = emit_power(emit_weight(ce, A.m), A.power, (float)*A.wsum);
        A.origin[i] = make_float4(A.center[0], A.center[1], A.center[2], A.center[3]);
        A.dirs[i] = make_float4((float)d.x, (float)d.y, (float)d.z, 0.0f);
        A.pow[i] = pw;
        mine = (double)pw;
    }
    const double s = block_sum_fixed(mine, s4);
    if (threadIdx.x == 0) A.tile[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_emit_collimated(EmitArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.count) return;
    const int64_t g = A.first + i;
    const d3 o = emit_colli_origin(A.draws[g], A.draws[A.n + g], A.diameter, A.Rx, A.Rz);
    A.origin[i] = make_float4(add_f32((float)o.x, A.center[0]), add_f32((float)o.y, A.center[1]),
                              add_f32((float)o.z, A.center[2]), add_f32(0.0f, A.center[3]));
    A.dirs[i] = make_float4(A.dir[0], A.dir[1], A.dir[2], 0.0f);
    A.pow[i] = A.power;
}

struct RotateArgs {
    int64_t n;
    double R[9], piv[4];
    float4 *origin, *dirs;
};

__global__ __launch_bounds__(256) void k_rays_rotate(RotateArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const float4 o = A.origin[i], d = A.dirs[i];
    const d3 ro = rotate_origin(o.x, o.y, o.z, A.R, A.piv);
    const d3 rd = rotate_dir(d.x, d.y, d.z, A.R);
    A.origin[i] = make_float4((float)ro.x, (float)ro.y, (float)ro.z, (float)(0.0 + A.piv[3]));
    A.dirs[i] = make_float4((float)rd.x, (float)rd.y, (float)rd.z, 0.0f);
}

}  // namespace lpck
