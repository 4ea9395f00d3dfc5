// Host build of the bin rule shared with the HIP kernels
// (lightpycl_amd/csrc/lpc_math.hpp bin_index), for tests/test_map_host.py.
// Built with g++ -ffp-contract=off.
#include "lpc_math.hpp"

extern "C" {

// v[n] against the edges e[nb + 1] -> out[n] (the bin, -1 outside or NaN)
void bin_eval(const double *v, long long n, const double *e, int nb, int *out)
{
    for (long long i = 0; i < n; ++i) out[i] = lpc::bin_index(v[i], e, nb);
}

}  // extern "C"
