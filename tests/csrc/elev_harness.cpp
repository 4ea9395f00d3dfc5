// Host build of the elevation arithmetic shared with the HIP kernels
// (lightpycl_amd/csrc/lpc_math.hpp elev_cos / elevation), for tests/test_beam_host.py.
// Built with g++ -ffp-contract=off.
#include "lpc_math.hpp"

extern "C" {

// pos4: (n,4) float32 rows, pole: double[4] -> c[n] (the cosine), e[n] (the elevation)
void elev_eval(const float *pos4, long long n, const double *pole, double *c, double *e)
{
    for (long long i = 0; i < n; ++i) {
        const float *p = pos4 + 4 * i;
        c[i] = lpc::elev_cos(p[0], p[1], p[2], p[3], pole);
        e[i] = lpc::elevation(p[0], p[1], p[2], p[3], pole);
    }
}

}  // extern "C"
