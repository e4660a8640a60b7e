// dw_episode.h -- host and device: what the per-env logic of the recorders shares (dw_stats.h, dw_amp_stats.h, dw_trace.h, dw_meter.h): the
// bit casts, the SoA view of a statistics window, the contact mask and the order of the summarize sums.  Plain C++ for the g++ builds of
// the tests; DESIGN.md section 16a.
#ifndef DW_EPISODE_H
#define DW_EPISODE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPI_HD __host__ __device__ __forceinline__
#else
#define EPI_HD inline
#endif

namespace epi {

EPI_HD float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
EPI_HD uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// SoA view of st / ac: word k of env e at k * n + e
struct Rows {
    uint32_t *st;
    float *ac;
    int n, e;
    EPI_HD uint32_t &w(int k) const { return st[(size_t)k * n + e]; }
    EPI_HD float &a(int k) const { return ac[(size_t)k * n + e]; }
};

// bit g of (lo | hi << 32): Gym body g (not a sole) is over the threshold, over(x, y, z) of its contact force
template <int NB, int LFOOT, int RFOOT, class Over>
EPI_HD void contact_mask(const float *cf, uint32_t &lo, uint32_t &hi, Over over) {
    lo = hi = 0u;
    for (int g = 0; g < NB; ++g)
        if (g != LFOOT && g != RFOOT && over(cf[3 * g], cf[3 * g + 1], cf[3 * g + 2])) {
            if (g < 32) lo |= 1u << g;
            else hi |= 1u << (g - 32);
        }
}

// the fixed order of every float sum of a summarize: RT partial sums in double over e = t, t + RT, ..., then a halving tree
constexpr int RT = 256;

EPI_HD double partial(const float *row, int n, int t) {
    double s = 0.0;
    for (int e = t; e < n; e += RT) s += (double)row[e];
    return s;
}

}  // namespace epi

#endif
