// dw_factor_wave.h -- device-only: the stages that dwl_k_solve (dw_forward_dynamics.hip) and dwc_k_solve (dw_contact_dynamics.hip) run alike
// to form M and its L' D L factor and to solve with it, a wave of L = 64 lanes per env.  The per-env arithmetic is dw_factor.h's and
// dw_jacobian.h's; what stands here is how it is spread over the lanes, and the workgroup barriers between its steps.  Every lane of the
// workgroup calls every function here, with the same arguments apart from its own t, lane, live and the env's E, H and B: the barriers are
// the workgroup's, every loop bound is the same for every env.
#ifndef DW_FACTOR_WAVE_H
#define DW_FACTOR_WAVE_H

#include <hip/hip_runtime.h>

#include "dw_factor.h"

namespace dwl {

constexpr int L = 64, SLOTS = 16 * 16;

// a lane per (env, record) forms its inertia; then a lane per (env, moving body) sums its subtree (body-major, leaves first: a wave's lanes
// hold bodies with subtrees of like size, and the wave that walked the chain starts on the leaves).  ENV: the words of an env's store
template <int ENV>
__device__ __forceinline__ void inertia(const dwb::Tab &T, float *s_env, bool has_ms, const float *s_ms, int ne, int t) {
    if (t < ne * dwj::NI) {
        const int e = t / dwj::NI, k = t - e * dwj::NI;
        float *E = s_env + e * ENV;
        dwj::record_inertia(T, E + dwj::E_KS, has_ms ? s_ms + e * NB : nullptr, k, E + dwj::E_REC + k * dwj::RW);
    }
    __syncthreads();
    if (t < ne * dwj::NM) {
        const int b = t / ne;
        dwj::body_sum(T, s_env + (t - b * ne) * ENV, dwj::NM - 1 - b);
    }
    __syncthreads();
}

// the 396 pattern words of M into the env's store H; arm: the env's dof_armature row, or nullptr for none
__device__ __forceinline__ void form(const dwb::Tab &T, const float *E, float *H, const float *arm, int lane, bool live) {
    if (live)
        for (int p = lane; p < PAT; p += L) H[p] = form_word(T, E, arm, p);
    __syncthreads();
}

// rows 38 down to 1 eliminated in place, then the multipliers divided out in one pass.  A row's 16 x 16 numbered updates are four to a lane:
// all four read, then all four written, so that a lane waits for one round of loads
__device__ __forceinline__ void eliminate(const dwb::Tab &T, float *H, int lane, bool live) {
    int r1 = row_start(T, NV);
    for (int k = NV - 1; k >= 1; --k) {
        const int r0 = row_start(T, k), n = clamp_len(r1 - r0);
        r1 = r0;
        if (live) {
            float v[SLOTS / L];
            int p[SLOTS / L];
#pragma unroll
            for (int i = 0; i < SLOTS / L; ++i) {
                const int u = lane + L * i, s = u >> 4, c = u & 15;
                p[i] = -1;
                if (s < n - 1 && c <= s) v[i] = eliminate_one(T, H, r0, n, s, c, &p[i]);
            }
#pragma unroll
            for (int i = 0; i < SLOTS / L; ++i)
                if (p[i] >= 0) H[p[i]] = v[i];
        }
        __syncthreads();
    }
    if (live)
        for (int p = lane; p < PAT; p += L) scale_word(T, H, p);
    __syncthreads();
}

// the sweeps of nc <= CAP columns B [nc][NV] over the factored store H: rows 38 down to 1 of L'^-1, the division by D, columns 0 up to 37 of
// L^-1.  Every step's updates, columns times the step's pattern words, go over the env's lanes (2 x 32 for one or two columns, 8 x 8
// otherwise) with a barrier between steps
__device__ __forceinline__ void sweeps(const dwb::Tab &T, const float *H, float *B, int nc, int lane, bool live) {
    const int sh = nc <= 2 ? 1 : 3, cl = lane & ((1 << sh) - 1), el = lane >> sh, cs = 1 << sh, es = L >> sh;
    int r1 = row_start(T, NV);
    for (int k = NV - 1; k >= 1; --k) {
        const int r0 = row_start(T, k), m = clamp_len(r1 - r0) - 1;
        r1 = r0;
        if (live)
            for (int c = cl; c < nc; c += cs)
                for (int j = el; j < m; j += es) back_one(T, H, B + c * NV, k, r0, j);
        __syncthreads();
    }
    if (live)
        for (int c = cl; c < nc; c += cs)
            for (int k = el; k < NV; k += es) scale_one(T, H, B + c * NV, k);
    __syncthreads();
    int q0 = tcol_start(T, 0);
    for (int i = 0; i < NV - 1; ++i) {
        const int q1 = tcol_start(T, i + 1), m = q1 - q0;
        if (live)
            for (int c = cl; c < nc; c += cs)
                for (int j = el; j < m; j += es) fwd_one(T, H, B + c * NV, i, q0, j);
        q0 = q1;
        __syncthreads();
    }
}

}  // namespace dwl

#endif
