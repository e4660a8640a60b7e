// dw_record_group.h -- device-only: the stages of a staged record launch, shared by dws_k_record (dw_stats.hip) and dwe_k_record
// (dw_amp_stats.hip), and the body of their summarize kernels.  A workgroup of TPB lanes takes EPB envs, t =
// threadIdx.x.  The order is the caller's to keep: every *_load of a kernel before its first *_store, zero_counts before the first barrier.
#ifndef DW_RECORD_GROUP_H
#define DW_RECORD_GROUP_H

#include "../../include/dyros_walk.h"
#include "dw_episode.h"
#include "dw_group.h"

namespace rec {

// envs and lanes per workgroup: 32 / 128 measured fastest at 16384 envs against 16 / 128, 16 / 64, 8 / 128, 8 / 64, 4 / 64
constexpr int EPB = 32, TPB = 128;
constexpr int NB = DW_NUM_BODIES;
constexpr int CFW = EPB * NB * 3;                   // contact words of a workgroup
constexpr int NCF = (CFW / 4 + TPB - 1) / TPB;      // 16-byte pieces of them per lane
static_assert(EPB <= TPB && TPB % 64 == 0, "one lane per env");
static_assert(CFW % 4 == 0 && (NB * 3 * EPB * 4) % 16 == 0, "a workgroup's contact span is whole 16-byte pieces from a 16-byte aligned start");

constexpr int regs(int words) { return (words + TPB - 1) / TPB; }

// the contact rows of envs e0 .. e0 + ne - 1 into registers: one contiguous span of ne * 114 words from a 16-byte aligned start (e0 * 456 B);
// a whole group in 16-byte loads, the last group word by word
__device__ __forceinline__ void contact_load(float4 (&v)[NCF], const float *__restrict__ contact_forces, int e0, int ne, int t) {
    const float *cf = contact_forces + (size_t)e0 * NB * 3;
    const int ncf = ne * NB * 3;
#pragma unroll
    for (int k = 0; k < NCF; ++k) {
        const int i = t + k * TPB;
        if (ne == EPB) {
            if (i < CFW / 4) v[k] = reinterpret_cast<const float4 *>(cf)[i];
        } else {
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (4 * i + 0 < ncf) x.x = cf[4 * i + 0];
            if (4 * i + 1 < ncf) x.y = cf[4 * i + 1];
            if (4 * i + 2 < ncf) x.z = cf[4 * i + 2];
            if (4 * i + 3 < ncf) x.w = cf[4 * i + 3];
            v[k] = x;
        }
    }
}
__device__ __forceinline__ void contact_store(float4 *s_cf4, const float4 (&v)[NCF], int t) {
#pragma unroll
    for (int k = 0; k < NCF; ++k) {
        const int i = t + k * TPB;
        if (i < CFW / 4) s_cf4[i] = v[k];
    }
}

// words i = t, t + TPB, ... < cnt of the span that starts at src: into registers, and from there to LDS
template <int WORDS, int N>
__device__ __forceinline__ void span_load(float (&v)[N], const float *__restrict__ src, int cnt, int t) {
    static_assert(N == regs(WORDS), "register count");
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = t + k * TPB;
        v[k] = i < cnt ? src[i] : 0.0f;
    }
}
template <int WORDS, int N>
__device__ __forceinline__ void span_store(float *dst, const float (&v)[N], int t) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = t + k * TPB;
        if (i < WORDS) dst[i] = v[k];
    }
}

// the integer counts of a workgroup, gathered in LDS: what an update calls add and max on
struct LdsCount {
    unsigned int *w;
    __device__ void add(int k, unsigned int v) const { if (v) atomicAdd(&w[k], v); }
    __device__ void max(int k, unsigned int v) const { atomicMax(&w[k], v); }
};

template <int WINDOW>
__device__ __forceinline__ void zero_counts(unsigned int (*s_mask)[2], unsigned int *s_ct, int t) {
    for (int i = t; i < EPB * 2; i += TPB) s_mask[i >> 1][i & 1] = 0u;
    for (int i = t; i < WINDOW; i += TPB) s_ct[i] = 0u;
}

// the bodies over the threshold as a bit mask per env: one lane per env and body, the soles left out
template <int LFOOT, int RFOOT, class Over>
__device__ __forceinline__ void mask_pass(const float *s_cf, unsigned int (*s_mask)[2], int ne, int t, Over over) {
    for (int i = t; i < ne * NB; i += TPB) {
        const int el = i / NB, g = i - NB * el;
        const float *f = s_cf + 3 * i;
        if (g != LFOOT && g != RFOOT && over(f[0], f[1], f[2])) atomicOr(&s_mask[el][g >> 5], 1u << (g & 31));
    }
}

// the workgroup's counts into ct: one atomic per non-zero word (RECORDS is count_call's, LEN_MAX a maximum)
template <int WINDOW, int RECORDS, int LEN_MAX>
__device__ __forceinline__ void flush(const unsigned int *s_ct, unsigned long long *ct, int t) {
    for (int i = t; i < WINDOW; i += TPB) {
        const unsigned int v = s_ct[i];
        if (v == 0u || i == RECORDS) continue;
        if (i == LEN_MAX) atomicMax(&ct[i], (unsigned long long)v);
        else atomicAdd(&ct[i], (unsigned long long)v);
    }
}

// a summarize kernel of epi::RT lanes: one workgroup per float word of ac (word blockIdx.x), every sum in epi's fixed order; workgroup 0
// also converts the counts
template <int CT_WORDS, int SUM_AC>
__device__ __forceinline__ void summarize(int n, const float *__restrict__ ac, const unsigned long long *__restrict__ ct, double *out) {
    __shared__ double red[epi::RT];
    const int t = threadIdx.x, k = blockIdx.x;
    if (k == 0)
        for (int i = t; i < CT_WORDS; i += epi::RT) out[i] = (double)ct[i];
    red[t] = epi::partial(ac + (size_t)k * n, n, t);
    __syncthreads();
    for (int s = epi::RT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) out[SUM_AC + k] = red[0];
}

}  // namespace rec

#endif
