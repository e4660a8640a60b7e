// dw_group.h -- device-only: what the model-tensor kernels (dw_bodies.hip, dw_sensors.hip, dw_jacobian.hip, dw_dynamics.hip,
// dw_forward_dynamics.hip, dw_contact_dynamics.hip) share outside the per-env arithmetic: the loads and the store that a workgroup of TPB
// lanes makes together, t = threadIdx.x; and, with the recorders (dw_stats.hip, dw_amp_stats.hip, dw_trace.hip, dw_meter.hip, dw_gait.hip),
// the error buffer of an ABI's entry points and the "listed envs" launch.  namespace grp: no ABI prefix (dwg is the gait profile's).
#ifndef DW_GROUP_H
#define DW_GROUP_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace grp {

// the text dw?_last_error returns: every translation unit holds one of its own, since the error is per ABI
struct Err {
    char s[256] = "";
    int fail(const char *msg) { snprintf(s, sizeof(s), "%s", msg); return -1; }
    int fail(const char *who, const char *msg) { snprintf(s, sizeof(s), "%s: %s", who, msg); return -1; }
    int fail_hip(const char *who, hipError_t e) { return fail(who, hipGetErrorString(e)); }
    // after a kernel launch of entry point `who`
    int launched(const char *who) {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return 0;
        snprintf(s, sizeof(s), "%s: launch: %s", who, hipGetErrorString(e));
        return -1;
    }
    // num_envs of a launch in groups of `group` envs
    int envs(const char *who, int32_t num_envs, int group) {
        if (num_envs >= 1 && num_envs <= 0x7fffffff - group) return 0;
        snprintf(s, sizeof(s), "%s: num_envs must be in [1, 2^31 - %d)", who, group);
        return -1;
    }
    // lanes of a "listed envs" launch: num_ids of them, or with no list every env; -1: refused (more than most ids, or a negative count)
    int listed(const char *who, const int32_t *env_ids, int32_t num_ids, int32_t num_envs, int32_t most) {
        const int m = env_ids ? num_ids : num_envs;
        if (m < 0 || (env_ids && num_ids > most)) return fail(who, "bad env id list");
        return m;
    }
};

// lane i of a "listed envs" kernel: e is its env; false where the lane has none (past the list, or an id that is no env)
__device__ __forceinline__ bool listed_env(const int32_t *__restrict__ ids, int num_ids, int n, int &e) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_ids) return false;
    e = ids ? ids[i] : i;
    return e >= 0 && e < n;
}

// the model table from global memory into LDS, 16 bytes per lane
template <int TPB, int WORDS>
__device__ __forceinline__ void load_table(const uint4 *__restrict__ table, int t, uint4 *dst) {
    static_assert(WORDS % 4 == 0, "the table is loaded in 16-byte pieces");
    for (int i = t; i < WORDS / 4; i += TPB) dst[i] = table[i];
}

// the group's rows from global memory into LDS: consecutive lanes, consecutive words
template <int TPB>
__device__ __forceinline__ void load_rows(const float *__restrict__ src, int e0, int ne, int row, int t, float *dst) {
    src += (size_t)e0 * row;
    for (int i = t; i < ne * row; i += TPB) dst[i] = src[i];
}

// a group's contiguous block: words [0, total) of dst, word(i) formed on the way out, 16 bytes per lane where dst is 16-byte aligned
template <int TPB, class W>
__device__ __forceinline__ void store_block(float *__restrict__ dst, int total, bool aligned, int t, W word) {
    int done = 0;
    if (aligned) {
        const int nv = total / 4;
        for (int i4 = t; i4 < nv; i4 += TPB) {
            const float a = word(4 * i4), b = word(4 * i4 + 1), c = word(4 * i4 + 2), d = word(4 * i4 + 3);
            reinterpret_cast<float4 *>(dst)[i4] = make_float4(a, b, c, d);
        }
        done = 4 * nv;
    }
    for (int i = done + t; i < total; i += TPB) dst[i] = word(i);
}

}  // namespace grp

#endif
