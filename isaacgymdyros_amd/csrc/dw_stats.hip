// dw_stats.hip -- the kernels of DyrosDynamicWalk's episode statistics (include/dyros_stats.h).  The per-env logic is
// dw_stats.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   k_record     one launch per step.  A workgroup of 128 lanes takes 32 envs: their contact rows (32 x 456 B, one contiguous span),
//                root rows and the 12 action_torque words of their env_state rows are staged in LDS with consecutive lanes on consecutive words; the
//                bodies over 1 N become a bit mask per env (one lane per env and body); then one lane per env runs dws::update, its integer
//                counts gathered in LDS and added to ct with one atomic per non-zero word and workgroup.
//   k_restart    one lane per listed env (or every env).
//   k_summarize  one workgroup per float word of ac: every sum in dws's fixed order; the counts converted.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_stats.h"

namespace {

char s_err[256] = "";
int fail(const char *msg) { snprintf(s_err, sizeof(s_err), "%s", msg); return -1; }
int fail_hip(const char *who, hipError_t e) { snprintf(s_err, sizeof(s_err), "%s: %s", who, hipGetErrorString(e)); return -1; }

// envs and lanes per workgroup: 32 / 128 measured fastest at 16384 envs against 16 / 128, 16 / 64, 8 / 128, 8 / 64, 4 / 64
constexpr int EPB = 32, TPB = 128;
constexpr int CFW = EPB * dws::NB * 3;              // contact words of a workgroup
constexpr int TQW = 12;                             // action_torque
static_assert(EPB <= TPB && TPB % 64 == 0, "one lane per env");
static_assert((dws::NB * 3 * EPB) % 4 == 0, "a workgroup's contact span is whole 16-byte pieces");

struct LdsCount {
    unsigned int *w;
    __device__ void add(int k, unsigned int v) const { if (v) atomicAdd(&w[k], v); }
    __device__ void max(int k, unsigned int v) const { atomicMax(&w[k], v); }
};

__global__ __launch_bounds__(TPB) void dws_k_record(int n, const float *__restrict__ root_states, const float *__restrict__ contact_forces,
                                                    const float *__restrict__ env_state, const int64_t *__restrict__ reset_buf,
                                                    const float *__restrict__ total_mass, uint32_t *__restrict__ st, float *__restrict__ ac,
                                                    unsigned long long *ct, uint8_t *cause, float max_len, float dt_policy) {
    __shared__ float4 s_cf4[CFW / 4];
    __shared__ float s_root[EPB * 13];
    __shared__ float s_tq[EPB * TQW];
    __shared__ unsigned int s_mask[EPB][2];
    __shared__ unsigned int s_ct[DWS_CT_WINDOW];
    float *s_cf = reinterpret_cast<float *>(s_cf4);
    const int t = threadIdx.x, e0 = blockIdx.x * EPB;
    const int ne = n - e0 < EPB ? n - e0 : EPB;          // envs of this workgroup (the last one may hold fewer)
    // ---- every global load first, into registers: the contact rows (one contiguous span of ne * 114 words from a 16-byte aligned start,
    //      e0 * 456 B), the root rows, the torque words; and on lanes 0 .. ne - 1 the env's own words and its running state ----
    constexpr int NCF = (CFW / 4 + TPB - 1) / TPB, NRT = (EPB * 13 + TPB - 1) / TPB, NTQ = (EPB * TQW + TPB - 1) / TPB;
    const float *cf = contact_forces + (size_t)e0 * dws::NB * 3;
    const int ncf = ne * dws::NB * 3;
    float4 vcf[NCF];
    float vrt[NRT], vtq[NTQ];
#pragma unroll
    for (int k = 0; k < NCF; ++k) {
        const int i = t + k * TPB;
        if (ne == EPB) {
            if (i < CFW / 4) vcf[k] = reinterpret_cast<const float4 *>(cf)[i];
        } else {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (4 * i + 0 < ncf) v.x = cf[4 * i + 0];
            if (4 * i + 1 < ncf) v.y = cf[4 * i + 1];
            if (4 * i + 2 < ncf) v.z = cf[4 * i + 2];
            if (4 * i + 3 < ncf) v.w = cf[4 * i + 3];
            vcf[k] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < NRT; ++k) {
        const int i = t + k * TPB;
        vrt[k] = i < ne * 13 ? root_states[(size_t)e0 * 13 + i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < NTQ; ++k) {
        const int i = t + k * TPB, el = i / TQW, w = i - TQW * el;
        vtq[k] = i < ne * TQW ? env_state[(size_t)(e0 + el) * dws::ESW + DW_ES_ACTION_TORQUE + w] : 0.0f;
    }
    const bool own = t < ne;
    const int e = e0 + (own ? t : 0);
    const dws::Rows r{st, ac, n, e};
    dws::EnvIn in;
    dws::St s;
    dws::AcHot h;
    if (own) {
        const float *es = env_state + (size_t)e * dws::ESW;
        const int *esi = reinterpret_cast<const int *>(es);
        in.tv0 = es[DW_ES_TARGET_VEL];
        in.tv1 = es[DW_ES_TARGET_VEL + 1];
        in.tf0 = es[DW_ES_TARGET_FORCE];
        in.tf1 = es[DW_ES_TARGET_FORCE + 1];
        in.last_return = es[DW_ES_LAST_RETURN];
        in.total_mass = total_mass[e];
        in.pert_on = esi[DW_ES_PERT_ON];
        in.nan_resets = esi[DW_ES_NAN_RESETS];
        in.reset = reset_buf[e] != 0;
        s = dws::load(r);
        h = dws::load_hot(r);
    }
    // ---- into LDS; the bodies over 1 N as a bit mask per env (one lane per env and body) ----
#pragma unroll
    for (int k = 0; k < NCF; ++k) {
        const int i = t + k * TPB;
        if (i < CFW / 4) s_cf4[i] = vcf[k];
    }
#pragma unroll
    for (int k = 0; k < NRT; ++k) {
        const int i = t + k * TPB;
        if (i < EPB * 13) s_root[i] = vrt[k];
    }
#pragma unroll
    for (int k = 0; k < NTQ; ++k) {
        const int i = t + k * TPB;
        if (i < EPB * TQW) s_tq[i] = vtq[k];
    }
    for (int i = t; i < EPB * 2; i += TPB) s_mask[i >> 1][i & 1] = 0u;
    for (int i = t; i < DWS_CT_WINDOW; i += TPB) s_ct[i] = 0u;
    __syncthreads();
    for (int i = t; i < ne * dws::NB; i += TPB) {
        const int el = i / dws::NB, g = i - dws::NB * el;
        const float *f = s_cf + 3 * i;
        if (g != DWS_LFOOT && g != DWS_RFOOT && dws::over_1n(f[0], f[1], f[2])) atomicOr(&s_mask[el][g >> 5], 1u << (g & 31));
    }
    __syncthreads();
    // ---- one lane per env ----
    if (own) {
        in.cf = s_cf + t * dws::NB * 3;
        in.root = s_root + t * 13;
        in.tq = s_tq + t * TQW;
        LdsCount c{s_ct};
        cause[e] = (uint8_t)dws::update(in, s_mask[t][0], s_mask[t][1], s, h, r, c, max_len, dt_policy);
        dws::store(r, s);
        dws::store_hot(r, h);
    }
    if (blockIdx.x == 0 && t == 0) dws::count_call(reinterpret_cast<uint64_t *>(ct), reinterpret_cast<const int *>(env_state)[DW_ES_PERT_START]);
    __syncthreads();
    for (int i = t; i < DWS_CT_WINDOW; i += TPB) {
        const unsigned int v = s_ct[i];
        if (v == 0u || i == DWS_CT_RECORDS) continue;
        if (i == DWS_CT_LEN_MAX) atomicMax(&ct[i], (unsigned long long)v);
        else atomicAdd(&ct[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void dws_k_restart(int n, const int32_t *__restrict__ ids, int num_ids, const float *__restrict__ root_states,
                                                     const float *__restrict__ env_state, const int64_t *__restrict__ progress_buf, uint32_t *st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_ids) return;
    const int e = ids ? ids[i] : i;
    if (e < 0 || e >= n) return;
    const float *es = env_state + (size_t)e * dws::ESW;
    const int *esi = reinterpret_cast<const int *>(es);
    dws::St s;
    dws::begin(s, (int)progress_buf[e], root_states + (size_t)e * 13, es[DW_ES_TARGET_VEL], esi[DW_ES_PERT_ON] ? 1 : 0, esi[DW_ES_NAN_RESETS]);
    dws::store(dws::Rows{st, nullptr, n, e}, s);
}

// one workgroup per float word of ac (word blockIdx.x); workgroup 0 also converts the counts
__global__ __launch_bounds__(dws::RT) void dws_k_summarize(int n, const float *__restrict__ ac, const unsigned long long *__restrict__ ct, double *out) {
    __shared__ double red[dws::RT];
    const int t = threadIdx.x, k = blockIdx.x;
    if (k == 0)
        for (int i = t; i < DWS_CT_WORDS; i += dws::RT) out[i] = (double)ct[i];
    red[t] = dws::partial(ac + (size_t)k * n, n, t);
    __syncthreads();
    for (int s = dws::RT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) out[DWS_SUM_AC + k] = red[0];
}

}  // namespace

extern "C" {

int dws_abi_version(void) { return DWS_ABI_VERSION; }
const char *dws_last_error(void) { return s_err; }

int dws_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *env_state, const int64_t *reset_buf,
               const float *total_mass, void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float dt_policy,
               void *stream) {
    if (num_envs < 1) return fail("dws_record: num_envs must be positive");
    if (!root_states || !contact_forces || !env_state || !reset_buf || !total_mass || !st || !ac || !ct || !cause)
        return fail("dws_record: a buffer is missing");
    if (!(max_episode_length > 0.0f)) return fail("dws_record: max_episode_length must be positive");
    if ((reinterpret_cast<uintptr_t>(contact_forces) & 15u) != 0u) return fail("dws_record: contact_forces must be 16-byte aligned");
    hipLaunchKernelGGL(dws_k_record, dim3((num_envs + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, root_states, contact_forces,
                       env_state, reset_buf, total_mass, (uint32_t *)st, ac, (unsigned long long *)ct, cause, max_episode_length, dt_policy);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip("dws_record: launch", e);
}

int dws_restart(int32_t num_envs, const int32_t *env_ids, int32_t num_ids, const float *root_states, const float *env_state,
                const int64_t *progress_buf, void *st, void *stream) {
    if (num_envs < 1) return fail("dws_restart: num_envs must be positive");
    if (!root_states || !env_state || !progress_buf || !st) return fail("dws_restart: a buffer is missing");
    const int m = env_ids ? num_ids : num_envs;
    if (m < 0 || (env_ids && num_ids > num_envs)) return fail("dws_restart: bad env id list");
    if (m == 0) return 0;
    hipLaunchKernelGGL(dws_k_restart, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)num_envs, env_ids, m, root_states, env_state,
                       progress_buf, (uint32_t *)st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip("dws_restart: launch", e);
}

int dws_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream) {
    if (num_envs < 1) return fail("dws_summarize: num_envs must be positive");
    if (!ac || !ct || !out) return fail("dws_summarize: a buffer is missing");
    hipLaunchKernelGGL(dws_k_summarize, dim3(DWS_AC_WORDS), dim3(dws::RT), 0, (hipStream_t)stream, (int)num_envs, ac, (const unsigned long long *)ct, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip("dws_summarize: launch", e);
}

}  // extern "C"
