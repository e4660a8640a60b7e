// dw_amp_stats.hip -- the kernels of TocabiAMPLower's episode statistics (include/dyros_amp_stats.h).  The per-env logic is
// dw_amp_stats.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwe_k_record     one launch per step, the shape of dws_k_record (dw_stats.hip).  A workgroup of 128 lanes takes 32 envs: their contact rows
//                    (32 x 456 B, one contiguous span), root rows, reward_values and commands rows are staged in LDS with consecutive lanes on
//                    consecutive words; the bodies with a component over 1 become a bit mask per env (one lane per env and body); then one lane
//                    per env runs dwe::update, its integer counts gathered in LDS and added to ct with one atomic per non-zero word and workgroup.
//   dwe_k_summarize  one workgroup per float word of ac: every sum in dwe's fixed order; the counts converted.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_amp_stats.h"

namespace {

char s_err[256] = "";
int fail(const char *msg) { snprintf(s_err, sizeof(s_err), "%s", msg); return -1; }
int fail_hip(const char *who, hipError_t e) { snprintf(s_err, sizeof(s_err), "%s: %s", who, hipGetErrorString(e)); return -1; }

// envs and lanes per workgroup: dws_k_record's, measured there
constexpr int EPB = 32, TPB = 128;
constexpr int CFW = EPB * dwe::NB * 3;              // contact words of a workgroup
constexpr int RTW = EPB * 13, RVW = EPB * DWE_REW_TERMS, CMW = EPB * 3;
static_assert(EPB <= TPB && TPB % 64 == 0, "one lane per env");
static_assert(CFW % 4 == 0 && (dwe::NB * 3 * EPB * 4) % 16 == 0, "a workgroup's contact span is whole 16-byte pieces from a 16-byte aligned start");
static_assert(DWE_CT_WINDOW <= TPB, "one lane per count word");

struct LdsCount {
    unsigned int *w;
    __device__ void add(int k, unsigned int v) const { if (v) atomicAdd(&w[k], v); }
    __device__ void max(int k, unsigned int v) const { atomicMax(&w[k], v); }
};

// words i = t, t + TPB, ... < cnt of the span that starts at src: into registers (every load before the first store)
template <int WORDS, int N>
__device__ __forceinline__ void span_load(float (&v)[N], const float *__restrict__ src, int cnt, int t) {
    static_assert(N == (WORDS + TPB - 1) / TPB, "register count");
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

__global__ __launch_bounds__(TPB) void dwe_k_record(int n, const float *__restrict__ root_states, const float *__restrict__ contact_forces,
                                                    const float *__restrict__ rigid_body_pos, const float *__restrict__ commands,
                                                    const float *__restrict__ rew_buf, const float *__restrict__ reward_values,
                                                    const int64_t *__restrict__ reset_buf, const int64_t *__restrict__ progress_buf,
                                                    const float *__restrict__ total_mass, uint32_t *__restrict__ st, float *__restrict__ ac,
                                                    unsigned long long *ct, uint8_t *cause, dwe::Cfg C) {
    __shared__ float4 s_cf4[CFW / 4];
    __shared__ float s_root[RTW];
    __shared__ float s_rv[RVW];
    __shared__ float s_cmd[CMW];
    __shared__ unsigned int s_mask[EPB][2];
    __shared__ unsigned int s_ct[DWE_CT_WINDOW];
    float *s_cf = reinterpret_cast<float *>(s_cf4);
    const int t = threadIdx.x, e0 = blockIdx.x * EPB;
    const int ne = n - e0 < EPB ? n - e0 : EPB;          // envs of this workgroup (the last one may hold fewer)
    // ---- every global load first, into registers: the contact rows (one contiguous span of ne * 114 words from a 16-byte aligned start,
    //      e0 * 456 B), the root / reward_values / commands rows; and on lanes 0 .. ne - 1 the env's own words and its running state ----
    constexpr int NCF = (CFW / 4 + TPB - 1) / TPB, NRT = (RTW + TPB - 1) / TPB, NRV = (RVW + TPB - 1) / TPB, NCM = (CMW + TPB - 1) / TPB;
    const float *cf = contact_forces + (size_t)e0 * dwe::NB * 3;
    const int ncf = ne * dwe::NB * 3;
    float4 vcf[NCF];
    float vrt[NRT], vrv[NRV], vcm[NCM];
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
    span_load<RTW>(vrt, root_states + (size_t)e0 * 13, ne * 13, t);
    span_load<RVW>(vrv, reward_values + (size_t)e0 * DWE_REW_TERMS, ne * DWE_REW_TERMS, t);
    span_load<CMW>(vcm, commands + (size_t)e0 * 3, ne * 3, t);
    const bool own = t < ne;
    const int e = e0 + (own ? t : 0);
    const dwe::Rows r{st, ac, n, e};
    dwe::EnvIn in;
    dwe::St s;
    dwe::AcHot h;
    if (own) {
        const float *bp = rigid_body_pos + (size_t)e * dwe::NB * 3;
        in.zl = bp[DWE_LFOOT * 3 + 2];
        in.zr = bp[DWE_RFOOT * 3 + 2];
        in.rew = rew_buf[e];
        in.total_mass = total_mass[e];
        in.p = (int)progress_buf[e];
        in.reset = reset_buf[e] != 0;
        s = dwe::load(r);
        h = dwe::load_hot(r);
    }
    // ---- into LDS; the bodies with a component over 1 as a bit mask per env (one lane per env and body) ----
#pragma unroll
    for (int k = 0; k < NCF; ++k) {
        const int i = t + k * TPB;
        if (i < CFW / 4) s_cf4[i] = vcf[k];
    }
    span_store<RTW>(s_root, vrt, t);
    span_store<RVW>(s_rv, vrv, t);
    span_store<CMW>(s_cmd, vcm, t);
    for (int i = t; i < EPB * 2; i += TPB) s_mask[i >> 1][i & 1] = 0u;
    for (int i = t; i < DWE_CT_WINDOW; i += TPB) s_ct[i] = 0u;
    __syncthreads();
    for (int i = t; i < ne * dwe::NB; i += TPB) {
        const int el = i / dwe::NB, g = i - dwe::NB * el;
        const float *f = s_cf + 3 * i;
        if (g != DWE_LFOOT && g != DWE_RFOOT && dwe::over_1(f[0], f[1], f[2])) atomicOr(&s_mask[el][g >> 5], 1u << (g & 31));
    }
    __syncthreads();
    // ---- one lane per env ----
    if (own) {
        in.root = s_root + t * 13;
        in.rv = s_rv + t * DWE_REW_TERMS;
        in.cmd = s_cmd + t * 3;
        in.fzl = s_cf[(t * dwe::NB + DWE_LFOOT) * 3 + 2];
        in.fzr = s_cf[(t * dwe::NB + DWE_RFOOT) * 3 + 2];
        LdsCount c{s_ct};
        int bin;
        cause[e] = (uint8_t)dwe::update(in, s_mask[t][0], s_mask[t][1], s, h, r, c, C, bin);
        dwe::store(r, s);
        dwe::store_hot(r, h, bin);
    }
    if (blockIdx.x == 0 && t == 0) dwe::count_call(reinterpret_cast<uint64_t *>(ct));
    __syncthreads();
    for (int i = t; i < DWE_CT_WINDOW; i += TPB) {
        const unsigned int v = s_ct[i];
        if (v == 0u || i == DWE_CT_RECORDS) continue;
        if (i == DWE_CT_LEN_MAX) atomicMax(&ct[i], (unsigned long long)v);
        else atomicAdd(&ct[i], (unsigned long long)v);
    }
}

// one workgroup per float word of ac (word blockIdx.x); workgroup 0 also converts the counts
__global__ __launch_bounds__(dwe::RT) void dwe_k_summarize(int n, const float *__restrict__ ac, const unsigned long long *__restrict__ ct, double *out) {
    __shared__ double red[dwe::RT];
    const int t = threadIdx.x, k = blockIdx.x;
    if (k == 0)
        for (int i = t; i < DWE_CT_WORDS; i += dwe::RT) out[i] = (double)ct[i];
    red[t] = dwe::partial(ac + (size_t)k * n, n, t);
    __syncthreads();
    for (int s = dwe::RT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) out[DWE_SUM_AC + k] = red[0];
}

}  // namespace

extern "C" {

int dwe_abi_version(void) { return DWE_ABI_VERSION; }
const char *dwe_last_error(void) { return s_err; }

int dwe_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *rigid_body_pos, const float *commands,
               const float *rew_buf, const float *reward_values, const int64_t *reset_buf, const int64_t *progress_buf, const float *total_mass,
               void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float termination_height,
               int32_t enable_early_termination, float command_x_lo, float command_x_hi, void *stream) {
    if (num_envs < 1) return fail("dwe_record: num_envs must be positive");
    if (!root_states || !contact_forces || !rigid_body_pos || !commands || !rew_buf || !reward_values || !reset_buf || !progress_buf ||
        !total_mass || !st || !ac || !ct || !cause)
        return fail("dwe_record: a buffer is missing");
    if (!(max_episode_length > 0.0f)) return fail("dwe_record: max_episode_length must be positive");
    if ((reinterpret_cast<uintptr_t>(contact_forces) & 15u) != 0u) return fail("dwe_record: contact_forces must be 16-byte aligned");
    dwe::Cfg C;
    C.max_len = max_episode_length; C.term_h = termination_height; C.cmd_lo = command_x_lo; C.cmd_hi = command_x_hi;
    C.eet = enable_early_termination != 0;
    hipLaunchKernelGGL(dwe_k_record, dim3((num_envs + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, root_states, contact_forces,
                       rigid_body_pos, commands, rew_buf, reward_values, reset_buf, progress_buf, total_mass, (uint32_t *)st, ac,
                       (unsigned long long *)ct, cause, C);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip("dwe_record: launch", e);
}

int dwe_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream) {
    if (num_envs < 1) return fail("dwe_summarize: num_envs must be positive");
    if (!ac || !ct || !out) return fail("dwe_summarize: a buffer is missing");
    hipLaunchKernelGGL(dwe_k_summarize, dim3(DWE_AC_WORDS), dim3(dwe::RT), 0, (hipStream_t)stream, (int)num_envs, ac, (const unsigned long long *)ct, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip("dwe_summarize: launch", e);
}

}  // extern "C"
