// dw_stats.hip -- the kernels of DyrosDynamicWalk's episode statistics (include/dyros_stats.h).  The per-env logic is
// dw_stats.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   k_record     one launch per step.  A workgroup of 128 lanes takes 32 envs: their contact rows (32 x 456 B, one contiguous span),
//                root rows and the 12 action_torque words of their env_state rows are staged in LDS with consecutive lanes on consecutive words; the
//                bodies over 1 N become a bit mask per env (one lane per env and body); then one lane per env runs dws::update, its integer
//                counts gathered in LDS and added to ct with one atomic per non-zero word and workgroup.
//   k_restart    one lane per listed env (or every env).
//   k_summarize  one workgroup per float word of ac: every sum in dws's fixed order; the counts converted.
#include "dw_record_group.h"
#include "dw_stats.h"

namespace {

grp::Err s_err;

using rec::EPB;
using rec::TPB;
constexpr int RTW = EPB * 13, TQW = 12;             // root words of a workgroup; action_torque words of an env

__global__ __launch_bounds__(TPB) void dws_k_record(int n, const float *__restrict__ root_states, const float *__restrict__ contact_forces,
                                                    const float *__restrict__ env_state, const int64_t *__restrict__ reset_buf,
                                                    const float *__restrict__ total_mass, uint32_t *__restrict__ st, float *__restrict__ ac,
                                                    unsigned long long *ct, uint8_t *cause, float max_len, float dt_policy) {
    __shared__ float4 s_cf4[rec::CFW / 4];
    __shared__ float s_root[RTW];
    __shared__ float s_tq[EPB * TQW];
    __shared__ unsigned int s_mask[EPB][2];
    __shared__ unsigned int s_ct[DWS_CT_WINDOW];
    float *s_cf = reinterpret_cast<float *>(s_cf4);
    const int t = threadIdx.x, e0 = blockIdx.x * EPB;
    const int ne = n - e0 < EPB ? n - e0 : EPB;          // envs of this workgroup (the last one may hold fewer)
    // ---- every global load first, into registers: the contact rows, the root rows, the torque words (a strided gather from env_state);
    //      and on lanes 0 .. ne - 1 the env's own words and its running state ----
    float4 vcf[rec::NCF];
    float vrt[rec::regs(RTW)], vtq[rec::regs(EPB * TQW)];
    rec::contact_load(vcf, contact_forces, e0, ne, t);
    rec::span_load<RTW>(vrt, root_states + (size_t)e0 * 13, ne * 13, t);
#pragma unroll
    for (int k = 0; k < rec::regs(EPB * TQW); ++k) {
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
    // ---- into LDS; the bodies over 1 N as a bit mask per env ----
    rec::contact_store(s_cf4, vcf, t);
    rec::span_store<RTW>(s_root, vrt, t);
    rec::span_store<EPB * TQW>(s_tq, vtq, t);
    rec::zero_counts<DWS_CT_WINDOW>(s_mask, s_ct, t);
    __syncthreads();
    rec::mask_pass<DWS_LFOOT, DWS_RFOOT>(s_cf, s_mask, ne, t, dws::Over1N{});
    __syncthreads();
    // ---- one lane per env ----
    if (own) {
        in.cf = s_cf + t * dws::NB * 3;
        in.root = s_root + t * 13;
        in.tq = s_tq + t * TQW;
        rec::LdsCount c{s_ct};
        cause[e] = (uint8_t)dws::update(in, s_mask[t][0], s_mask[t][1], s, h, r, c, max_len, dt_policy);
        dws::store(r, s);
        dws::store_hot(r, h);
    }
    if (blockIdx.x == 0 && t == 0) dws::count_call(reinterpret_cast<uint64_t *>(ct), reinterpret_cast<const int *>(env_state)[DW_ES_PERT_START]);
    __syncthreads();
    rec::flush<DWS_CT_WINDOW, DWS_CT_RECORDS, DWS_CT_LEN_MAX>(s_ct, ct, t);
}

__global__ __launch_bounds__(256) void dws_k_restart(int n, const int32_t *__restrict__ ids, int num_ids, const float *__restrict__ root_states,
                                                     const float *__restrict__ env_state, const int64_t *__restrict__ progress_buf, uint32_t *st) {
    int e;
    if (!grp::listed_env(ids, num_ids, n, e)) return;
    const float *es = env_state + (size_t)e * dws::ESW;
    const int *esi = reinterpret_cast<const int *>(es);
    dws::St s;
    dws::begin(s, (int)progress_buf[e], root_states + (size_t)e * 13, es[DW_ES_TARGET_VEL], esi[DW_ES_PERT_ON] ? 1 : 0, esi[DW_ES_NAN_RESETS]);
    dws::store(dws::Rows{st, nullptr, n, e}, s);
}

__global__ __launch_bounds__(dws::RT) void dws_k_summarize(int n, const float *__restrict__ ac, const unsigned long long *__restrict__ ct, double *out) {
    rec::summarize<DWS_CT_WORDS, DWS_SUM_AC>(n, ac, ct, out);
}

}  // namespace

extern "C" {

int dws_abi_version(void) { return DWS_ABI_VERSION; }
const char *dws_last_error(void) { return s_err.s; }

int dws_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *env_state, const int64_t *reset_buf,
               const float *total_mass, void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float dt_policy,
               void *stream) {
    if (num_envs < 1) return s_err.fail("dws_record: num_envs must be positive");
    if (!root_states || !contact_forces || !env_state || !reset_buf || !total_mass || !st || !ac || !ct || !cause)
        return s_err.fail("dws_record: a buffer is missing");
    if (!(max_episode_length > 0.0f)) return s_err.fail("dws_record: max_episode_length must be positive");
    if ((reinterpret_cast<uintptr_t>(contact_forces) & 15u) != 0u) return s_err.fail("dws_record: contact_forces must be 16-byte aligned");
    hipLaunchKernelGGL(dws_k_record, dim3((num_envs + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, root_states, contact_forces,
                       env_state, reset_buf, total_mass, (uint32_t *)st, ac, (unsigned long long *)ct, cause, max_episode_length, dt_policy);
    return s_err.launched("dws_record");
}

int dws_restart(int32_t num_envs, const int32_t *env_ids, int32_t num_ids, const float *root_states, const float *env_state,
                const int64_t *progress_buf, void *st, void *stream) {
    if (num_envs < 1) return s_err.fail("dws_restart: num_envs must be positive");
    if (!root_states || !env_state || !progress_buf || !st) return s_err.fail("dws_restart: a buffer is missing");
    const int m = s_err.listed("dws_restart", env_ids, num_ids, num_envs, num_envs);
    if (m <= 0) return m;
    hipLaunchKernelGGL(dws_k_restart, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)num_envs, env_ids, m, root_states, env_state,
                       progress_buf, (uint32_t *)st);
    return s_err.launched("dws_restart");
}

int dws_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream) {
    if (num_envs < 1) return s_err.fail("dws_summarize: num_envs must be positive");
    if (!ac || !ct || !out) return s_err.fail("dws_summarize: a buffer is missing");
    hipLaunchKernelGGL(dws_k_summarize, dim3(DWS_AC_WORDS), dim3(dws::RT), 0, (hipStream_t)stream, (int)num_envs, ac, (const unsigned long long *)ct, out);
    return s_err.launched("dws_summarize");
}

}  // extern "C"
