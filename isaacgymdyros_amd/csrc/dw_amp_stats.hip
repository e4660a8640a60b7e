// dw_amp_stats.hip -- the kernels of TocabiAMPLower's episode statistics (include/dyros_amp_stats.h).  The per-env logic is
// dw_amp_stats.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwe_k_record     one launch per step, the shape of dws_k_record (dw_stats.hip).  A workgroup of 128 lanes takes 32 envs: their contact rows
//                    (32 x 456 B, one contiguous span), root rows, reward_values and commands rows are staged in LDS with consecutive lanes on
//                    consecutive words; the bodies with a component over 1 become a bit mask per env (one lane per env and body); then one lane
//                    per env runs dwe::update, its integer counts gathered in LDS and added to ct with one atomic per non-zero word and workgroup.
//   dwe_k_summarize  one workgroup per float word of ac: every sum in dwe's fixed order; the counts converted.
#include "dw_record_group.h"
#include "dw_amp_stats.h"

namespace {

grp::Err s_err;

using rec::EPB;
using rec::TPB;
constexpr int RTW = EPB * 13, RVW = EPB * DWE_REW_TERMS, CMW = EPB * 3;
static_assert(dwe::NB == rec::NB, "contact_forces rows");
static_assert(DWE_CT_WINDOW <= TPB, "one lane per count word");

__global__ __launch_bounds__(TPB) void dwe_k_record(int n, const float *__restrict__ root_states, const float *__restrict__ contact_forces,
                                                    const float *__restrict__ rigid_body_pos, const float *__restrict__ commands,
                                                    const float *__restrict__ rew_buf, const float *__restrict__ reward_values,
                                                    const int64_t *__restrict__ reset_buf, const int64_t *__restrict__ progress_buf,
                                                    const float *__restrict__ total_mass, uint32_t *__restrict__ st, float *__restrict__ ac,
                                                    unsigned long long *ct, uint8_t *cause, dwe::Cfg C) {
    __shared__ float4 s_cf4[rec::CFW / 4];
    __shared__ float s_root[RTW];
    __shared__ float s_rv[RVW];
    __shared__ float s_cmd[CMW];
    __shared__ unsigned int s_mask[EPB][2];
    __shared__ unsigned int s_ct[DWE_CT_WINDOW];
    float *s_cf = reinterpret_cast<float *>(s_cf4);
    const int t = threadIdx.x, e0 = blockIdx.x * EPB;
    const int ne = n - e0 < EPB ? n - e0 : EPB;          // envs of this workgroup (the last one may hold fewer)
    // ---- every global load first, into registers: the contact rows, the root / reward_values / commands rows; and on lanes 0 .. ne - 1
    //      the env's own words and its running state.  The contact load is rec::contact_load's text, spelled out: called as a function it
    //      changed this kernel's schedule, and the record's median was 0.11 us over the parent's slowest round (profiles/recorder_stages.txt) ----
    float4 vcf[rec::NCF];
    float vrt[rec::regs(RTW)], vrv[rec::regs(RVW)], vcm[rec::regs(CMW)];
    const float *cf = contact_forces + (size_t)e0 * rec::NB * 3;
    const int ncf = ne * rec::NB * 3;
#pragma unroll
    for (int k = 0; k < rec::NCF; ++k) {
        const int i = t + k * TPB;
        if (ne == EPB) {
            if (i < rec::CFW / 4) vcf[k] = reinterpret_cast<const float4 *>(cf)[i];
        } else {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (4 * i + 0 < ncf) v.x = cf[4 * i + 0];
            if (4 * i + 1 < ncf) v.y = cf[4 * i + 1];
            if (4 * i + 2 < ncf) v.z = cf[4 * i + 2];
            if (4 * i + 3 < ncf) v.w = cf[4 * i + 3];
            vcf[k] = v;
        }
    }
    rec::span_load<RTW>(vrt, root_states + (size_t)e0 * 13, ne * 13, t);
    rec::span_load<RVW>(vrv, reward_values + (size_t)e0 * DWE_REW_TERMS, ne * DWE_REW_TERMS, t);
    rec::span_load<CMW>(vcm, commands + (size_t)e0 * 3, ne * 3, t);
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
    // ---- into LDS; the bodies with a component over 1 as a bit mask per env ----
    rec::contact_store(s_cf4, vcf, t);
    rec::span_store<RTW>(s_root, vrt, t);
    rec::span_store<RVW>(s_rv, vrv, t);
    rec::span_store<CMW>(s_cmd, vcm, t);
    rec::zero_counts<DWE_CT_WINDOW>(s_mask, s_ct, t);
    __syncthreads();
    rec::mask_pass<DWE_LFOOT, DWE_RFOOT>(s_cf, s_mask, ne, t, dwe::Over1{});
    __syncthreads();
    // ---- one lane per env ----
    if (own) {
        in.root = s_root + t * 13;
        in.rv = s_rv + t * DWE_REW_TERMS;
        in.cmd = s_cmd + t * 3;
        in.fzl = s_cf[(t * dwe::NB + DWE_LFOOT) * 3 + 2];
        in.fzr = s_cf[(t * dwe::NB + DWE_RFOOT) * 3 + 2];
        rec::LdsCount c{s_ct};
        int bin;
        cause[e] = (uint8_t)dwe::update(in, s_mask[t][0], s_mask[t][1], s, h, r, c, C, bin);
        dwe::store(r, s);
        dwe::store_hot(r, h, bin);
    }
    if (blockIdx.x == 0 && t == 0) dwe::count_call(reinterpret_cast<uint64_t *>(ct));
    __syncthreads();
    rec::flush<DWE_CT_WINDOW, DWE_CT_RECORDS, DWE_CT_LEN_MAX>(s_ct, ct, t);
}

__global__ __launch_bounds__(dwe::RT) void dwe_k_summarize(int n, const float *__restrict__ ac, const unsigned long long *__restrict__ ct, double *out) {
    rec::summarize<DWE_CT_WORDS, DWE_SUM_AC>(n, ac, ct, out);
}

}  // namespace

extern "C" {

int dwe_abi_version(void) { return DWE_ABI_VERSION; }
const char *dwe_last_error(void) { return s_err.s; }

int dwe_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *rigid_body_pos, const float *commands,
               const float *rew_buf, const float *reward_values, const int64_t *reset_buf, const int64_t *progress_buf, const float *total_mass,
               void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float termination_height,
               int32_t enable_early_termination, float command_x_lo, float command_x_hi, void *stream) {
    if (num_envs < 1) return s_err.fail("dwe_record: num_envs must be positive");
    if (!root_states || !contact_forces || !rigid_body_pos || !commands || !rew_buf || !reward_values || !reset_buf || !progress_buf ||
        !total_mass || !st || !ac || !ct || !cause)
        return s_err.fail("dwe_record: a buffer is missing");
    if (!(max_episode_length > 0.0f)) return s_err.fail("dwe_record: max_episode_length must be positive");
    if ((reinterpret_cast<uintptr_t>(contact_forces) & 15u) != 0u) return s_err.fail("dwe_record: contact_forces must be 16-byte aligned");
    dwe::Cfg C;
    C.max_len = max_episode_length; C.term_h = termination_height; C.cmd_lo = command_x_lo; C.cmd_hi = command_x_hi;
    C.eet = enable_early_termination != 0;
    hipLaunchKernelGGL(dwe_k_record, dim3((num_envs + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, root_states, contact_forces,
                       rigid_body_pos, commands, rew_buf, reward_values, reset_buf, progress_buf, total_mass, (uint32_t *)st, ac,
                       (unsigned long long *)ct, cause, C);
    return s_err.launched("dwe_record");
}

int dwe_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream) {
    if (num_envs < 1) return s_err.fail("dwe_summarize: num_envs must be positive");
    if (!ac || !ct || !out) return s_err.fail("dwe_summarize: a buffer is missing");
    hipLaunchKernelGGL(dwe_k_summarize, dim3(DWE_AC_WORDS), dim3(dwe::RT), 0, (hipStream_t)stream, (int)num_envs, ac, (const unsigned long long *)ct, out);
    return s_err.launched("dwe_summarize");
}

}  // extern "C"
