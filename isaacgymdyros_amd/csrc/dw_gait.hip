// dw_gait.hip -- the kernels of DyrosDynamicWalk's gait profile (include/dyros_gait.h).  The per-env sample is
// dw_gait.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   k_record     one launch per step.  A workgroup of 256 lanes takes DWG_GROUP = 64 envs.  Every global load is issued before the first store:
//                the 36 joint words of each env (12 dof_pos, 12 target_qpos, 12 action_torque) with consecutive lanes on consecutive words of
//                a 12-word run, staged in LDS; and on lanes 0 .. 63 the env's own scalars.  One lane per env then runs dwg::sample, which
//                adds its non-zero words to a [B][40] int64 table in LDS with LDS integer atomics.  The rows of the bins that were touched
//                are then added, non-zero words only, to the workgroup's own partial table in global memory (plain read-modify-writes: no
//                other workgroup touches it), and the four counters with one 64-bit atomic each.
//   k_summarize  one lane per table word: the sum of the partial tables in workgroup order (any order gives the same integers).
//   k_clear      zeroes the partial tables and the counters.
#include "dw_group.h"
#include "dw_gait.h"

namespace {

grp::Err s_err;

constexpr int EPB = DWG_GROUP, TPB = 256;
constexpr int JW = 3 * dwg::NJ;                       // staged words per env: dof_pos, target_qpos, action_torque
constexpr int NST = (EPB * JW + TPB - 1) / TPB;       // staged words per lane
constexpr int TABLE = DWG_BINS_MAX * dwg::W;
static_assert(EPB <= TPB && TPB % 64 == 0, "one lane per env");
static_assert(TABLE % 2 == 0, "the table is zeroed in 16-byte pieces");
static_assert(TABLE * 8 + EPB * JW * 4 + DWG_BINS_MAX * 4 + 16 <= 64 * 1024, "static LDS");

struct LdsAdd {
    unsigned long long *table;
    unsigned int *used;
    __device__ void bin(int b) const { used[b] = 1u; }
    __device__ void add(int b, int w, int64_t v) const {
        if (v != 0) atomicAdd(&table[b * dwg::W + w], (unsigned long long)v);
    }
};

__global__ __launch_bounds__(TPB) void dwg_k_record(int n, int bins, int min_step, int skip_pushes, const float *__restrict__ root_states,
                                                    const float *__restrict__ dof_state, const float *__restrict__ contact_forces,
                                                    const float *__restrict__ env_state, const float *__restrict__ stacked_rewards,
                                                    const int64_t *__restrict__ reset_buf, const int64_t *__restrict__ progress_buf,
                                                    const float *__restrict__ total_mass, long long *part, unsigned long long *ct) {
    __shared__ ulonglong2 s_table2[TABLE / 2];
    __shared__ float s_jw[EPB * JW];
    __shared__ unsigned int s_used[DWG_BINS_MAX];
    __shared__ unsigned int s_ct[DWG_CT_WORDS];
    unsigned long long *s_table = reinterpret_cast<unsigned long long *>(s_table2);
    const int t = threadIdx.x, e0 = blockIdx.x * EPB;
    const int ne = n - e0 < EPB ? n - e0 : EPB;          // envs of this workgroup (the last one may hold fewer)
    const int words = bins * dwg::W;
    // ---- every global load first ----
    float vst[NST];
#pragma unroll
    for (int k = 0; k < NST; ++k) {
        const int i = t + k * TPB, el = i / JW, w = i - JW * el;
        float x = 0.0f;
        if (el < ne) {
            const size_t e = (size_t)(e0 + el);
            x = w < dwg::NJ ? dof_state[e * (2 * DW_NUM_DOF) + 2 * w]
              : w < 2 * dwg::NJ ? env_state[e * dwg::ESW + DW_ES_TARGET_QPOS + (w - dwg::NJ)]
                                : env_state[e * dwg::ESW + DW_ES_ACTION_TORQUE + (w - 2 * dwg::NJ)];
        }
        vst[k] = x;
    }
    const bool own = t < ne;
    dwg::EnvIn in;
    if (own) {
        const size_t e = (size_t)(e0 + t);
        const float *es = env_state + e * dwg::ESW;
        const int *esi = reinterpret_cast<const int *>(es);
        const float *cf = contact_forces + e * (DW_NUM_BODIES * 3);
        in.fl = cf[3 * DWS_LFOOT + 2];
        in.fr = cf[3 * DWS_RFOOT + 2];
        in.total_mass = total_mass[e];
        in.tf0 = es[DW_ES_TARGET_FORCE];
        in.tf1 = es[DW_ES_TARGET_FORCE + 1];
        in.root_z = root_states[e * 13 + 2];
        in.root_vx = root_states[e * 13 + 7];
        in.tv0 = es[DW_ES_TARGET_VEL];
        in.paid = stacked_rewards[e * DW_NUM_REW + DWG_PAID_COLUMN];
        in.mocap_idx = esi[DW_ES_MOCAP_IDX];
        in.pert_on = esi[DW_ES_PERT_ON];
        in.reset = reset_buf[e] != 0;
        in.progress = progress_buf[e];
    }
    // ---- LDS: the table zeroed, the joint words staged ----
    for (int i = t; i < words / 2; i += TPB) s_table2[i] = make_ulonglong2(0ull, 0ull);
    for (int i = t; i < bins; i += TPB) s_used[i] = 0u;
    if (t < DWG_CT_WORDS) s_ct[t] = 0u;
#pragma unroll
    for (int k = 0; k < NST; ++k) {
        const int i = t + k * TPB;
        if (i < EPB * JW) s_jw[i] = vst[k];
    }
    __syncthreads();
    // ---- one lane per env ----
    if (own) {
        in.dof_pos = s_jw + t * JW;
        in.dof_stride = 1;
        in.tqpos = s_jw + t * JW + dwg::NJ;
        in.tq = s_jw + t * JW + 2 * dwg::NJ;
        const LdsAdd a{s_table, s_used};
        atomicAdd(&s_ct[dwg::sample(in, bins, min_step, skip_pushes, a)], 1u);
    }
    __syncthreads();
    // ---- the touched rows into this workgroup's partial table ----
    long long *mine = part + (size_t)blockIdx.x * words;
    for (int i = t; i < words; i += TPB) {
        if (s_used[i / dwg::W] == 0u) continue;
        const long long v = (long long)s_table[i];
        if (v != 0) mine[i] += v;
    }
    if (t < DWG_CT_WORDS && s_ct[t] != 0u) atomicAdd(&ct[t], (unsigned long long)s_ct[t]);
}

__global__ __launch_bounds__(256) void dwg_k_summarize(int groups, int words, const long long *__restrict__ part,
                                                       const long long *__restrict__ ct, long long *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) {
        long long s = 0;
        for (int g = 0; g < groups; ++g) s += part[(size_t)g * words + i];
        out[i] = s;
    } else if (i < words + DWG_CT_WORDS) {
        out[i] = ct[i - words];
    }
}

__global__ __launch_bounds__(256) void dwg_k_clear(size_t words, long long *part, long long *ct) {
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < words; i += (size_t)gridDim.x * blockDim.x) part[i] = 0;
    if (i0 < DWG_CT_WORDS) ct[i0] = 0;
}

int check_shape(const char *who, int32_t num_envs, int32_t bins) {
    if (s_err.envs(who, num_envs, EPB) != 0) return -1;
    return dwg::bins_ok(bins) ? 0 : s_err.fail(who, "bins must be one of 12, 24, 36, 72, 144");
}

}  // namespace

extern "C" {

int dwg_abi_version(void) { return DWG_ABI_VERSION; }
const char *dwg_last_error(void) { return s_err.s; }

int64_t dwg_groups(int32_t num_envs) {
    if (num_envs < 1 || num_envs > 0x7fffffff - EPB) return -1;
    return dwg::groups(num_envs);
}

int dwg_record(int32_t num_envs, int32_t bins, int32_t min_episode_step, int32_t skip_pushes, const float *root_states, const float *dof_state,
               const float *contact_forces, const float *env_state, const float *stacked_rewards, const int64_t *reset_buf,
               const int64_t *progress_buf, const float *total_mass, int64_t *part, int64_t *ct, void *stream) {
    if (check_shape("dwg_record", num_envs, bins) != 0) return -1;
    if (min_episode_step < 0) return s_err.fail("dwg_record: min_episode_step must not be negative");
    if (!root_states || !dof_state || !contact_forces || !env_state || !stacked_rewards || !reset_buf || !progress_buf || !total_mass || !part || !ct)
        return s_err.fail("dwg_record: a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(part) & 7u) != 0u || (reinterpret_cast<uintptr_t>(ct) & 7u) != 0u)
        return s_err.fail("dwg_record: part and ct must be 8-byte aligned");
    hipLaunchKernelGGL(dwg_k_record, dim3(dwg::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, (int)bins, (int)min_episode_step,
                       (int)(skip_pushes != 0), root_states, dof_state, contact_forces, env_state, stacked_rewards, reset_buf, progress_buf, total_mass,
                       (long long *)part, (unsigned long long *)ct);
    return s_err.launched("dwg_record");
}

int dwg_clear(int32_t num_envs, int32_t bins, int64_t *part, int64_t *ct, void *stream) {
    if (check_shape("dwg_clear", num_envs, bins) != 0) return -1;
    if (!part || !ct) return s_err.fail("dwg_clear: a buffer is missing");
    const size_t words = (size_t)dwg::groups(num_envs) * bins * dwg::W;
    const size_t blocks = (words + 255) / 256;
    hipLaunchKernelGGL(dwg_k_clear, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, words, (long long *)part,
                       (long long *)ct);
    return s_err.launched("dwg_clear");
}

int dwg_summarize(int32_t num_envs, int32_t bins, const int64_t *part, const int64_t *ct, int64_t *out, void *stream) {
    if (check_shape("dwg_summarize", num_envs, bins) != 0) return -1;
    if (!part || !ct || !out) return s_err.fail("dwg_summarize: a buffer is missing");
    const int words = bins * dwg::W;
    hipLaunchKernelGGL(dwg_k_summarize, dim3((words + DWG_CT_WORDS + 255) / 256), dim3(256), 0, (hipStream_t)stream, dwg::groups(num_envs), words,
                       (const long long *)part, (const long long *)ct, (long long *)out);
    return s_err.launched("dwg_summarize");
}

}  // extern "C"
