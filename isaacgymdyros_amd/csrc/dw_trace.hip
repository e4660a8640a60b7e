// dw_trace.hip -- the kernels of DyrosDynamicWalk's run trace (include/dyros_trace.h).  The row assembly and the slot
// state are dw_trace.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwt_k_record  one launch per step.  One wavefront per slot, four slots per workgroup of 256 lanes.  A held slot leaves after bumping
//                 `seen` (wave-uniform).  Otherwise every global load is issued first -- per source span, consecutive lanes on consecutive
//                 words: 13 root words, the 66 interleaved dof_state words, the env_state spans, 114 contact words, 15 + 1 reward words --
//                 then the row is put together in LDS (the de-interleave of dof_state happens there), the non-foot maximum is a wave
//                 reduction, and the row leaves as 52 16-byte stores of consecutive lanes.  Plain stores, no atomics: one wave owns a slot.
//   dwt_k_arm     one lane per listed env (or every env).
//   dwt_k_gather  one wavefront per output row, the same 16 bytes per lane.
#include "dw_group.h"
#include "dw_trace.h"

namespace {

grp::Err s_err;

constexpr int WAVE = 64, SPB = 4, TPB = SPB * WAVE;          // slots (wavefronts) and lanes per workgroup
constexpr int ROW4 = dwt::ROW / 4;                            // 16-byte pieces of a row
constexpr int CFP = (dwt::CFW + 3) / 4 * 4;                   // a wave's contact words in LDS
static_assert(ROW4 <= WAVE, "a row is one 16-byte store per lane");
static_assert(dwt::CFW <= 2 * WAVE && dwt::NB <= WAVE, "a contact row is two loads per lane, one body per lane");

// lanes of one wavefront exchange through LDS
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(TPB) void dwt_k_record(int n, int k, int depth, int hold_mode, const int32_t *__restrict__ slot_env,
                                                    const float *__restrict__ root_states, const float *__restrict__ dof_state,
                                                    const float *__restrict__ contact_forces, const float *__restrict__ env_state,
                                                    const float *__restrict__ rew_buf, const float *__restrict__ stacked_rewards,
                                                    const int64_t *__restrict__ reset_buf, const int64_t *__restrict__ timeout_buf, float max_len,
                                                    uint32_t *__restrict__ ss, float4 *__restrict__ ring) {
    __shared__ float4 s_row4[SPB][ROW4];
    __shared__ float s_cf[SPB][CFP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int s = blockIdx.x * SPB + w;
    if (s >= k) return;                                   // (wave-uniform, as every branch on s, e and t below)
    const int e = slot_env[s];
    dwt::Slot t = dwt::load(ss, k, s);
    const bool no_env = e < 0 || e >= n;                  // a slot table that names no env of this launch writes nothing
    t.seen += 1u;
    if (no_env | (t.held != 0u)) {                        // (one branch on both loads: they travel together)
        if (!no_env && lane == 0) ss[(size_t)DWT_SS_SEEN * k + s] = t.seen;
        return;
    }
    // ---- every global load first, into registers ----
    const dwt::Src src = dwt::rows_of(e, root_states, dof_state, env_state, rew_buf, stacked_rewards);
    float v[dwt::NSPAN];
#pragma unroll
    for (int q = 0; q < dwt::NSPAN; ++q) {
        const dwt::Span sp = dwt::span(q);
        v[q] = lane < sp.len ? src.p[sp.buf][sp.src + lane] : 0.0f;
    }
    const float *cf = contact_forces + (size_t)e * dwt::CFW;
    const float c0 = cf[lane], c1 = lane + WAVE < dwt::CFW ? cf[lane + WAVE] : 0.0f;
    const int *esi = reinterpret_cast<const int *>(src.p[dwt::B_ES]);
    const int pert_on = esi[DW_ES_PERT_ON], pert_start = esi[DW_ES_PERT_START], nan_resets = esi[DW_ES_NAN_RESETS];
    const bool reset = reset_buf[e] != 0, timeout = timeout_buf[e] != 0;
    // ---- the row in LDS ----
    float *row = reinterpret_cast<float *>(s_row4[w]);
#pragma unroll
    for (int q = 0; q < dwt::NSPAN; ++q) {
        const dwt::Span sp = dwt::span(q);
        if (lane < sp.len) row[dwt::dst_of(sp, lane)] = v[q];
    }
    s_cf[w][lane] = c0;
    if (lane + WAVE < dwt::CFW) s_cf[w][lane + WAVE] = c1;
    const dwt::Step o = dwt::advance(t, depth, hold_mode, reset, timeout, pert_on, pert_start, nan_resets, max_len);
    if (lane < 4) row[lane] = dwt::u2f(lane == 0 ? o.head[0] : lane == 1 ? o.head[1] : lane == 2 ? o.head[2] : o.head[3]);
    if (lane < DWT_LEN_PAD) row[DWT_CH_PAD + lane] = 0.0f;
    wave_sync();
    // ---- the soles' rows; the largest |F| of the other bodies: one body per lane, then a butterfly (every lane ends with the winner) ----
    dwt::Cand c = dwt::cand_of(s_cf[w], lane);
#pragma unroll
    for (int x = WAVE / 2; x >= 1; x >>= 1) {
        dwt::Cand d;
        d.key = __shfl_xor(c.key, x, WAVE);
        d.g = __shfl_xor(c.g, x, WAVE);
        d.v = __shfl_xor(c.v, x, WAVE);
        c = dwt::better(c, d);
    }
    if (lane < DWT_LEN_FOOT_FORCE) row[DWT_CH_FOOT_FORCE + lane] = s_cf[w][lane < 3 ? 3 * DWS_LFOOT + lane : 3 * DWS_RFOOT + lane - 3];
    if (lane == 0) {
        row[DWT_CH_NF_MAX] = c.v;
        row[DWT_CH_NF_BODY] = (float)c.g;
    }
    wave_sync();
    // ---- out: 52 consecutive 16-byte pieces ----
    if (lane < ROW4) ring[((size_t)s * depth + o.at) * ROW4 + lane] = s_row4[w][lane];
    if (lane == 0) dwt::store(ss, k, s, t);
}

__global__ __launch_bounds__(256) void dwt_k_arm(int n, int k, const int32_t *__restrict__ ids, int num_ids, const int64_t *__restrict__ progress_buf,
                                                 const int32_t *__restrict__ env_slot, uint32_t *ss) {
    int e;
    if (!grp::listed_env(ids, num_ids, n, e)) return;
    const int s = env_slot[e];
    if (s < 0 || s >= k) return;
    dwt::Slot t;
    dwt::arm(t, progress_buf[e]);
    dwt::store(ss, k, s, t);
}

__global__ __launch_bounds__(TPB) void dwt_k_gather(int k, int depth, const int32_t *__restrict__ slot_ids, int num_ids, const uint32_t *__restrict__ ss,
                                                    const float4 *__restrict__ ring, float4 *__restrict__ out, int32_t *__restrict__ out_rows) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int gw = blockIdx.x * SPB + threadIdx.x / WAVE;          // output row (num_ids * depth < 2^31: dwt_gather)
    if (gw >= num_ids * depth) return;
    const int i = gw / depth;
    const uint32_t r = (uint32_t)(gw - i * depth);
    const int s = slot_ids ? slot_ids[i] : i;
    const bool ok = s >= 0 && s < k;
    const uint32_t cursor = ok ? ss[(size_t)DWT_SS_CURSOR * k + s] : 0u;
    const uint32_t nr = dwt::rows(cursor, depth);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < nr && lane < ROW4) v = ring[((size_t)s * depth + dwt::src_row(cursor, depth, r)) * ROW4 + lane];
    if (lane < ROW4) out[(size_t)gw * ROW4 + lane] = v;
    if (r == 0u && lane == 0) out_rows[i] = (int32_t)nr;
}

}  // namespace

extern "C" {

int dwt_abi_version(void) { return DWT_ABI_VERSION; }
const char *dwt_last_error(void) { return s_err.s; }

int dwt_record(int32_t num_envs, int32_t num_slots, int32_t depth, int32_t hold_mode, const int32_t *slot_env, const float *root_states,
               const float *dof_state, const float *contact_forces, const float *env_state, const float *rew_buf,
               const float *stacked_rewards, const int64_t *reset_buf, const int64_t *timeout_buf, float max_episode_length, void *ss,
               void *ring, void *stream) {
    if (num_envs < 1) return s_err.fail("dwt_record: num_envs must be positive");
    if (num_slots < 1 || num_slots > num_envs) return s_err.fail("dwt_record: num_slots must be in [1, num_envs]");
    if (depth < 1) return s_err.fail("dwt_record: depth must be positive");
    if (hold_mode != DWT_HOLD_NEVER && hold_mode != DWT_HOLD_FALL && hold_mode != DWT_HOLD_RESET) return s_err.fail("dwt_record: unknown hold mode");
    if (!slot_env || !root_states || !dof_state || !contact_forces || !env_state || !rew_buf || !stacked_rewards || !reset_buf || !timeout_buf ||
        !ss || !ring)
        return s_err.fail("dwt_record: a buffer is missing");
    if (!(max_episode_length > 0.0f)) return s_err.fail("dwt_record: max_episode_length must be positive");
    if ((reinterpret_cast<uintptr_t>(ring) & 15u) != 0u) return s_err.fail("dwt_record: ring must be 16-byte aligned");
    hipLaunchKernelGGL(dwt_k_record, dim3((num_slots + SPB - 1) / SPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, (int)num_slots, (int)depth,
                       (int)hold_mode, slot_env, root_states, dof_state, contact_forces, env_state, rew_buf, stacked_rewards, reset_buf, timeout_buf,
                       max_episode_length, (uint32_t *)ss, (float4 *)ring);
    return s_err.launched("dwt_record");
}

int dwt_arm(int32_t num_envs, int32_t num_slots, const int32_t *env_ids, int32_t num_ids, const int64_t *progress_buf,
            const int32_t *env_slot, void *ss, void *stream) {
    if (num_envs < 1) return s_err.fail("dwt_arm: num_envs must be positive");
    if (num_slots < 1 || num_slots > num_envs) return s_err.fail("dwt_arm: num_slots must be in [1, num_envs]");
    if (!progress_buf || !env_slot || !ss) return s_err.fail("dwt_arm: a buffer is missing");
    const int m = s_err.listed("dwt_arm", env_ids, num_ids, num_envs, INT32_MAX);
    if (m <= 0) return m;
    hipLaunchKernelGGL(dwt_k_arm, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)num_envs, (int)num_slots, env_ids, m, progress_buf,
                       env_slot, (uint32_t *)ss);
    return s_err.launched("dwt_arm");
}

int dwt_gather(int32_t num_slots, int32_t depth, const int32_t *slot_ids, int32_t num_ids, const void *ss, const void *ring, void *out,
               int32_t *out_rows, void *stream) {
    if (num_slots < 1) return s_err.fail("dwt_gather: num_slots must be positive");
    if (depth < 1) return s_err.fail("dwt_gather: depth must be positive");
    if (num_ids < 0 || (!slot_ids && num_ids > num_slots)) return s_err.fail("dwt_gather: bad slot id list");
    if (!ss || !ring || !out || !out_rows) return s_err.fail("dwt_gather: a buffer is missing");
    if (((reinterpret_cast<uintptr_t>(ring) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0u) return s_err.fail("dwt_gather: ring and out must be 16-byte aligned");
    if ((int64_t)num_ids * depth > 0x7fffffff - SPB) return s_err.fail("dwt_gather: num_ids * depth is too large");
    if (num_ids == 0) return 0;
    const int rows = num_ids * depth;
    hipLaunchKernelGGL(dwt_k_gather, dim3((rows + SPB - 1) / SPB), dim3(TPB), 0, (hipStream_t)stream, (int)num_slots, (int)depth, slot_ids, (int)num_ids,
                       (const uint32_t *)ss, (const float4 *)ring, (float4 *)out, out_rows);
    return s_err.launched("dwt_gather");
}

}  // extern "C"
