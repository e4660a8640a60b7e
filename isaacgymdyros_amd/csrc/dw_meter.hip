// dw_meter.hip -- the kernels of the learners' episode-return meter (include/dyros_meter.h).  The arithmetic is
// dw_meter.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwm_k_record  one launch per step, one lane per env, DWM_GROUP envs per workgroup.  Every lane advances its env's running episode (all
//                 columns in registers: the loop over DWM_COLS_MAX is unrolled under a uniform guard, no scratch) and clears it if the env
//                 is done.  The C + 1 sums over the finished, finite episodes are reduced by the xor butterfly inside a wavefront (skipped,
//                 with the same +0.0f, by a wavefront that finished none), then ((w0 + w1) + w2) + w3 through LDS; the partial row leaves as
//                 write-through stores of wavefront 0, which drains them before lane 0 draws a ticket with an agent-scope acquire-release
//                 increment.  The workgroup that draws the last ticket reads the partial rows past its L1, adds them in workgroup-index order
//                 (64 rows per pass through LDS, one lane per column), updates ms and sets the ticket back to zero.  No workgroup waits.
//   dwm_k_clear   zeroes ms and the head of work.
#include "dw_group.h"
#include "dw_meter.h"

namespace {

grp::Err s_err;

using dwm::CMAX;
using dwm::GROUP;
using dwm::HEAD;
using dwm::NW;
using dwm::WAVE;
constexpr int CH = 64;                        // partial rows per pass of the finishing workgroup
constexpr int RWMAX = CMAX + 3;

// one object: the wavefronts' sums, the finishing flag and the finishing workgroup's rows
struct Lds {
    float w[NW][CMAX + 1];
    uint32_t cnt[NW][2];
    uint32_t last;
    uint32_t tot[RWMAX];
    uint32_t rows[CH * RWMAX];
};

__device__ __forceinline__ float wave_sum(float t) {
#pragma unroll
    for (int x = WAVE / 2; x >= 1; x >>= 1) t = t + __shfl_xor(t, x, WAVE);
    return t;
}

__device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// words that another workgroup reads or has written in this launch: agent scope, past the L1
__device__ __forceinline__ void put(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t get(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(GROUP) void dwm_k_record(int n, int cols, uint32_t max_size, const float *__restrict__ rew,
                                                      const float *__restrict__ stacked, int stride, const int64_t *__restrict__ done,
                                                      float *__restrict__ cur, uint32_t *ms, uint32_t *work) {
    __shared__ Lds s;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int i = blockIdx.x * GROUP + tid;
    const bool live = i < n;
    const bool dn = live && done[i] != 0;
    // ---- the env's running episode: every column in a register; every load is issued before the first store (the columns of cur are
    //      one pointer to the compiler, so a store between two loads would order them) ----
    float v[CMAX], inc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        v[c] = inc[c] = 0.0f;
        if (c < cols && live) {          // (c < cols is uniform)
            v[c] = cur[(size_t)c * n + i];
            inc[c] = c == 0 ? rew[i] : stacked[(size_t)i * stride + (c - 1)];
        }
    }
    float len = live ? cur[(size_t)cols * n + i] : 0.0f;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {          // (lanes and columns that loaded nothing add 0 to 0)
        v[c] = dwm::bump(v[c], inc[c]);
        fin = fin && dwm::finite(v[c]);
    }
    len = dwm::bump(len, live ? 1.0f : 0.0f);
    // (the stores after all the arithmetic: a block that waits for a loaded value between two stores waits for the first store too)
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < cols && live) cur[(size_t)c * n + i] = dwm::keep(v[c], dn);
    }
    if (live) cur[(size_t)cols * n + i] = dwm::keep(len, dn);
    const bool in_d = dn && fin;
    // ---- the wavefront's sums (a wavefront with no finished episode adds +0.0f throughout: the butterfly's result, without it) ----
    const unsigned long long bd = __ballot(in_d), bx = __ballot(dn && !fin);
    if (bd != 0ull) {          // (wave-uniform)
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < cols) {
                const float t = wave_sum(dwm::term(v[c], in_d));
                if (lane == 0) s.w[w][c] = t;
            }
        }
        const float t = wave_sum(dwm::term(len, in_d));
        if (lane == 0) s.w[w][cols] = t;
    } else if (lane <= cols) {
        s.w[w][lane] = 0.0f;
    }
    if (lane == 0) {
        s.cnt[w][0] = (uint32_t)__popcll(bd);
        s.cnt[w][1] = (uint32_t)__popcll(bx);
    }
    __syncthreads();
    // ---- the partial row: wavefront 0 stores it write-through and drains ----
    const int rw = dwm::row_words(cols);
    uint32_t *rows = work + HEAD;
    if (tid < rw) {
        uint32_t word;
        if (tid <= cols) word = dwm::f2u(dwm::group_sum(s.w[0][tid], s.w[1][tid], s.w[2][tid], s.w[3][tid]));
        else word = s.cnt[0][tid - cols - 1] + s.cnt[1][tid - cols - 1] + s.cnt[2][tid - cols - 1] + s.cnt[3][tid - cols - 1];
        put(rows + (size_t)blockIdx.x * rw + tid, word);
    }
    if (w == 0) {
        drain();
        if (lane == 0) {
            // (the acquire-release increment is the hand-off's fence pair; the row does not lean on it: it was stored write-through and
            //  drained above, and the finishing workgroup reads the rows past its L1)
            const uint32_t ticket = __hip_atomic_fetch_add(work, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s.last = ticket == gridDim.x - 1u ? 1u : 0u;
        }
    }
    __syncthreads();
    if (s.last == 0u) return;          // (uniform over the workgroup)
    // ---- the finishing workgroup: the partial rows in workgroup-index order, one lane per column ----
    const int g = (int)gridDim.x;
    float acc = 0.0f;
    double dacc = 0.0;
    uint32_t cnt = 0u;
    for (int base = 0; base < g; base += CH) {
        const int nr = g - base < CH ? g - base : CH;
        for (int j = tid; j < nr * rw; j += GROUP) s.rows[j] = get(rows + (size_t)base * rw + j);
        __syncthreads();
        if (tid < rw) {
            for (int r = 0; r < nr; ++r) {
                const uint32_t word = s.rows[r * rw + tid];
                if (tid <= cols) {
                    acc = acc + dwm::u2f(word);
                    dacc = dacc + (double)dwm::u2f(word);
                } else {
                    cnt += word;
                }
            }
        }
        __syncthreads();
    }
    if (tid < rw) s.tot[tid] = tid <= cols ? dwm::f2u(acc) : cnt;
    __syncthreads();
    if (tid >= rw) return;
    // (lanes of wavefront 0 from here: every load of ms is issued before any store to it)
    const uint32_t k = s.tot[cols + 1], bad = s.tot[cols + 2];
    const uint32_t current_size = ms[DWM_MS_CURRENT_SIZE];
    unsigned long long *ms64 = reinterpret_cast<unsigned long long *>(ms);
    double *msd = reinterpret_cast<double *>(ms);
    if (k > 0u) {
        if (tid <= cols) {
            float *mean = reinterpret_cast<float *>(ms) + (tid < cols ? DWM_MS_MEAN + tid : DWM_MS_MEAN_LEN);
            *mean = dwm::window_mean(*mean, acc, k, max_size, current_size);
        }
        if (tid == 0) {
            msd[DWM_MS_SUM_RET / 2] = msd[DWM_MS_SUM_RET / 2] + dacc;
            ms64[DWM_MS_GAMES / 2] += (unsigned long long)k;
        }
        if (tid == cols) msd[DWM_MS_SUM_LEN / 2] = msd[DWM_MS_SUM_LEN / 2] + dacc;
        if (tid == cols + 1) ms[DWM_MS_CURRENT_SIZE] = dwm::window_old(k, max_size, current_size) + dwm::window_new(k, max_size);
    }
    if (tid == cols + 2) {
        if (bad > 0u) ms64[DWM_MS_DISCARDED / 2] += (unsigned long long)bad;
        put(work, 0u);          // the ticket: the next launch, or a graph replay, starts clean
    }
}

__global__ __launch_bounds__(WAVE) void dwm_k_clear(uint32_t *ms, uint32_t *work) {
    const int t = threadIdx.x;
    if (t < DWM_MS_WORDS) ms[t] = 0u;
    if (t < HEAD) work[t] = 0u;
}

#define DWM_STR_(x) #x
#define DWM_STR(x) DWM_STR_(x)
int check_shape(const char *who, int32_t num_envs, int32_t cols) {
    if (s_err.envs(who, num_envs, GROUP) != 0) return -1;
    return cols >= 1 && cols <= DWM_COLS_MAX ? 0 : s_err.fail(who, "cols must be in [1, " DWM_STR(DWM_COLS_MAX) "]");
}

}  // namespace

extern "C" {

int dwm_abi_version(void) { return DWM_ABI_VERSION; }
const char *dwm_last_error(void) { return s_err.s; }

int64_t dwm_work_words(int32_t num_envs, int32_t cols) {
    if (check_shape("dwm_work_words", num_envs, cols) != 0) return -1;
    return dwm::work_words(num_envs, cols);
}

int dwm_record(int32_t num_envs, int32_t cols, int32_t max_size, const float *rew, const float *stacked, int32_t stacked_stride,
               const int64_t *done, float *cur, void *ms, void *work, void *stream) {
    if (check_shape("dwm_record", num_envs, cols) != 0) return -1;
    if (max_size < 1) return s_err.fail("dwm_record: max_size must be positive");
    if (!rew || !done || !cur || !ms || !work) return s_err.fail("dwm_record: a buffer is missing");
    if (cols > 1 && !stacked) return s_err.fail("dwm_record: cols > 1 needs the stacked reward terms");
    if (cols > 1 && stacked_stride < cols - 1) return s_err.fail("dwm_record: stacked_stride must be at least cols - 1");
    if ((reinterpret_cast<uintptr_t>(ms) & 7u) != 0u) return s_err.fail("dwm_record: ms must be 8-byte aligned");
    hipLaunchKernelGGL(dwm_k_record, dim3(dwm::groups(num_envs)), dim3(GROUP), 0, (hipStream_t)stream, (int)num_envs, (int)cols, (uint32_t)max_size,
                       rew, stacked, (int)stacked_stride, done, cur, (uint32_t *)ms, (uint32_t *)work);
    return s_err.launched("dwm_record");
}

int dwm_clear(void *ms, void *work, void *stream) {
    if (!ms || !work) return s_err.fail("dwm_clear: a buffer is missing");
    hipLaunchKernelGGL(dwm_k_clear, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, (uint32_t *)ms, (uint32_t *)work);
    return s_err.launched("dwm_clear");
}

}  // extern "C"
