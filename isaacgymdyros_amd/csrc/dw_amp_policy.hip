// dw_amp_policy.hip -- the actor-critic of the consumer's side of TocabiAMPLower (include/dyros_amp_policy.h; reference:
// learning/amp_continuous.py:91-167, 260-329, learning/common_agent.py:413-511, cfg/train/TocabiAMPLowerPPO.yaml).  gfx950, fp32 throughout;
// the products of both 512-512 MLPs on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32: one rounding per product, no downcast).
//
// One product kernel, dwa_mm<TA, TB>, serves every layer: C = op(A) op(B) over a 128 x 128 tile, 32-deep k slices through LDS, four waves of
// 64 x 64 (4 x 4 MFMA tiles of 16 x 16), two problems per launch (actor and critic: blockIdx.z), split over K into slabs that dwa_slab_sum
// adds in slab order (no float atomics anywhere, so a replayed graph gives the bits of the eager launches).
//
// The backward pass in products (per net; B rows, Z = pre-activation gradients, [.|1] = a column of ones appended for the bias):
//   heads   dZ2 = relu'(h2) * (dmu muW)  (actor) / relu'(h2) * dv w  (critic)     -- per row, vector unit (dwa_heads_bwd)
//           [dmuW | dmub] = dmu^T [h2a | 1],  [dw | db] = dv^T [h2c | 1]          -- dwa_mm<1, 0>, K = B
//   layer 2 [dW2 | db2] = dZ2^T [h1 | 1]                                          -- dwa_mm<1, 0>, K = B
//           dZ1 = relu'(h1) * (dZ2 W2)                                            -- dwa_mm<0, 0>, K = 512, written over h1
//   layer 1 [dW1 | db1] = dZ1^T [x | 1]                                           -- dwa_mm<1, 0>, K = B
// No input gradient is formed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/dyros_amp_policy.h"

// Built with -ffp-contract=off (build.py): no product and sum are fused into one fma unless written as fmaf, so GAE, the sampled action
// and the unnormalised value repeat torch's separately rounded operations (HIP's default contraction ignores `#pragma clang fp contract`).

namespace {

char g_err[256] = "";
int fail_hip(const char *who, hipError_t e) { snprintf(g_err, sizeof(g_err), "%s: %s", who, hipGetErrorString(e)); return -1; }
int fail(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return -1; }
int done(const char *who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(who, e);
}

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int HID = DWA_HID;
constexpr int HL = HID + 4;          // row length of the hidden-layer buffers: column HID holds the ones of the bias gradients
constexpr int DL = 32;               // row length of the head-gradient rows: dmu in columns 0 .. A - 1, dv in column 16
constexpr float NORM_EPS = 1e-5f, NORM_CLIP = 5.0f;

// offsets into the parameter layout
struct Off {
    size_t w1[2], b1[2], w2[2], b2[2], hw[2], hb[2];
};
__host__ __device__ inline Off offsets(int D, int A) {
    Off o;
    const size_t net = (size_t)D * HID + HID + (size_t)HID * HID + HID;
    for (int n = 0; n < 2; ++n) {
        const size_t base = n ? net + (size_t)A * HID + A : 0;
        o.w1[n] = base;
        o.b1[n] = base + (size_t)D * HID;
        o.w2[n] = o.b1[n] + HID;
        o.b2[n] = o.w2[n] + (size_t)HID * HID;
        o.hw[n] = o.b2[n] + HID;
        o.hb[n] = o.hw[n] + (size_t)(n ? 1 : A) * HID;
    }
    return o;
}

__device__ __forceinline__ float wave_sum(float x) {
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);          // (every lane ends with the same bits: each step adds a pair both ways)
    return x;
}

// ------------------------------------------------------------------------------------------------------------------------- products
// Operand staging: an operand whose k index is contiguous in memory (A with TA = 0, B with TB = 1) sits in LDS as [row][k] with rows of
// SKM floats, the other one as [k][row] with rows of SMK floats; both strides make a wave's MFMA operand reads (16 rows x 4 k) conflict-free.
constexpr int TM = 128, TN = 128, TK = 32, SKM = TK + 4, SMK = TM + 16;
static_assert(TM * SKM == TK * SMK, "one LDS size for both stagings");
enum { E_STORE = 0, E_BIAS_RELU = 1, E_MASK = 2 };
struct MmOp {
    const float *A, *B, *bias;
    float *C;
    int M;
};
struct Mm {
    MmOp op[2];
    int N, K, lda, ldb, ldc, kc, nz, mode;
    long long zstride;          // floats between the slabs of one problem (E_STORE)
};

template <int KC>          // KC = 1: k contiguous in memory
__device__ __forceinline__ void stage_load(const float *__restrict__ X, int ld, int r0, int rlim, int kb, int k1, float (&reg)[16], int t) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = t + 256 * q;
        const int r = KC ? e >> 5 : e & 127, k = KC ? e & 31 : e >> 7;
        const int gr = r0 + r, gk = kb + k;
        reg[q] = (gr < rlim && gk < k1) ? X[KC ? (size_t)gr * ld + gk : (size_t)gk * ld + gr] : 0.0f;
    }
}
template <int KC>
__device__ __forceinline__ void stage_store(float *__restrict__ S, const float (&reg)[16], int t) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = t + 256 * q;
        if (KC) S[(e >> 5) * SKM + (e & 31)] = reg[q];
        else S[(e >> 7) * SMK + (e & 127)] = reg[q];
    }
}

template <int TA, int TB>
__global__ __launch_bounds__(256) void dwa_mm(const Mm G) {
    __shared__ float As[TM * SKM];
    __shared__ float Bs[TN * SKM];
    const int pr = blockIdx.z / G.nz, z = blockIdx.z - pr * G.nz;
    const MmOp op = G.op[pr];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, lk = lane >> 4;
    const int n0 = blockIdx.x * TN, m0 = blockIdx.y * TM, wm = (w >> 1) * 64, wn = (w & 1) * 64;
    if (m0 >= op.M) return;          // (the smaller problem of a launch)
    const int k0 = z * G.kc, k1 = min(G.K, k0 + G.kc);
    const int live = min(4, (op.M - m0 - wm + 15) / 16);          // MFMA row tiles of this wave holding live rows (wave-uniform)
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    float ra[16], rb[16];
    if (k0 < k1) {
        stage_load<1 - TA>(op.A, G.lda, m0, op.M, k0, k1, ra, t);
        stage_load<TB>(op.B, G.ldb, n0, G.N, k0, k1, rb, t);
    }
    for (int kb = k0; kb < k1; kb += TK) {
        __syncthreads();          // (the previous slice is consumed)
        stage_store<1 - TA>(As, ra, t);
        stage_store<TB>(Bs, rb, t);
        __syncthreads();
        if (kb + TK < k1) {          // (the next slice's loads fly while this one is multiplied)
            stage_load<1 - TA>(op.A, G.lda, m0, op.M, kb + TK, k1, ra, t);
            stage_load<TB>(op.B, G.ldb, n0, G.N, kb + TK, k1, rb, t);
        }
#pragma unroll
        for (int kk = 0; kk < TK / 4; ++kk) {
            const int k = 4 * kk + lk;
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = TA ? As[k * SMK + wm + 16 * i + li] : As[(wm + 16 * i + li) * SKM + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = TB ? Bs[(wn + 16 * j + li) * SKM + k] : Bs[k * SMK + wn + 16 * j + li];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < live)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D of v_mfma_f32_16x16x4_f32: register r of lane l holds row 4 (l >> 4) + r, column l & 15 of the 16 x 16 tile
    float *C = op.C + (G.mode == E_STORE ? (size_t)z * G.zstride : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn + 16 * j + li;
            if (col >= G.N) continue;
            const float bj = G.mode == E_BIAS_RELU ? op.bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + 16 * i + 4 * lk + r;
                if (row >= op.M) continue;
                float *c = C + (size_t)row * G.ldc + col;
                if (G.mode == E_BIAS_RELU) *c = fmaxf(acc[i][j][r] + bj, 0.0f);
                else if (G.mode == E_MASK) *c = *c > 0.0f ? acc[i][j][r] : 0.0f;          // (relu's backward: threshold_backward)
                else *c = acc[i][j][r];
            }
        }
}

// g[W] += sum of the slabs (in slab order) of [M][N] products whose last column is the bias gradient
struct SlabSum {
    const float *slab;
    float *gw[2], *gb[2];
    int M[2], N, nz;
    long long zstride;
};
__global__ __launch_bounds__(256) void dwa_slab_sum(const SlabSum S) {
    const int pr = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.M[pr] * S.N) return;
    const int m = e / S.N, n = e - m * S.N;
    const float *x = S.slab + (size_t)pr * S.nz * S.zstride + e;
    float s = 0.0f;
    for (int z = 0; z < S.nz; ++z) s += x[(size_t)z * S.zstride];
    if (n < S.N - 1) S.gw[pr][(size_t)m * (S.N - 1) + n] += s;
    else S.gb[pr][m] += s;
}

// ------------------------------------------------------------------------------------------------------------------------- rows
// rl_games' RunningMeanStd normalisation: (x - mean) / sqrt(var + 1e-5) with the fp64 statistics cast to fp32 first, clamped to +-5.  Row r
// of xn: the D normalised words, a 1 (the bias column of dW1), zeros to XL.  `ones`: the bias columns of the hidden-layer buffers too.
__global__ __launch_bounds__(256) void dwa_norm_rows(const float *__restrict__ x, const double *__restrict__ st, int R, int D, int XL,
                                                     float *__restrict__ xn, float *__restrict__ h1, float *__restrict__ h2, int ones) {
    const size_t n = (size_t)R * XL;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / XL), k = (int)(e - (size_t)r * XL);
        float y = 0.0f;
        if (k < D) {
            const float mu = (float)st[k], var = (float)st[D + k];
            y = fminf(fmaxf((x[(size_t)r * D + k] - mu) / sqrtf(var + NORM_EPS), -NORM_CLIP), NORM_CLIP);
        } else if (k == D) {
            y = 1.0f;
        }
        xn[e] = y;
        if (ones && k == 0)
            for (int net = 0; net < 2; ++net) {
                h1[((size_t)net * R + r) * HL + HID] = 1.0f;
                h2[((size_t)net * R + r) * HL + HID] = 1.0f;
            }
    }
}

// The heads of one row, one wave: lane l holds h[i] = h2[l + 64 i]; mu [A] and v come back in every lane.
__device__ __forceinline__ void heads(const float *__restrict__ p, const Off &o, int A, const float (&ha)[8], const float (&hc)[8], int lane,
                                      float (&mu)[DWA_A_MAX], float &v, int actor) {
    if (actor) {
        const float *mw = p + o.hw[0];
#pragma unroll
        for (int a = 0; a < DWA_A_MAX; ++a) {
            mu[a] = 0.0f;
            if (a < A) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < 8; ++i) s = fmaf(ha[i], mw[(size_t)a * HID + lane + 64 * i], s);
                mu[a] = wave_sum(s) + p[o.hb[0] + a];
            }
        }
    }
    const float *vw = p + o.hw[1];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(hc[i], vw[lane + 64 * i], s);
    v = wave_sum(s) + p[o.hb[1]];
}

// ActorCritic.unnorm_value: v * sqrt(var.float() + eps) + mean.float(), unfused
__device__ __forceinline__ float unnorm(float v, const double *__restrict__ vs) {
    return __fadd_rn(__fmul_rn(v, sqrtf(__fadd_rn((float)vs[1], NORM_EPS))), (float)vs[0]);
}

constexpr int RW = 4;          // rows (waves) per workgroup of the row kernels
__global__ __launch_bounds__(64 * RW) void dwa_act_out(const float *__restrict__ p, const double *__restrict__ vs, const float *__restrict__ logstd,
                                                       const float *__restrict__ noise, const float *__restrict__ h2, int N, int D, int A,
                                                       float *__restrict__ action, float *__restrict__ clamped, float *__restrict__ mu_out,
                                                       float *__restrict__ nlp_out, float *__restrict__ value) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * RW + (threadIdx.x >> 6);
    if (r >= N) return;
    const Off o = offsets(D, A);
    float ha[8], hc[8], mu[DWA_A_MAX], v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ha[i] = h2[(size_t)r * HL + lane + 64 * i];
        hc[i] = h2[((size_t)N + r) * HL + lane + 64 * i];
    }
    heads(p, o, A, ha, hc, lane, mu, v, 1);
    if (lane != 0) return;
    // neglogp as ActorCritic.neglogp: 0.5 sum(((a - mu) / exp(s))^2) + 0.5 log(2 pi) A + sum(s)
    float sq = 0.0f, ss = 0.0f;
#pragma unroll
    for (int a = 0; a < DWA_A_MAX; ++a) {
        if (a < A) {
            const float sd = expf(logstd[a]);
            const float act = __fadd_rn(mu[a], __fmul_rn(sd, noise[(size_t)r * A + a]));
            const float zz = (act - mu[a]) / sd;
            sq = __fadd_rn(sq, __fmul_rn(zz, zz));
            ss += logstd[a];
            action[(size_t)r * A + a] = act;
            clamped[(size_t)r * A + a] = fminf(fmaxf(act, -1.0f), 1.0f);
            mu_out[(size_t)r * A + a] = mu[a];
        }
    }
    nlp_out[r] = __fadd_rn(__fadd_rn(0.5f * sq, (float)(0.9189385332046727 * A)), ss);
    value[r] = unnorm(v, vs);
}

__global__ __launch_bounds__(64 * RW) void dwa_critic_out(const float *__restrict__ p, const double *__restrict__ vs, const float *__restrict__ term,
                                                          const float *__restrict__ h2, int N, int D, int A, float *__restrict__ value) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * RW + (threadIdx.x >> 6);
    if (r >= N) return;
    const Off o = offsets(D, A);
    float ha[8], hc[8], mu[DWA_A_MAX], v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ha[i] = 0.0f;
        hc[i] = h2[(size_t)r * HL + lane + 64 * i];
    }
    heads(p, o, A, ha, hc, lane, mu, v, 0);
    if (lane == 0) value[r] = __fmul_rn(unnorm(v, vs), 1.0f - term[r]);
}

// The losses of calc_gradients for one row per wave, their gradients with respect to mu and v (into dd: dmu in columns 0 .. A - 1, dv in
// column 16), dZ2 of both nets (into z2), and the rows' loss sums per workgroup (part[block][4], waves summed in order).
struct Heads {
    const float *p, *logstd, *act, *old_nlp, *adv, *ret, *h2;
    float *dd, *z2, *part;
    int B, D, A;
    DwaLoss c;
};
constexpr int HEAD_BLOCKS = 2048;
__global__ __launch_bounds__(64 * RW) void dwa_heads_bwd(const Heads H) {
    __shared__ float red[RW][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, B = H.B, A = H.A;
    const Off o = offsets(H.D, A);
    const float invB = 1.0f / (float)B, e = H.c.e_clip, lo = (float)(1.0 - (double)e), hi = (float)(1.0 + (double)e);
    const float nlp_c = (float)(0.9189385332046727 * A);
    const float *mw = H.p + o.hw[0], *vw = H.p + o.hw[1];
    float la = 0.0f, lc = 0.0f, lb = 0.0f, lf = 0.0f;
    for (int r = blockIdx.x * RW + w; r < B; r += gridDim.x * RW) {
        float ha[8], hc[8], mu[DWA_A_MAX], v;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ha[i] = H.h2[(size_t)r * HL + lane + 64 * i];
            hc[i] = H.h2[((size_t)B + r) * HL + lane + 64 * i];
        }
        heads(H.p, o, A, ha, hc, lane, mu, v, 1);
        float sq = 0.0f, ss = 0.0f, zs[DWA_A_MAX];
#pragma unroll
        for (int a = 0; a < DWA_A_MAX; ++a) {
            zs[a] = 0.0f;
            if (a < A) {
                zs[a] = (H.act[(size_t)r * A + a] - mu[a]) / expf(H.logstd[a]);
                sq = __fadd_rn(sq, __fmul_rn(zs[a], zs[a]));
                ss += H.logstd[a];
            }
        }
        const float nlp = __fadd_rn(__fadd_rn(0.5f * sq, nlp_c), ss);
        const float ratio = expf(H.old_nlp[r] - nlp), adv = H.adv[r];
        const float x1 = __fmul_rn(-adv, ratio), x2 = __fmul_rn(-adv, fminf(fmaxf(ratio, lo), hi));
        // torch.max splits the gradient of equal arguments in halves; clamp passes it inside [lo, hi] inclusive
        const float g1 = x1 > x2 ? 1.0f : (x1 == x2 ? 0.5f : 0.0f), in = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;
        const float dratio = (g1 * -adv + (1.0f - g1) * in * -adv) * invB;
        const float dnlp = -ratio * dratio, ret = H.ret[r];
        const float dv = H.c.critic_coef * invB * 2.0f * (v - ret);
        float dmu[DWA_A_MAX], bl = 0.0f;
#pragma unroll
        for (int a = 0; a < DWA_A_MAX; ++a) {
            dmu[a] = 0.0f;
            if (a < A) {
                const float hi1 = fmaxf(mu[a] - 1.0f, 0.0f), lo1 = fminf(mu[a] + 1.0f, 0.0f);
                bl += hi1 * hi1 + lo1 * lo1;
                dmu[a] = dnlp * (-zs[a] / expf(H.logstd[a])) + H.c.bounds_coef * invB * 2.0f * (hi1 + lo1);
            }
        }
        la += fmaxf(x1, x2);
        lc += (ret - v) * (ret - v);
        lb += bl;
        lf += fabsf(ratio - 1.0f) > e ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = lane + 64 * i;
            float s = 0.0f;
#pragma unroll
            for (int a = 0; a < DWA_A_MAX; ++a)
                if (a < A) s = fmaf(dmu[a], mw[(size_t)a * HID + j], s);
            H.z2[(size_t)r * HL + j] = ha[i] > 0.0f ? s : 0.0f;
            H.z2[((size_t)B + r) * HL + j] = hc[i] > 0.0f ? dv * vw[j] : 0.0f;
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < DWA_A_MAX; ++a)
                if (a < A) H.dd[(size_t)r * DL + a] = dmu[a];
            H.dd[(size_t)r * DL + 16] = dv;
        }
    }
    if (lane == 0) { red[w][0] = la; red[w][1] = lc; red[w][2] = lb; red[w][3] = lf; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float s = 0.0f;
        for (int q = 0; q < RW; ++q) s += red[q][threadIdx.x];
        H.part[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
    }
}
__global__ __launch_bounds__(64) void dwa_log_sum(const float *__restrict__ part, int nb, int B, float *__restrict__ state) {
    if (threadIdx.x < 4) {
        float s = 0.0f;
        for (int b = 0; b < nb; ++b) s += part[(size_t)b * 4 + threadIdx.x];
        state[DWA_S_A_LOSS + threadIdx.x] += s / (float)B;
    }
    if (threadIdx.x == 0) state[DWA_S_UPDATES] += 1.0f;
}

// ------------------------------------------------------------------------------------------------------------------------- statistics
constexpr int STAT_PARTS = 1024;
__global__ __launch_bounds__(256) void dwa_stats_part(const float *__restrict__ x, int B, int D, double *__restrict__ part) {
    const int b = blockIdx.x, lo = (int)((long)B * b / STAT_PARTS), hi = (int)((long)B * (b + 1) / STAT_PARTS);
    for (int c = threadIdx.x; c < D; c += 256) {
        double s = 0.0, q = 0.0;
        for (int r = lo; r < hi; ++r) {
            const double v = x[(size_t)r * D + c];
            s += v;
            q += v * v;
        }
        part[(size_t)b * 2 * D + c] = s;
        part[(size_t)b * 2 * D + D + c] = q;
    }
}
__global__ __launch_bounds__(256) void dwa_stats_fin(const double *__restrict__ part, int B, int D, const double *__restrict__ in,
                                                     double *__restrict__ out) {
    const double n = (double)B, count = in[2 * D], tot = count + n;
    for (int c = threadIdx.x; c < D; c += 256) {
        double s = 0.0, q = 0.0;
        for (int b = 0; b < STAT_PARTS; ++b) { s += part[(size_t)b * 2 * D + c]; q += part[(size_t)b * 2 * D + D + c]; }
        const double bm = s / n, bv = fmax(q - s * bm, 0.0) / (n - 1.0);          // unbiased, as torch.var
        const double mean = in[c], var = in[D + c], delta = bm - mean;
        out[c] = mean + delta * n / tot;
        out[D + c] = (var * count + bv * n + delta * delta * count * n / tot) / tot;
    }
    __syncthreads();          // (every thread has read in[2 D] before out may alias it)
    if (threadIdx.x == 0) out[2 * D] = tot;
}

// ------------------------------------------------------------------------------------------------------------------------- Adam
// torch.optim.Adam (foreach form): m.lerp_(g, 1 - b1); v = v * b2 + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void dwa_opt_step(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                                    const float *__restrict__ state, int NP) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NP) return;
    const double step = (double)state[DWA_S_STEP] + 1.0;
    const float step_size = (float)((double)state[DWA_S_LR] / (1.0 - pow(0.9, step)));
    const float bc2s = (float)sqrt(1.0 - pow(0.999, step));
    const float gi = g[i];
    const float mi = m[i] + 0.1f * (gi - m[i]);
    const float vi = v[i] * 0.999f + (float)(1.0 - 0.999) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= step_size * (mi / (sqrtf(vi) / bc2s + 1e-8f));
    g[i] = 0.0f;
}
__global__ void dwa_opt_tick(float *__restrict__ state) { state[DWA_S_STEP] += 1.0f; }

// ------------------------------------------------------------------------------------------------------------------------- GAE
// discount_values: delta = r + gamma next - v; last = delta + (gamma tau) (1 - done) last; each operation rounded on its own, as torch does it
__global__ __launch_bounds__(256) void dwa_gae_scan(const float *__restrict__ done, const float *__restrict__ val, const float *__restrict__ rew,
                                                    const float *__restrict__ nxt, int H, int N, float gamma, float gt, float *__restrict__ adv,
                                                    float *__restrict__ ret) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float last = 0.0f;
    for (int t = H - 1; t >= 0; --t) {
        const size_t i = (size_t)t * N + n;
        const float nd = __fsub_rn(1.0f, done[i]);
        const float delta = __fsub_rn(__fadd_rn(rew[i], __fmul_rn(gamma, nxt[i])), val[i]);
        last = __fadd_rn(delta, __fmul_rn(__fmul_rn(gt, nd), last));
        adv[i] = last;
        ret[i] = __fadd_rn(last, val[i]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------- play
// dwa_play: the actor alone, eval mode.  Every product is v_mfma_f32_16x16x4_f32 on one 16-row tile; the k index of a
// 16-deep block is permuted so that lane (li, lk) feeds k = 4 lk + kk to the kk-th MFMA of the block: its A and W words are then four
// consecutive floats (one ds_read_b128 / global_load_dwordx4 each), and W's rows are read in 64-byte pieces.  Two forms:
//   N > PLAY_SMALL_N  dwa_play_rows: one launch of 16-row workgroups; the normalised rows and both hidden layers stay in LDS (2 x 16 x 516
//                     floats, two workgroups per CU), each wave makes 128 of the 512 columns of a layer, the actor's weights stream from L2
//   N <= PLAY_SMALL_N dwa_play_cols (x 2) and dwa_play_head: a 16-column slice of a layer per workgroup (32 workgroups share the weights
//                     instead of each reading all 2 MB), its four waves split K, the quarters added in wave order; h1 and h2 go through the
//                     workspace
// Both end in play_out: the mu head as one 16 x 16 tile whose K the four waves split, added in wave order, then the bias, the optional noise
// and the clamp.  No atomics: a replay gives the bits of the eager call.
constexpr int PR = 16;                  // rows per workgroup of dwa_play_rows / dwa_play_head
constexpr int PS = HID + 4;             // LDS row length (floats) of their row images: >= any D rounded up to 16
constexpr int PLAY_SMALL_N = 64;        // the largest N of the column-split form (four row tiles per wave)
static_assert(DWA_D_MAX <= HID, "the input rows share the hidden-layer row images");

struct Play {
    const float *p, *logstd, *obs, *noise;
    const double *st;
    float *clamped, *mu, *h1, *h2;
    int N, D, A, pal, oal;              // pal / oal: p / obs 16-byte aligned (and D a multiple of 4) -- the vector loads are allowed
};

// four consecutive floats of a row from k; zeros from kmax on (vec: the row is 16-byte aligned wherever k is)
__device__ __forceinline__ f4 ld4(const float *__restrict__ row, int k, int kmax, int vec) {
    if (vec && k + 4 <= kmax) return *(const f4 *)(row + k);
    f4 x;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = k + q < kmax ? row[k + q] : 0.0f;
    return x;
}

// acc[j] += A [16 rows of lda floats, LDS] x W[c0 + 16 j + li][k]^T over k < kpad (a multiple of 16), W read as zero from K or column ncol on
template <int NT>
__device__ __forceinline__ void play_mm(const float *As, int lda, const float *__restrict__ W, int ldw, int K, int kpad, int c0, int ncol, int lane,
                                        int vec, f4 (&acc)[NT]) {
    const int li = lane & 15, lk = lane >> 4;
    f4 b[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = c0 + 16 * j + li;
        b[j] = c < ncol ? ld4(W + (size_t)c * ldw, 4 * lk, K, vec) : (f4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    for (int kb = 0; kb < kpad; kb += 16) {
        f4 bn[NT];
        if (kb + 16 < kpad) {          // (the next block's weights fly while this one is multiplied)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int c = c0 + 16 * j + li;
                bn[j] = c < ncol ? ld4(W + (size_t)c * ldw, kb + 16 + 4 * lk, K, vec) : (f4){0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        const f4 a = *(const f4 *)(As + li * lda + kb + 4 * lk);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[j][kk], acc[j], 0, 0, 0);
        if (kb + 16 < kpad) {
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = bn[j];
        }
    }
}

// one hidden layer of 16 rows in LDS: Y = relu(X W^T + b), wave w making the columns 128 w .. 128 w + 127
__device__ __forceinline__ void play_layer(const float *X, const float *__restrict__ W, const float *__restrict__ bias, int K, int vec, float *Y,
                                           int w, int lane) {
    f4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    play_mm<8>(X, PS, W, K, K, (K + 15) / 16 * 16, 128 * w, HID, lane, vec, acc);
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = 128 * w + 16 * j + li;
        const float bj = bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) Y[(4 * lk + r) * PS + col] = fmaxf(acc[j][r] + bj, 0.0f);
    }
}

// the mu head of the 16 rows whose h2 is in X (LDS), then noise and clamp; R: 4 x 256 floats of LDS for the waves' partial tiles
__device__ __forceinline__ void play_out(const Play &P, const float *X, float *R, int row0, int w, int lane) {
    const Off o = offsets(P.D, P.A);
    f4 acc[1] = {(f4){0.0f, 0.0f, 0.0f, 0.0f}};
    play_mm<1>(X + 128 * w, PS, P.p + o.hw[0] + 128 * w, HID, 128, 128, 0, P.A, lane, P.pal, acc);
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) R[w * 256 + (4 * lk + r) * 16 + li] = acc[0][r];
    __syncthreads();
    const int t = threadIdx.x, r = t >> 4, a = t & 15, row = row0 + r;
    if (row >= P.N || a >= P.A) return;
    const float m = ((R[t] + R[256 + t]) + R[512 + t]) + R[768 + t] + P.p[o.hb[0] + a];
    float act = m;
    if (P.noise) act = __fadd_rn(m, __fmul_rn(expf(P.logstd[a]), P.noise[(size_t)row * P.A + a]));
    P.clamped[(size_t)row * P.A + a] = fminf(fmaxf(act, -1.0f), 1.0f);
    if (P.mu) P.mu[(size_t)row * P.A + a] = m;
}

// RunningMeanStd.forward in eval mode, as dwa_norm_rows
__device__ __forceinline__ float play_norm(float x, const double *__restrict__ st, int D, int k) {
    return fminf(fmaxf((x - (float)st[k]) / sqrtf((float)st[D + k] + NORM_EPS), -NORM_CLIP), NORM_CLIP);
}

__global__ __launch_bounds__(256) void dwa_play_rows(const Play P) {
    __shared__ float X[PR * PS];          // the normalised rows, then h2
    __shared__ float Y[PR * PS];          // h1, then the head's partial tiles
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, row0 = blockIdx.x * PR, D = P.D, dpad = (D + 15) / 16 * 16;
    const Off o = offsets(D, P.A);
    for (int e = t; e < PR * dpad; e += 256) {
        const int r = e / dpad, k = e - r * dpad, row = row0 + r;
        X[r * PS + k] = (row < P.N && k < D) ? play_norm(P.obs[(size_t)row * D + k], P.st, D, k) : 0.0f;
    }
    __syncthreads();
    play_layer(X, P.p + o.w1[0], P.p + o.b1[0], D, P.pal && !(D & 3), Y, w, lane);
    __syncthreads();
    play_layer(Y, P.p + o.w2[0], P.p + o.b2[0], HID, P.pal, X, w, lane);
    __syncthreads();
    play_out(P, X, Y, row0, w, lane);
}

// one layer for N <= PLAY_SMALL_N rows: out[r][c0 .. c0 + 15] = relu(A[r] W^T + b) for the 16-column slice c0 = 16 blockIdx.x; the four
// waves take a quarter of K's 16-deep blocks each.  NORM: A is the observation rows, normalised here (layer 1); else h1 (layer 2).
template <int NORM>
__global__ __launch_bounds__(256) void dwa_play_cols(const Play P) {
    __shared__ float R[4][PLAY_SMALL_N * 16];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, li = lane & 15, lk = lane >> 4, c0 = 16 * blockIdx.x, N = P.N;
    const Off o = offsets(P.D, P.A);
    const int K = NORM ? P.D : HID, nblk = (K + 15) / 16, kb0 = 16 * (nblk * w / 4), kb1 = 16 * (nblk * (w + 1) / 4);
    const float *W = P.p + (NORM ? o.w1[0] : o.w2[0]), *bias = P.p + (NORM ? o.b1[0] : o.b2[0]);
    const float *A = NORM ? P.obs : P.h1;
    const int wvec = P.pal && (NORM ? !(K & 3) : 1), avec = NORM ? P.oal : 1;
    const int rt = (N + 15) / 16;
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int kb = kb0; kb < kb1; kb += 16) {
        const int k = kb + 4 * lk;
        const f4 b = ld4(W + (size_t)(c0 + li) * K, k, K, wvec);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < rt) {          // (wave-uniform)
                const int row = 16 * i + li;
                f4 a = (f4){0.0f, 0.0f, 0.0f, 0.0f};
                if (row < N) {
                    a = ld4(A + (size_t)row * K, k, K, avec);
                    if (NORM) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) a[q] = k + q < K ? play_norm(a[q], P.st, K, k + q) : 0.0f;
                    }
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc[i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) R[w][(16 * i + 4 * lk + r) * 16 + li] = acc[i][r];
    __syncthreads();
    float *out = NORM ? P.h1 : P.h2;
    for (int e = t; e < N * 16; e += 256) {
        const int r = e >> 4, c = e & 15;
        out[(size_t)r * HID + c0 + c] = fmaxf(((R[0][e] + R[1][e]) + R[2][e]) + R[3][e] + bias[c0 + c], 0.0f);
    }
}

// the head for N <= PLAY_SMALL_N rows: h2 from the workspace into LDS, then play_out (one workgroup per 16 rows)
__global__ __launch_bounds__(256) void dwa_play_head(const Play P) {
    __shared__ float X[PR * PS];
    __shared__ float R[4 * 256];
    const int t = threadIdx.x, row0 = blockIdx.x * PR;
    for (int e = t; e < PR * HID; e += 256) {
        const int r = e / HID, k = e - r * HID;
        X[r * PS + k] = row0 + r < P.N ? P.h2[(size_t)(row0 + r) * HID + k] : 0.0f;
    }
    __syncthreads();
    play_out(P, X, R, row0, t >> 6, t & 63);
}

// ------------------------------------------------------------------------------------------------------------------------- host side
int check_da(int D, int A) { return D >= 1 && D <= DWA_D_MAX && A >= 1 && A <= DWA_A_MAX; }
int xl_of(int D) { return (D + 1 + 3) / 4 * 4; }
int slabs_of(int B) { return B <= 4096 ? 1 : (B + 4095) / 4096 > 16 ? 16 : (B + 4095) / 4096; }

struct Work {          // float offsets into the workspace
    size_t xn, h1, h2, z2, dd, part, slab, end;
};
Work layout(int R, int D, int grad) {
    Work w;
    const auto up = [](size_t x) { return (x + 63) / 64 * 64; };
    w.xn = 0;
    w.h1 = up(w.xn + (size_t)R * xl_of(D));
    w.h2 = up(w.h1 + (size_t)2 * R * HL);
    w.z2 = w.dd = w.part = w.slab = w.end = up(w.h2 + (size_t)2 * R * HL);
    if (grad) {
        w.dd = up(w.z2 + (size_t)2 * R * HL);
        w.part = up(w.dd + (size_t)R * DL);
        w.slab = up(w.part + (size_t)HEAD_BLOCKS * 4);
        w.end = up(w.slab + (size_t)2 * slabs_of(R) * HID * (HID + 1));
    }
    return w;
}

int mm(hipStream_t s, int ta, int tb, const Mm &G, int nprob, int maxM) {
    const dim3 grid((G.N + TN - 1) / TN, (maxM + TM - 1) / TM, nprob * G.nz);
    if (ta == 0 && tb == 1) hipLaunchKernelGGL((dwa_mm<0, 1>), grid, dim3(256), 0, s, G);
    else if (ta == 1 && tb == 0) hipLaunchKernelGGL((dwa_mm<1, 0>), grid, dim3(256), 0, s, G);
    else if (ta == 0 && tb == 0) hipLaunchKernelGGL((dwa_mm<0, 0>), grid, dim3(256), 0, s, G);
    else return fail("dwa_mm: no such operand form");
    return done("dwa_mm");
}

// normalisation and both hidden layers of net n0 .. n0 + nn - 1 over R rows into the workspace (h2 of net n at W + w.h2 + n R HL)
int forward(hipStream_t s, const float *p, const double *st, const float *x, int R, int D, int A, int n0, int nn, float *W, const Work &w, int ones) {
    const Off o = offsets(D, A);
    const int XL = xl_of(D);
    const size_t ne = (size_t)R * XL;
    const int nb = (int)((ne + 255) / 256 < 8192 ? (ne + 255) / 256 : 8192);
    hipLaunchKernelGGL(dwa_norm_rows, dim3(nb), dim3(256), 0, s, x, st, R, D, XL, W + w.xn, W + w.h1, W + w.h2, ones);
    if (done("dwa_norm_rows")) return -1;
    Mm G{};
    G.N = HID; G.K = D; G.lda = XL; G.ldb = D; G.ldc = HL; G.kc = (D + TK - 1) / TK * TK; G.nz = 1; G.mode = E_BIAS_RELU;
    for (int i = 0; i < nn; ++i) G.op[i] = MmOp{W + w.xn, p + o.w1[n0 + i], p + o.b1[n0 + i], W + w.h1 + (size_t)(n0 + i) * R * HL, R};
    if (mm(s, 0, 1, G, nn, R)) return -1;
    G.K = HID; G.lda = HL; G.ldb = HID; G.kc = HID;
    for (int i = 0; i < nn; ++i)
        G.op[i] = MmOp{W + w.h1 + (size_t)(n0 + i) * R * HL, p + o.w2[n0 + i], p + o.b2[n0 + i], W + w.h2 + (size_t)(n0 + i) * R * HL, R};
    return mm(s, 0, 1, G, nn, R);
}

// [dW | db] += slab-summed X^T [Y | 1] of both nets over the B rows (X: [B][ldx], M columns live; Y: [B][HL or XL], N - 1 columns)
int wgrad(hipStream_t s, const float *X0, const float *X1, int ldx, const int (&M)[2], const float *Y0, const float *Y1, int ldy, int N, int B,
          float *gw0, float *gb0, float *gw1, float *gb1, float *slab) {
    const int nz = slabs_of(B), kc = ((B + nz - 1) / nz + TK - 1) / TK * TK;
    const long long zs = (long long)(M[0] > M[1] ? M[0] : M[1]) * N;
    Mm G{};
    G.N = N; G.K = B; G.lda = ldx; G.ldb = ldy; G.ldc = N; G.kc = kc; G.nz = nz; G.mode = E_STORE; G.zstride = zs;
    G.op[0] = MmOp{X0, Y0, nullptr, slab, M[0]};
    G.op[1] = MmOp{X1, Y1, nullptr, slab + (size_t)nz * zs, M[1]};
    if (mm(s, 1, 0, G, 2, M[0] > M[1] ? M[0] : M[1])) return -1;
    SlabSum S{slab, {gw0, gw1}, {gb0, gb1}, {M[0], M[1]}, N, nz, zs};
    hipLaunchKernelGGL(dwa_slab_sum, dim3(((M[0] > M[1] ? M[0] : M[1]) * N + 255) / 256, 2), dim3(256), 0, s, S);
    return done("dwa_slab_sum");
}

}  // namespace

extern "C" {

int dwa_abi_version(void) { return DWA_ABI_VERSION; }
const char *dwa_last_error(void) { return g_err; }

int64_t dwa_workspace_bytes(int32_t rows, int32_t D, int32_t A, int32_t grad) {
    if (!check_da(D, A) || rows < 1 || (grad != 0 && grad != 1)) return -1;
    return (int64_t)layout(rows, D, grad).end * 4;
}
int64_t dwa_stats_workspace_bytes(int32_t D) { return D >= 1 && D <= DWA_D_MAX ? (int64_t)STAT_PARTS * 2 * D * 8 : -1; }

int dwa_stats(const float *x, int32_t B, int32_t D, const double *stats_in, double *stats_out, void *work, void *stream) {
    if (!x || !stats_in || !stats_out || !work || B < 2) return fail("dwa_stats: bad argument (an unbiased variance needs B >= 2)");
    if (D < 1 || D > DWA_D_MAX) return fail("dwa_stats: D must be in [1, 512]");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dwa_stats_part, dim3(STAT_PARTS), dim3(256), 0, s, x, B, D, (double *)work);
    if (done("dwa_stats_part")) return -1;
    hipLaunchKernelGGL(dwa_stats_fin, dim3(1), dim3(256), 0, s, (const double *)work, B, D, stats_in, stats_out);
    return done("dwa_stats_fin");
}

int dwa_act(const float *p, const double *obs_stats, const double *val_stats, const float *logstd, const float *obs, const float *noise, int32_t N,
            int32_t D, int32_t A, float *action, float *clamped, float *mu, float *neglogp, float *value, void *work, int64_t work_bytes,
            void *stream) {
    if (!p || !obs_stats || !val_stats || !logstd || !obs || !noise || !action || !clamped || !mu || !neglogp || !value || !work || N < 1)
        return fail("dwa_act: bad argument");
    if (!check_da(D, A)) return fail("dwa_act: D must be in [1, 512] and A in [1, 16]");
    const Work w = layout(N, D, 0);
    if (work_bytes < (int64_t)w.end * 4) return fail("dwa_act: workspace too small (dwa_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float *W = (float *)work;
    if (forward(s, p, obs_stats, obs, N, D, A, 0, 2, W, w, 0)) return -1;
    hipLaunchKernelGGL(dwa_act_out, dim3((N + RW - 1) / RW), dim3(64 * RW), 0, s, p, val_stats, logstd, noise, W + w.h2, N, D, A, action, clamped,
                       mu, neglogp, value);
    return done("dwa_act_out");
}

int dwa_critic(const float *p, const double *obs_stats, const double *val_stats, const float *obs, const float *terminate, int32_t N, int32_t D,
               int32_t A, float *value, void *work, int64_t work_bytes, void *stream) {
    if (!p || !obs_stats || !val_stats || !obs || !terminate || !value || !work || N < 1) return fail("dwa_critic: bad argument");
    if (!check_da(D, A)) return fail("dwa_critic: D must be in [1, 512] and A in [1, 16]");
    const Work w = layout(N, D, 0);
    if (work_bytes < (int64_t)w.end * 4) return fail("dwa_critic: workspace too small (dwa_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float *W = (float *)work;
    if (forward(s, p, obs_stats, obs, N, D, A, 1, 1, W, w, 0)) return -1;
    hipLaunchKernelGGL(dwa_critic_out, dim3((N + RW - 1) / RW), dim3(64 * RW), 0, s, p, val_stats, terminate, W + w.h2 + (size_t)N * HL, N, D, A,
                       value);
    return done("dwa_critic_out");
}

int dwa_grad(const float *p, const double *obs_stats, const float *logstd, const float *obs, const float *act, const float *old_nlp, const float *adv,
             const float *ret_n, int32_t B, int32_t D, int32_t A, DwaLoss coef, float *g, float *state, void *work, int64_t work_bytes,
             void *stream) {
    if (!p || !obs_stats || !logstd || !obs || !act || !old_nlp || !adv || !ret_n || !g || !state || !work || B < 1)
        return fail("dwa_grad: bad argument");
    if (!check_da(D, A)) return fail("dwa_grad: D must be in [1, 512] and A in [1, 16]");
    const Work w = layout(B, D, 1);
    if (work_bytes < (int64_t)w.end * 4) return fail("dwa_grad: workspace too small (dwa_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float *W = (float *)work;
    const Off o = offsets(D, A);
    const size_t BH = (size_t)B * HL;
    if (forward(s, p, obs_stats, obs, B, D, A, 0, 2, W, w, 1)) return -1;
    const int nb = (B + RW - 1) / RW < HEAD_BLOCKS ? (B + RW - 1) / RW : HEAD_BLOCKS;
    const Heads H{p, logstd, act, old_nlp, adv, ret_n, W + w.h2, W + w.dd, W + w.z2, W + w.part, B, D, A, coef};
    hipLaunchKernelGGL(dwa_heads_bwd, dim3(nb), dim3(64 * RW), 0, s, H);
    if (done("dwa_heads_bwd")) return -1;
    hipLaunchKernelGGL(dwa_log_sum, dim3(1), dim3(64), 0, s, (const float *)(W + w.part), nb, B, state);
    if (done("dwa_log_sum")) return -1;
    float *h1 = W + w.h1, *h2 = W + w.h2, *z2 = W + w.z2, *slab = W + w.slab;
    // the heads: [dmuW | dmub] = dmu^T [h2a | 1], [dw | db] = dv^T [h2c | 1]
    if (wgrad(s, W + w.dd, W + w.dd + 16, DL, {A, 1}, h2, h2 + BH, HL, HID + 1, B, g + o.hw[0], g + o.hb[0], g + o.hw[1], g + o.hb[1], slab))
        return -1;
    // layer 2: [dW2 | db2] = dZ2^T [h1 | 1]
    if (wgrad(s, z2, z2 + BH, HL, {HID, HID}, h1, h1 + BH, HL, HID + 1, B, g + o.w2[0], g + o.b2[0], g + o.w2[1], g + o.b2[1], slab)) return -1;
    // dZ1 = relu'(h1) * (dZ2 W2), over h1
    Mm G{};
    G.N = HID; G.K = HID; G.lda = HL; G.ldb = HID; G.ldc = HL; G.kc = HID; G.nz = 1; G.mode = E_MASK;
    for (int n = 0; n < 2; ++n) G.op[n] = MmOp{z2 + n * BH, p + o.w2[n], nullptr, h1 + n * BH, B};
    if (mm(s, 0, 0, G, 2, B)) return -1;
    // layer 1: [dW1 | db1] = dZ1^T [x | 1]
    return wgrad(s, h1, h1 + BH, HL, {HID, HID}, W + w.xn, W + w.xn, xl_of(D), D + 1, B, g + o.w1[0], g + o.b1[0], g + o.w1[1], g + o.b1[1], slab);
}

int dwa_opt(float *p, float *g, float *m, float *v, float *state, int32_t D, int32_t A, void *stream) {
    if (!p || !g || !m || !v || !state) return fail("dwa_opt: bad argument");
    if (!check_da(D, A)) return fail("dwa_opt: D must be in [1, 512] and A in [1, 16]");
    hipStream_t s = (hipStream_t)stream;
    const int NP = DWA_NP(D, A);
    hipLaunchKernelGGL(dwa_opt_step, dim3((NP + 255) / 256), dim3(256), 0, s, p, g, m, v, state, NP);
    if (done("dwa_opt_step")) return -1;
    hipLaunchKernelGGL(dwa_opt_tick, dim3(1), dim3(1), 0, s, state);
    return done("dwa_opt_tick");
}

int64_t dwa_play_workspace_bytes(int32_t N, int32_t D, int32_t A) {
    if (!check_da(D, A) || N < 1) return -1;
    return N <= PLAY_SMALL_N ? (int64_t)2 * N * HID * 4 : 0;
}

int dwa_play(const float *p, const double *obs_stats, const float *logstd, const float *obs, const float *noise, int32_t N, int32_t D, int32_t A,
             float *clamped, float *mu, void *work, int64_t work_bytes, void *stream) {
    if (!p || !obs_stats || !obs || !clamped || N < 1 || (noise && !logstd)) return fail("dwa_play: bad argument");
    if (!check_da(D, A)) return fail("dwa_play: D must be in [1, 512] and A in [1, 16]");
    const int64_t need = dwa_play_workspace_bytes(N, D, A);
    if (work_bytes < need || (need > 0 && !work)) return fail("dwa_play: workspace too small (dwa_play_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int pal = !((uintptr_t)p & 15), oal = !((uintptr_t)obs & 15) && !(D & 3);
    Play P{p, logstd, obs, noise, obs_stats, clamped, mu, (float *)work, (float *)work + (size_t)N * HID, N, D, A, pal, oal};
    if (N > PLAY_SMALL_N) {
        hipLaunchKernelGGL(dwa_play_rows, dim3((N + PR - 1) / PR), dim3(256), 0, s, P);
        return done("dwa_play_rows");
    }
    hipLaunchKernelGGL((dwa_play_cols<1>), dim3(HID / 16), dim3(256), 0, s, P);
    if (done("dwa_play_cols")) return -1;
    hipLaunchKernelGGL((dwa_play_cols<0>), dim3(HID / 16), dim3(256), 0, s, P);
    if (done("dwa_play_cols")) return -1;
    hipLaunchKernelGGL(dwa_play_head, dim3((N + PR - 1) / PR), dim3(256), 0, s, P);
    return done("dwa_play_head");
}

int dwa_gae(const float *done_, const float *values, const float *rewards, const float *next_values, int32_t H, int32_t N, float gamma,
            float gamma_tau, float *adv, float *ret, void *stream) {
    if (!done_ || !values || !rewards || !next_values || !adv || !ret || H < 1 || N < 1) return fail("dwa_gae: bad argument");
    hipLaunchKernelGGL(dwa_gae_scan, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, done_, values, rewards, next_values, H, N, gamma,
                       gamma_tau, adv, ret);
    return done("dwa_gae_scan");
}

}  // extern "C"
