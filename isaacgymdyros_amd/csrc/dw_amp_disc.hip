// dw_amp_disc.hip -- the AMP discriminator of the consumer's side of TocabiAMPLower (include/dyros_amp_disc.h; reference:
// learning/amp_continuous.py:260-329, 404-457, 500-543, learning/amp_network_builder.py:74-110).  gfx950, fp32 throughout, products on the
// vector unit.  Every reduction runs in a fixed order (split-K products write one partial slab per workgroup, summed in slab order by
// dwd_k_disc_finish), so a replayed graph gives the bits of the eager launches.
//
// The gradient penalty as an analytic double backward.  With relu masks m1 = (h1 > 0), m2 = (h2 > 0) held constant (torch's relu backward
// has no gradient with respect to its mask), the input gradient of one row's logit is a chain of products with the layer matrices:
//   u2 = m2 * w3,   u1 = m1 * (W2^T u2),   g = W1^T u1                                         (g = d logit / d x, [D])
// and P = gp / Bd * sum_rows |g|^2 back through that chain, with G = 2 gp / Bd * g:
//   dW1 += u1 G^T,   dV1 = m1 * (W1 G),   dW2 += u2 dV1^T,   dw3 += m2 * (W2 dV1)      (no bias gradient: the masks are constants)
// The BCE part of the same row backpropagates dl = d loss / d logit through the same vectors: dz2 = dl u2, dz1 = dl u1, so for every row
//   dW2 += u2 (dl h1 + [demo] dV1)^T,   dW1 += u1 (dl x + [demo] G)^T,   dw3 += dl h2 + [demo] m2 * (W2 dV1)
// and the bias gradients are the same sums with a column of dl appended to the right operand.  Each of these is ONE product over the
// rows of the minibatch (dwd_grad: the right operands are built in place of h1, h2 and x by dwd_k_disc_build).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/dyros_amp_disc.h"

namespace {

char g_err[256] = "";
int fail_hip(const char *who, hipError_t e) { snprintf(g_err, sizeof(g_err), "%s: %s", who, hipGetErrorString(e)); return -1; }
int fail(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return -1; }
int done(const char *who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(who, e);
}

constexpr int HID = DWD_HID;
constexpr int HL = HID + 1;          // row length of the hidden-layer matrices: the column past the last holds dl for the bias gradients
constexpr float NORM_EPS = 1e-5f, NORM_CLIP = 5.0f;

// offsets into the parameter layout
__host__ __device__ inline size_t off_b1(int D) { return (size_t)D * HID; }
__host__ __device__ inline size_t off_w2(int D) { return off_b1(D) + HID; }
__host__ __device__ inline size_t off_b2(int D) { return off_w2(D) + (size_t)HID * HID; }
__host__ __device__ inline size_t off_w3(int D) { return off_b2(D) + HID; }
__host__ __device__ inline size_t off_b3(int D) { return off_w3(D) + HID; }

// rl_games' RunningMeanStd normalisation: (x - mean) / sqrt(var + 1e-5) with the fp64 statistics cast to fp32 first, clamped to +-5
__device__ __forceinline__ float normalise(float x, const double *__restrict__ st, int D, int k) {
    const float mu = (float)st[k], var = (float)st[D + k];
    const float y = (x - mu) / sqrtf(var + NORM_EPS);
    return fminf(fmaxf(y, -NORM_CLIP), NORM_CLIP);
}

// ------------------------------------------------------------------------------------------------------------------------- the reward
// 32 rows per workgroup of 256 threads: thread (rg = t >> 5, cg = t & 31) owns rows 4 rg .. 4 rg + 3 and columns cg + 32 j (j < 8).  The
// normalised rows sit in LDS (zero-padded to a multiple of 16 columns); the first hidden layer replaces them there; a 16-deep slice of the
// layer's weights is staged per step, transposed so that a wave's reads are conflict-free.
constexpr int RR = 32, RK = 16, XS = 356;          // XS >= DWD_D_MAX rounded up to 16, + 4 against bank conflicts; >= HL
static_assert(XS >= ((DWD_D_MAX + 15) / 16) * 16 && XS >= HID + 4, "LDS row");

__device__ __forceinline__ void row_layer(const float *__restrict__ As, const float *__restrict__ W, int K, int KP, float *__restrict__ Ws,
                                          float (&acc)[4][8], int t) {
    const int rg = t >> 5, cg = t & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
    for (int kc = 0; kc < KP; kc += RK) {
        __syncthreads();          // (the previous slice is consumed)
        const float *wr = W + (size_t)t * K + kc;          // thread t stages row t of W (output t), 16 columns
#pragma unroll
        for (int kk = 0; kk < RK; ++kk) Ws[kk * HID + t] = kc + kk < K ? wr[kk] : 0.0f;
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < RK; ++kk) {
            float a[4], b[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[(4 * rg + i) * XS + kc + kk];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = Ws[kk * HID + cg + 32 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
    }
}

__global__ __launch_bounds__(256) void dwd_k_fwd_reward(const float *__restrict__ p, const double *__restrict__ st, const float *__restrict__ x,
                                                        const float *__restrict__ task, int B, int D, float scale, float task_w, float disc_w,
                                                        float *__restrict__ disc_r, float *__restrict__ combined, float *__restrict__ logits) {
    __shared__ float Xs[RR * XS];
    __shared__ float Ws[RK * HID];
    const int t = threadIdx.x, rg = t >> 5, cg = t & 31, r0 = blockIdx.x * RR, DP = (D + RK - 1) / RK * RK;
    for (int e = t; e < RR * DP; e += 256) {
        const int r = e / DP, k = e - r * DP;
        Xs[r * XS + k] = (r0 + r < B && k < D) ? normalise(x[(size_t)(r0 + r) * D + k], st, D, k) : 0.0f;
    }
    float acc[4][8];
    row_layer(Xs, p, D, DP, Ws, acc, t);
    const float *b1 = p + off_b1(D);
    __syncthreads();          // (every thread is past its last read of the rows: the hidden layer replaces them)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float bj = b1[cg + 32 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i) Xs[(4 * rg + i) * XS + cg + 32 * j] = fmaxf(acc[i][j] + bj, 0.0f);
    }
    row_layer(Xs, p + off_w2(D), HID, HID, Ws, acc, t);
    const float *b2 = p + off_b2(D), *w3 = p + off_w3(D);
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float bj = b2[cg + 32 * j], wj = w3[cg + 32 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fmaf(wj, fmaxf(acc[i][j] + bj, 0.0f), s[i]);
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += __shfl_xor(s[i], o, 64);          // (within the 32 lanes of one row group)
    if (cg == 0) {
        const float b3 = p[off_b3(D)];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 4 * rg + i;
            if (r < B) {
                const float l = s[i] + b3;
                const float prob = 1.0f / (1.0f + expf(-l));
                const float dr = -logf(fmaxf(1.0f - prob, 1e-4f)) * scale;
                disc_r[r] = dr;
                combined[r] = task_w * task[r] + disc_w * dr;
                if (logits) logits[r] = l;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- statistics
constexpr int STAT_PARTS = 1024;          // (many short row slabs: each thread's loop is a chain of dependent adds)
__global__ __launch_bounds__(256) void dwd_k_stats_part(const float *__restrict__ x, int B, int D, double *__restrict__ part) {
    const int b = blockIdx.x, lo = (int)((long)B * b / STAT_PARTS), hi = (int)((long)B * (b + 1) / STAT_PARTS);
    for (int c = threadIdx.x; c < D; c += 256) {
        double s = 0.0, q = 0.0;
#pragma unroll 8
        for (int r = lo; r < hi; ++r) {
            const double v = x[(size_t)r * D + c];
            s += v;
            q += v * v;
        }
        part[(size_t)b * 2 * D + c] = s;
        part[(size_t)b * 2 * D + D + c] = q;
    }
}
__global__ __launch_bounds__(256) void dwd_k_stats_fin(const double *__restrict__ part, int B, int D, const double *__restrict__ in,
                                                       double *__restrict__ out) {
    const double n = (double)B, count = in[2 * D], tot = count + n;
    for (int c = threadIdx.x; c < D; c += 256) {
        double s = 0.0, q = 0.0;
#pragma unroll 8
        for (int b = 0; b < STAT_PARTS; ++b) { s += part[(size_t)b * 2 * D + c]; q += part[(size_t)b * 2 * D + D + c]; }
        const double bm = s / n, bv = fmax(q - s * bm, 0.0) / (n - 1.0);          // unbiased, as torch.var
        const double mean = in[c], var = in[D + c], delta = bm - mean;
        out[c] = mean + delta * n / tot;
        out[D + c] = (var * count + bv * n + delta * delta * count * n / tot) / tot;
    }
    __syncthreads();          // (every thread has read in[2 D] before out may alias it)
    if (threadIdx.x == 0) out[2 * D] = tot;
}

// ------------------------------------------------------------------------------------------------------------------------- products
// C = alpha * op(A) op(B) over a 128 x 128 tile, 16-deep slices through LDS, 8 x 8 results per thread.  op(A)(m, k) = ta ? A[k lda + m] :
// A[m lda + k].  Split over K: workgroup z covers [z kc, (z + 1) kc) and writes its own slab C + z M ldc.
constexpr int GM = 128, GN = 128, GK = 16, GPAD = 4;
enum { E_STORE = 0, E_BIAS_RELU = 1, E_MASK = 2 };
struct Gemm {
    const float *A, *B, *bias, *mask;
    float *C;
    int M, N, K, lda, ldb, ldc, ldm, ta, tb, kc, mode;
    float alpha;
};
__global__ __launch_bounds__(256) void dwd_k_gemm(const Gemm G) {
    __shared__ float As[GK][GM + GPAD];
    __shared__ float Bs[GK][GN + GPAD];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int n0 = blockIdx.x * GN, m0 = blockIdx.y * GM, k0 = blockIdx.z * G.kc;
    const int k1 = min(G.K, k0 + G.kc);
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
    for (int kb = k0; kb < k1; kb += GK) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = t + 256 * q;
            int m, k;
            if (G.ta) { k = e >> 7; m = e & 127; } else { m = e >> 4; k = e & 15; }
            const int gm = m0 + m, gk = kb + k;
            float v = 0.0f;
            if (gm < G.M && gk < k1) v = G.A[G.ta ? (size_t)gk * G.lda + gm : (size_t)gm * G.lda + gk];
            As[k][m] = v;
            int n;
            if (G.tb) { n = e >> 4; k = e & 15; } else { k = e >> 7; n = e & 127; }
            const int gn = n0 + n, gk2 = kb + k;
            Bs[k][n] = (gn < G.N && gk2 < k1) ? G.B[G.tb ? (size_t)gn * G.ldb + gk2 : (size_t)gk2 * G.ldb + gn] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < GK; ++kk) {
            float a[8], b[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = Bs[kk][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    float *C = G.C + (size_t)blockIdx.z * G.M * G.ldc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + ty + 16 * i;
        if (m >= G.M) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = n0 + tx + 16 * j;
            if (n >= G.N) continue;
            float v = G.alpha * acc[i][j];
            if (G.mode == E_BIAS_RELU) v = fmaxf(acc[i][j] + G.bias[n], 0.0f);
            else if (G.mode == E_MASK) v = G.mask[(size_t)m * G.ldm + n] > 0.0f ? v : 0.0f;
            C[(size_t)m * G.ldc + n] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- the loss
struct Rows {
    const float *agent, *replay, *demo;
    const double *st_agent, *st_replay, *st_demo;
    int na, nr, nd, D;
};
__device__ __forceinline__ float row_in(const Rows &R, int r, int k) {
    if (r < R.na) return normalise(R.agent[(size_t)r * R.D + k], R.st_agent, R.D, k);
    r -= R.na;
    if (r < R.nr) return normalise(R.replay[(size_t)r * R.D + k], R.st_replay, R.D, k);
    r -= R.nr;
    return normalise(R.demo[(size_t)r * R.D + k], R.st_demo, R.D, k);
}
// xn [R][D + 1]: the rows normalised with their own set's snapshot
__global__ __launch_bounds__(256) void dwd_k_disc_norm(const Rows R, float *__restrict__ xn) {
    const size_t n = (size_t)(R.na + R.nr + R.nd) * R.D;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / R.D), k = (int)(e - (size_t)r * R.D);
        xn[(size_t)r * (R.D + 1) + k] = row_in(R, r, k);
    }
}

// One wave per row: the logit from h2, dl = d (disc_coef disc_loss) / d logit, u2 = m2 * w3, and per workgroup the logged sums
// (agent BCE, demo BCE, agent logit, demo logit, agent hits, demo hits) in fixed order.
constexpr int HEAD_ROWS = 64;          // rows per workgroup (16 per wave)
__global__ __launch_bounds__(256) void dwd_k_disc_head(const float *__restrict__ p, const float *__restrict__ h2, int R, int nA, int D, float ca, float cd,
                                                      float *__restrict__ u2, float *__restrict__ dl, double *__restrict__ part) {
    __shared__ double red[4][6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *w3 = p + off_w3(D);
    const float b3 = p[off_b3(D)];
    float w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = w3[lane + 64 * q];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < HEAD_ROWS / 4; ++k) {
        const int r = blockIdx.x * HEAD_ROWS + wv * (HEAD_ROWS / 4) + k;
        if (r >= R) break;
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float h = h2[(size_t)r * HL + lane + 64 * q];
            s = fmaf(w[q], h, s);
            u2[(size_t)r * HID + lane + 64 * q] = h > 0.0f ? w[q] : 0.0f;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        const float l = s + b3, sig = 1.0f / (1.0f + expf(-l));
        const bool agent = r < nA;
        if (lane == 0) dl[r] = agent ? ca * sig : cd * (sig - 1.0f);
        const double sp = log1p(exp(-fabs((double)l)));          // BCE with logits: softplus(l) against 0, softplus(-l) against 1
        if (agent) { acc[0] += fmax((double)l, 0.0) + sp; acc[2] += l; acc[4] += l < 0.0f; }
        else { acc[1] += fmax(-(double)l, 0.0) + sp; acc[3] += l; acc[5] += l > 0.0f; }
    }
    if (lane == 0)
        for (int i = 0; i < 6; ++i) red[wv][i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 6) part[(size_t)blockIdx.x * 6 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The right operands of the weight-gradient products, in place, one wave per row (r >= nA: a demo row, rd = r - nA):
//   h1 <- dl h1 + [demo] dv1,  h2 <- dl h2 + [demo] e2 (= m2 * W2 dV1),  xn <- dl xn + [demo] alpha gx;  the last column of each <- dl.
// gpr[rd] = |gx|^2 (the demo row's |d logit / d x|^2).
__global__ __launch_bounds__(256) void dwd_k_disc_build(float *__restrict__ h1, float *__restrict__ h2, float *__restrict__ xn, const float *__restrict__ dl,
                                                       const float *__restrict__ dv1, const float *__restrict__ e2, const float *__restrict__ gx, int R, int nA,
                                                       int D, float alpha, double *__restrict__ gpr) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float d = dl[r];
    const int rd = r - nA;
    const bool demo = rd >= 0;
    float *a = h1 + (size_t)r * HL, *b = h2 + (size_t)r * HL, *x = xn + (size_t)r * (D + 1);
    for (int j = lane; j < HID; j += 64) {
        a[j] = d * a[j] + (demo ? dv1[(size_t)rd * HID + j] : 0.0f);
        b[j] = d * b[j] + (demo ? e2[(size_t)rd * HID + j] : 0.0f);
    }
    double q = 0.0;
    for (int k = lane; k < D; k += 64) {
        const float gk = demo ? gx[(size_t)rd * D + k] : 0.0f;
        x[k] = d * x[k] + alpha * gk;
        q += (double)gk * gk;
    }
    if (lane == 0) { a[HID] = d; b[HID] = d; x[D] = d; }
    if (demo) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
        if (lane == 0) gpr[rd] = q;
    }
}

// P3 [S3][HL]: slab z's column sums of h2' over its rows (the third weight gradient: dw3 | db3 = column sums of h2').  Four row phases per
// slab (1024 threads), combined in phase order.
__global__ __launch_bounds__(1024) void dwd_k_disc_colsum(const float *__restrict__ h2, int R, int kc, float *__restrict__ P3) {
    __shared__ float red[4][HL];
    const int z = blockIdx.x, lo = z * kc, hi = min(R, lo + kc), ph = threadIdx.x >> 8, c = threadIdx.x & 255;
    float s = 0.0f, s_dl = 0.0f;
#pragma unroll 8
    for (int r = lo + ph; r < hi; r += 4) {
        s += h2[(size_t)r * HL + c];
        if (c == 0) s_dl += h2[(size_t)r * HL + HID];
    }
    red[ph][c] = s;
    if (c == 0) red[ph][HID] = s_dl;
    __syncthreads();
    if (threadIdx.x < HL) P3[(size_t)z * HL + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// g += the slab sums of the three weight-gradient products (P1 [S][HID][D + 1], P2 [S][HID][HL], P3 [S][HL]) + the regularisers' gradients.
// The last workgroup reduces the logged sums into state.
struct Finish {
    const float *p, *P1, *P2, *P3;
    const double *head, *gpr;
    float *g, *state;
    int D, S1, S2, S3, nhead, nA, nd;
    float coef, lreg, gpen, wdec;
};
__global__ __launch_bounds__(256) void dwd_k_disc_finish(const Finish F) {
    const int D = F.D, NP = DWD_NP(D);
    if (blockIdx.x + 1 < gridDim.x) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= NP) return;
        const float wreg = 2.0f * F.coef * F.wdec;
        float s = 0.0f, reg = 0.0f;
        size_t o;
        if (i < (int)off_b1(D)) {
            const int j = i / D, k = i - j * D;
            o = (size_t)j * (D + 1) + k;
            for (int z = 0; z < F.S1; ++z) s += F.P1[(size_t)z * HID * (D + 1) + o];
            reg = wreg * F.p[i];
        } else if (i < (int)off_w2(D)) {
            o = (size_t)(i - off_b1(D)) * (D + 1) + D;
            for (int z = 0; z < F.S1; ++z) s += F.P1[(size_t)z * HID * (D + 1) + o];
        } else if (i < (int)off_b2(D)) {
            const int e = i - (int)off_w2(D), a = e / HID, b = e - a * HID;
            o = (size_t)a * HL + b;
            for (int z = 0; z < F.S2; ++z) s += F.P2[(size_t)z * HID * HL + o];
            reg = wreg * F.p[i];
        } else if (i < (int)off_w3(D)) {
            o = (size_t)(i - off_b2(D)) * HL + HID;
            for (int z = 0; z < F.S2; ++z) s += F.P2[(size_t)z * HID * HL + o];
        } else {
            o = (size_t)(i - off_w3(D));          // w3 [0, HID) and b3 (HID)
#pragma unroll 8
            for (int z = 0; z < F.S3; ++z) s += F.P3[(size_t)z * HL + o];
            if (o < HID) reg = 2.0f * F.coef * (F.lreg + F.wdec) * F.p[i];
        }
        F.g[i] += s + reg;
        return;
    }
    // the logged values: sums in thread order, then a fixed tree
    __shared__ double red[256][8];
    const int t = threadIdx.x;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = t; b < F.nhead; b += 256)
        for (int c = 0; c < 6; ++c) v[c] += F.head[(size_t)b * 6 + c];
    for (int r = t; r < F.nd; r += 256) v[6] += F.gpr[r];
    const int nw = (int)off_b1(D);
    for (int i = t; i < NP; i += 256) {
        const bool wt = i < nw || (i >= (int)off_w2(D) && i < (int)off_b2(D)) || (i >= (int)off_w3(D) && i < (int)off_b3(D));
        const double x = F.p[i];
        if (wt) v[7] += x * x;
    }
    for (int c = 0; c < 8; ++c) red[t][c] = v[c];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w)
            for (int c = 0; c < 8; ++c) red[t][c] += red[t + w][c];
        __syncthreads();
    }
    if (t == 0) {
        double lsq = 0.0;
        for (int j = 0; j < HID; ++j) lsq += (double)F.p[off_w3(D) + j] * F.p[off_w3(D) + j];
        const double nA = F.nA, nd = F.nd;
        const double pred = 0.5 * (red[0][0] / nA + red[0][1] / nd), gp = red[0][6] / nd, wd = red[0][7];
        float *S = F.state;
        S[DWD_S_LOSS] += (float)(F.coef * (pred + F.lreg * lsq + F.gpen * gp + F.wdec * wd));
        S[DWD_S_PRED] += (float)pred;
        S[DWD_S_LOGIT_REG] += (float)lsq;
        S[DWD_S_GRAD_PEN] += (float)gp;
        S[DWD_S_WEIGHT_DEC] += (float)wd;
        S[DWD_S_AGENT_LOGIT] += (float)(red[0][2] / nA);
        S[DWD_S_DEMO_LOGIT] += (float)(red[0][3] / nd);
        S[DWD_S_AGENT_ACC] += (float)(red[0][4] / nA);
        S[DWD_S_DEMO_ACC] += (float)(red[0][5] / nd);
        S[DWD_S_UPDATES] += 1.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- Adam
// torch.optim.Adam (foreach form): m.lerp_(g, 1 - b1); v = v * b2 + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void dwd_k_disc_step(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                                       const float *__restrict__ state, int NP) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NP) return;
    const double step = (double)state[DWD_S_STEP] + 1.0;
    const float step_size = (float)((double)state[DWD_S_LR] / (1.0 - pow(0.9, step)));
    const float bc2s = (float)sqrt(1.0 - pow(0.999, step));
    const float gi = g[i];
    const float mi = m[i] + 0.1f * (gi - m[i]);
    const float vi = v[i] * 0.999f + (float)(1.0 - 0.999) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= step_size * (mi / (sqrtf(vi) / bc2s + 1e-8f));
    g[i] = 0.0f;
}
__global__ void dwd_k_disc_tick(float *__restrict__ state) { state[DWD_S_STEP] += 1.0f; }

// ------------------------------------------------------------------------------------------------------------------------- host side
int check_d(int D) { return D >= DWD_OBS_STEP && D <= DWD_D_MAX && D % DWD_OBS_STEP == 0; }

int gemm(hipStream_t s, const float *A, int ta, int lda, const float *B, int tb, int ldb, float *C, int ldc, int M, int N, int K, int mode,
         float alpha, const float *bias, const float *mask, int ldm, int slabs) {
    Gemm G{A, B, bias, mask, C, M, N, K, lda, ldb, ldc, ldm, ta, tb, 0, mode, alpha};
    G.kc = ((K + slabs - 1) / slabs + GK - 1) / GK * GK;
    dim3 grid((N + GN - 1) / GN, (M + GM - 1) / GM, slabs);
    hipLaunchKernelGGL(dwd_k_gemm, grid, dim3(256), 0, s, G);
    return done("dwd_k_gemm");
}

// slabs of a split over `rows`: enough workgroups to fill the chip, at least 1024 rows each (a function of the sizes only)
int slabs_for(int rows) { return rows <= 1024 ? 1 : (rows / 1024 < 64 ? rows / 1024 : 64); }

// The workspace of dwd_grad, float offsets
struct Ws {
    size_t xn, h1, h2, u2, u1, gx, dv1, e2, dl, head, gpr, P1, P2, P3, end;
    int S, S3;
};
Ws layout(int D, int na, int nr, int nd) {
    const size_t R = (size_t)na + nr + nd;
    const int S = slabs_for((int)R);
    Ws w;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t a = o; o += (n + 63) / 64 * 64; return a; };
    w.xn = take(R * (D + 1));
    w.h1 = take(R * HL);
    w.h2 = take(R * HL);
    w.u2 = take(R * HID);
    w.u1 = take(R * HID);
    w.gx = take((size_t)nd * D);
    w.dv1 = take((size_t)nd * HID);
    w.e2 = take((size_t)nd * HID);
    w.dl = take(R);
    w.head = take(2 * 6 * ((R + HEAD_ROWS - 1) / HEAD_ROWS));          // doubles
    w.gpr = take(2 * (size_t)nd);                                      // doubles
    w.P1 = take((size_t)S * HID * (D + 1));
    w.P2 = take((size_t)S * HID * HL);
    const int S3 = 4 * S;          // (dwd_k_disc_colsum: more, shorter slabs -- its loop is a chain of dependent loads)
    w.P3 = take((size_t)S3 * HL);
    w.end = o;
    w.S = S;
    w.S3 = S3;
    return w;
}

}  // namespace

extern "C" {

int dwd_abi_version(void) { return DWD_ABI_VERSION; }
const char *dwd_last_error(void) { return g_err; }

int64_t dwd_grad_workspace_bytes(int32_t D, int32_t na, int32_t nr, int32_t nd) {
    if (!check_d(D) || na < 0 || nr < 0 || nd < 1 || na + nr < 1) return -1;
    return (int64_t)layout(D, na, nr, nd).end * 4;
}
int64_t dwd_stats_workspace_bytes(int32_t D) { return check_d(D) ? (int64_t)STAT_PARTS * 2 * D * 8 : -1; }

int dwd_reward(const float *p, const double *stats, const float *amp_obs, const float *task_rew, int32_t B, int32_t D, float reward_scale,
               float task_w, float disc_w, float *disc_r, float *combined, float *logits, void *stream) {
    if (!p || !stats || !amp_obs || !task_rew || !disc_r || !combined || B < 1) return fail("dwd_reward: bad argument");
    if (!check_d(D)) return fail("dwd_reward: D must be a multiple of 34 in [34, 340]");
    hipLaunchKernelGGL(dwd_k_fwd_reward, dim3((B + RR - 1) / RR), dim3(256), 0, (hipStream_t)stream, p, stats, amp_obs, task_rew, B, D, reward_scale,
                       task_w, disc_w, disc_r, combined, logits);
    return done("dwd_reward");
}

int dwd_stats(const float *x, int32_t B, int32_t D, const double *stats_in, double *stats_out, void *work, void *stream) {
    if (!x || !stats_in || !stats_out || !work || B < 2) return fail("dwd_stats: bad argument (an unbiased variance needs B >= 2)");
    if (!check_d(D)) return fail("dwd_stats: D must be a multiple of 34 in [34, 340]");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dwd_k_stats_part, dim3(STAT_PARTS), dim3(256), 0, s, x, B, D, (double *)work);
    if (done("dwd_k_stats_part")) return -1;
    hipLaunchKernelGGL(dwd_k_stats_fin, dim3(1), dim3(256), 0, s, (const double *)work, B, D, stats_in, stats_out);
    return done("dwd_k_stats_fin");
}

int dwd_grad(const float *p, const float *agent, int32_t na, const float *replay, int32_t nr, const float *demo, int32_t nd, int32_t D,
             const double *st_a, const double *st_r, const double *st_d, DwdLoss c, float *g, float *state, void *work, int64_t work_bytes, void *stream) {
    if (!p || !demo || !st_d || !g || !state || !work || nd < 1 || na < 0 || nr < 0 || na + nr < 1) return fail("dwd_grad: bad argument");
    if ((na && (!agent || !st_a)) || (nr && (!replay || !st_r))) return fail("dwd_grad: bad argument");
    if (!check_d(D)) return fail("dwd_grad: D must be a multiple of 34 in [34, 340]");
    const Ws w = layout(D, na, nr, nd);
    if (work_bytes < (int64_t)w.end * 4) return fail("dwd_grad: workspace too small (dwd_grad_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float *W = (float *)work;
    const int R = na + nr + nd, nA = na + nr;
    float *xn = W + w.xn, *h1 = W + w.h1, *h2 = W + w.h2, *u2 = W + w.u2, *u1 = W + w.u1, *gx = W + w.gx, *dv1 = W + w.dv1, *e2 = W + w.e2,
          *dl = W + w.dl;
    double *head = (double *)(W + w.head), *gpr = (double *)(W + w.gpr);
    const float *W1 = p, *b1 = p + off_b1(D), *W2 = p + off_w2(D), *b2 = p + off_b2(D);
    const Rows rows{agent, replay, demo, st_a, st_r, st_d, na, nr, nd, D};
    const int nb = (int)(((size_t)R * D + 255) / 256);
    hipLaunchKernelGGL(dwd_k_disc_norm, dim3(nb < 8192 ? nb : 8192), dim3(256), 0, s, rows, xn);
    if (done("dwd_k_disc_norm")) return -1;
    // forward: h1 = relu(xn W1^T + b1), h2 = relu(h1 W2^T + b2)
    if (gemm(s, xn, 0, D + 1, W1, 1, D, h1, HL, R, HID, D, E_BIAS_RELU, 1.0f, b1, nullptr, 0, 1)) return -1;
    if (gemm(s, h1, 0, HL, W2, 1, HID, h2, HL, R, HID, HID, E_BIAS_RELU, 1.0f, b2, nullptr, 0, 1)) return -1;
    const int nhead = (R + HEAD_ROWS - 1) / HEAD_ROWS;
    hipLaunchKernelGGL(dwd_k_disc_head, dim3(nhead), dim3(256), 0, s, p, h2, R, nA, D, 0.5f * c.disc_coef / nA, 0.5f * c.disc_coef / nd, u2, dl, head);
    if (done("dwd_k_disc_head")) return -1;
    // u1 = m1 * (u2 W2); demo rows: gx = u1 W1, dv1 = m1 * (G W1^T) with G = alpha gx, e2 = m2 * (dv1 W2^T)
    if (gemm(s, u2, 0, HID, W2, 0, HID, u1, HID, R, HID, HID, E_MASK, 1.0f, nullptr, h1, HL, 1)) return -1;
    const float alpha = 2.0f * c.disc_coef * c.grad_penalty / nd;
    if (gemm(s, u1 + (size_t)nA * HID, 0, HID, W1, 0, D, gx, D, nd, D, HID, E_STORE, 1.0f, nullptr, nullptr, 0, 1)) return -1;
    if (gemm(s, gx, 0, D, W1, 1, D, dv1, HID, nd, HID, D, E_MASK, alpha, nullptr, h1 + (size_t)nA * HL, HL, 1)) return -1;
    if (gemm(s, dv1, 0, HID, W2, 1, HID, e2, HID, nd, HID, HID, E_MASK, 1.0f, nullptr, h2 + (size_t)nA * HL, HL, 1)) return -1;
    hipLaunchKernelGGL(dwd_k_disc_build, dim3((R + 3) / 4), dim3(256), 0, s, h1, h2, xn, dl, dv1, e2, gx, R, nA, D, alpha, gpr);
    if (done("dwd_k_disc_build")) return -1;
    // weight gradients, split over the rows: [dW1 | db1] = u1^T xn', [dW2 | db2] = u2^T h1', [dw3 | db3] = column sums of h2'
    if (gemm(s, u1, 1, HID, xn, 0, D + 1, W + w.P1, D + 1, HID, D + 1, R, E_STORE, 1.0f, nullptr, nullptr, 0, w.S)) return -1;
    if (gemm(s, u2, 1, HID, h1, 0, HL, W + w.P2, HL, HID, HL, R, E_STORE, 1.0f, nullptr, nullptr, 0, w.S)) return -1;
    hipLaunchKernelGGL(dwd_k_disc_colsum, dim3(w.S3), dim3(1024), 0, s, h2, R, (R + w.S3 - 1) / w.S3, W + w.P3);
    if (done("dwd_k_disc_colsum")) return -1;
    const Finish F{p, W + w.P1, W + w.P2, W + w.P3, head, gpr, g, state, D, w.S, w.S, w.S3, nhead, nA, nd, c.disc_coef, c.logit_reg, c.grad_penalty,
                   c.weight_decay};
    hipLaunchKernelGGL(dwd_k_disc_finish, dim3((DWD_NP(D) + 255) / 256 + 1), dim3(256), 0, s, F);
    return done("dwd_k_disc_finish");
}

int dwd_opt(float *p, float *g, float *m, float *v, float *state, int32_t D, void *stream) {
    if (!p || !g || !m || !v || !state) return fail("dwd_opt: bad argument");
    if (!check_d(D)) return fail("dwd_opt: D must be a multiple of 34 in [34, 340]");
    hipStream_t s = (hipStream_t)stream;
    const int NP = DWD_NP(D);
    hipLaunchKernelGGL(dwd_k_disc_step, dim3((NP + 255) / 256), dim3(256), 0, s, p, g, m, v, state, NP);
    if (done("dwd_k_disc_step")) return -1;
    hipLaunchKernelGGL(dwd_k_disc_tick, dim3(1), dim3(1), 0, s, state);
    return done("dwd_k_disc_tick");
}

}  // extern "C"
