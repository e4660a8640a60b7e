// A g++ build of the episode-return meter's arithmetic (isaacgymdyros_amd/csrc/dw_meter.h) with host pointers: the same functions
// dw_meter.hip runs, in the summation order include/dyros_meter.h documents, workgroup by workgroup.  tests/test_game_meter.py compiles it
// and holds it against a numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_meter.h"

namespace {

// the xor butterfly as lane 0 sees it: t[l] += t[l ^ x] for x = 32, 16, .., 1 (a + b == b + a, so every lane ends with the same bits)
float wave_sum(float *t) {
    for (int x = dwm::WAVE / 2; x >= 1; x >>= 1) {
        float u[dwm::WAVE];
        for (int l = 0; l < dwm::WAVE; ++l) u[l] = t[l] + t[l ^ x];
        memcpy(t, u, sizeof(u));
    }
    return t[0];
}

}  // namespace

extern "C" {

int64_t dwmh_work_words(int n, int cols) { return dwm::work_words(n, cols); }

int dwmh_record(int n, int cols, int max_size, const float *rew, const float *stacked, int stride, const int64_t *done, float *cur, uint32_t *ms,
                uint32_t *work) {
    const int g = dwm::groups(n), rw = dwm::row_words(cols);
    uint32_t *rows = work + dwm::HEAD;
    for (int b = 0; b < g; ++b) {
        float wsum[dwm::NW][dwm::CMAX + 1];
        uint32_t cnt[dwm::NW][2];
        for (int w = 0; w < dwm::NW; ++w) {
            float t[dwm::CMAX + 1][dwm::WAVE];
            cnt[w][0] = cnt[w][1] = 0u;
            for (int l = 0; l < dwm::WAVE; ++l) {
                const int i = b * dwm::GROUP + w * dwm::WAVE + l;
                const bool live = i < n, dn = live && done[i] != 0;
                float v[dwm::CMAX + 1];
                bool fin = true;
                for (int c = 0; c <= cols; ++c) {
                    v[c] = 0.0f;
                    if (!live) continue;
                    float *p = cur + (size_t)c * n + i;
                    v[c] = dwm::bump(*p, c == cols ? 1.0f : c == 0 ? rew[i] : stacked[(size_t)i * stride + (c - 1)]);
                    if (c < cols) fin = fin && dwm::finite(v[c]);
                    *p = dwm::keep(v[c], dn);
                }
                const bool in_d = dn && fin;
                for (int c = 0; c <= cols; ++c) t[c][l] = dwm::term(v[c], in_d);
                cnt[w][0] += in_d ? 1u : 0u;
                cnt[w][1] += (dn && !fin) ? 1u : 0u;
            }
            for (int c = 0; c <= cols; ++c) wsum[w][c] = wave_sum(t[c]);
        }
        for (int c = 0; c <= cols; ++c) rows[(size_t)b * rw + c] = dwm::f2u(dwm::group_sum(wsum[0][c], wsum[1][c], wsum[2][c], wsum[3][c]));
        for (int q = 0; q < 2; ++q) rows[(size_t)b * rw + cols + 1 + q] = cnt[0][q] + cnt[1][q] + cnt[2][q] + cnt[3][q];
    }
    // the finishing workgroup
    float acc[dwm::CMAX + 1];
    double dacc[dwm::CMAX + 1];
    uint32_t k = 0u, bad = 0u;
    for (int c = 0; c <= cols; ++c) { acc[c] = 0.0f; dacc[c] = 0.0; }
    for (int b = 0; b < g; ++b) {
        for (int c = 0; c <= cols; ++c) {
            const float x = dwm::u2f(rows[(size_t)b * rw + c]);
            acc[c] = acc[c] + x;
            dacc[c] = dacc[c] + (double)x;
        }
        k += rows[(size_t)b * rw + cols + 1];
        bad += rows[(size_t)b * rw + cols + 2];
    }
    const uint32_t current_size = ms[DWM_MS_CURRENT_SIZE];
    if (k > 0u) {
        for (int c = 0; c <= cols; ++c) {
            uint32_t *m = ms + (c < cols ? DWM_MS_MEAN + c : DWM_MS_MEAN_LEN);
            *m = dwm::f2u(dwm::window_mean(dwm::u2f(*m), acc[c], k, (uint32_t)max_size, current_size));
        }
        double d;
        uint64_t u;
        memcpy(&d, ms + DWM_MS_SUM_RET, 8); d = d + dacc[0]; memcpy(ms + DWM_MS_SUM_RET, &d, 8);
        memcpy(&d, ms + DWM_MS_SUM_LEN, 8); d = d + dacc[cols]; memcpy(ms + DWM_MS_SUM_LEN, &d, 8);
        memcpy(&u, ms + DWM_MS_GAMES, 8); u += k; memcpy(ms + DWM_MS_GAMES, &u, 8);
        ms[DWM_MS_CURRENT_SIZE] = dwm::window_old(k, (uint32_t)max_size, current_size) + dwm::window_new(k, (uint32_t)max_size);
    }
    if (bad > 0u) {
        uint64_t u;
        memcpy(&u, ms + DWM_MS_DISCARDED, 8); u += bad; memcpy(ms + DWM_MS_DISCARDED, &u, 8);
    }
    work[0] = 0u;
    return 0;
}

int dwmh_clear(uint32_t *ms, uint32_t *work) {
    memset(ms, 0, 4 * DWM_MS_WORDS);
    memset(work, 0, 4 * dwm::HEAD);
    return 0;
}

}  // extern "C"
