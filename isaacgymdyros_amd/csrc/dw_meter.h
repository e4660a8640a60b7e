// dw_meter.h -- the arithmetic of the episode-return meter (include/dyros_meter.h), written once for the HIP kernels of dw_meter.hip and for
// a g++ build (tests/meter_host.cpp), which the CPU tests hold against a numpy restatement.  Both builds use -ffp-contract=off.
#ifndef DW_METER_H
#define DW_METER_H

#include <stdint.h>
#include <string.h>

#include "../../include/dyros_meter.h"
#include "dw_episode.h"

#if defined(__HIPCC__)
#define DWM_HD __host__ __device__ inline
#else
#define DWM_HD inline
#endif

namespace dwm {

constexpr int GROUP = DWM_GROUP, WAVE = 64, NW = GROUP / WAVE, CMAX = DWM_COLS_MAX, HEAD = DWM_WORK_HEAD;
static_assert(NW == 4, "a partial row is ((w0 + w1) + w2) + w3");
static_assert(DWM_MS_MEAN + DWM_COLS_MAX == DWM_MS_MEAN_LEN && DWM_MS_GAMES % 2 == 0 && DWM_MS_DISCARDED % 2 == 0 && DWM_MS_SUM_RET % 2 == 0 &&
              DWM_MS_SUM_LEN % 2 == 0 && DWM_MS_SUM_LEN + 2 == DWM_MS_WORDS, "ms: the length's mean follows the columns'; 64-bit words are aligned");

using epi::f2u;
using epi::u2f;
DWM_HD bool finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

DWM_HD int groups(int n) { return (n + GROUP - 1) / GROUP; }
// a partial row: cols return sums, the length sum, |D| and the discarded count
DWM_HD int row_words(int cols) { return cols + 3; }
DWM_HD int64_t work_words(int n, int cols) { return (int64_t)HEAD + (int64_t)groups(n) * row_words(cols); }

// one env's column after the step's increment, and what the env keeps
DWM_HD float bump(float cur, float inc) { return cur + inc; }
DWM_HD float keep(float v, bool done) { return done ? 0.0f : v; }
// what an env adds to a sum over D
DWM_HD float term(float v, bool in_d) { return in_d ? v : 0.0f; }

// a workgroup's sum from its wavefronts'
DWM_HD float group_sum(float w0, float w1, float w2, float w3) { return ((w0 + w1) + w2) + w3; }

// AverageMeter.update for one column, k > 0 games whose sum is `total`
DWM_HD uint32_t window_old(uint32_t k, uint32_t max_size, uint32_t current_size) {
    const uint32_t size = k < max_size ? k : max_size, room = max_size - size;
    return room < current_size ? room : current_size;
}
DWM_HD uint32_t window_new(uint32_t k, uint32_t max_size) { return k < max_size ? k : max_size; }
DWM_HD float window_mean(float mean, float total, uint32_t k, uint32_t max_size, uint32_t current_size) {
    const float new_mean = total / (float)k;
    const uint32_t size = window_new(k, max_size), old = window_old(k, max_size, current_size);
    return (mean * (float)old + new_mean * (float)size) / (float)(old + size);
}

}  // namespace dwm

#endif
