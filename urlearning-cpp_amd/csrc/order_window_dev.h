// order_window_dev.h -- the arithmetic of the exact window re-optimisation of
// orders (order_window.hip, ulg_order_window; contract: include/ulg.h, "Order
// search"): the width and stride a call uses and a sweep's window starts, the
// squeezed index of a local mask, the LDS bytes of a width, a table word's
// value, one mask of the subset DP, the walk back from the full mask, and the
// serial form of a whole window -- scatter, subset-max, DP, accept -- which
// the check program (host/order_window_check.cpp) holds to a direct evaluation
// of every arrangement.  Host and device, as order_search_dev.h is, whose
// images it reuses.  The kernel calls the same functions per lane.
//
// A window at start a over x_0 .. x_{w-1} with U the variables before it:
//   T_j[squeeze_j(M)]  the image (os_float_image) of beta_j(M) = b_{x_j}(U + V(M)),
//                      j not in M; 0 = -inf.  w 2^(w-1) words.
//   F[M], c[M]         the best sum of an arrangement of V(M) after U and the
//                      local index that stands last in it.
#pragma once

#include "order_search_dev.h"

namespace ulg {

constexpr int kWindowMinWidth = 2, kWindowMaxWidth = 12;
constexpr int64_t kWindowMaxSweeps = 1 << 20;
constexpr int kWindowChunk = 256;       // list entries of one scatter item
constexpr uint8_t kWindowOutside = 255;  // the local bit of a variable that is not in the window

ULG_POST_HD int ow_width(int width, int n) { return width < n ? width : n; }
ULG_POST_HD int ow_stride(int stride, int width, int w) {
    const int s = stride ? stride : (width / 2 > 1 ? width / 2 : 1);
    return s < w ? s : w;
}
// the start after a; the sweep ends with the window at n - w
ULG_POST_HD int ow_next_start(int a, int stride, int n, int w) { return a + stride < n - w ? a + stride : n - w; }

// m without its bit j (which is clear): the index into T_j
ULG_POST_HD uint32_t ow_squeeze(uint32_t m, int j) { return (m & ((1u << j) - 1u)) | ((m >> (j + 1)) << j); }

ULG_POST_HD uint32_t ow_table_words(int w) { return (uint32_t)w << (w - 1); }
// F (8 B a mask), then T, then c (1 B a mask)
ULG_POST_HD size_t ow_lds_bytes(int w) { return ((size_t)8 << w) + (size_t)ow_table_words(w) * 4 + ((size_t)1 << w); }

ULG_POST_HD double ow_beta(uint32_t image) {
    if (!image) return -INFINITY;
    const uint32_t bits = os_float_bits(image);
    float s;
    __builtin_memcpy(&s, &bits, 4);
    return (double)s;
}

// The local mask of the part of S inside the window; bit[u] = the local bit of variable u.
ULG_POST_HD uint32_t ow_local_mask(uint64_t inside, const uint8_t *bit) {
    uint32_t m = 0;
    while (inside) {
        m |= 1u << bit[__builtin_ctzll(inside)];
        inside &= inside - 1;
    }
    return m;
}

// One round of the subset-max over every T_j: pair q of (w 2^(w-2)) of bit r (< w - 1), w >= 2
ULG_POST_HD void ow_butterfly(uint32_t *T, int w, int r, uint32_t q) {
    const uint32_t half = 1u << (w - 1), per = half >> 1;
    const uint32_t j = q >> (w - 2), i = q & (per - 1u);
    const uint32_t lo = (i & ((1u << r) - 1u)) | ((i >> r) << (r + 1));
    uint32_t *t = T + j * half;
    if (t[lo] > t[lo | (1u << r)]) t[lo | (1u << r)] = t[lo];
}

// F[M] and c[M] of a mask M != 0 from the layer below: j in M ascending, one add
// each, the least j among the maxima (the least j of M when all are -inf).
ULG_POST_HD void ow_dp_mask(uint32_t M, int w, const uint32_t *T, double *F, uint8_t *c) {
    const uint32_t half = 1u << (w - 1);
    double best = -INFINITY;
    int at = __builtin_ctz(M);
    for (uint32_t left = M; left; left &= left - 1) {
        const int j = __builtin_ctz(left);
        const uint32_t rest = M & ~(1u << j);
        const double cand = F[rest] + ow_beta(T[(uint32_t)j * half + ow_squeeze(rest, j)]);
        if (cand > best) best = cand, at = j;
    }
    F[M] = best, c[M] = (uint8_t)at;
}

// The walk back from the full mask: var[k], term[k] of window position k.
ULG_POST_HD void ow_backtrack(int w, const uint32_t *T, const uint8_t *c, const uint8_t *xs, uint8_t *var, double *term) {
    const uint32_t half = 1u << (w - 1);
    uint32_t M = (1u << w) - 1u;
    for (int k = w - 1; k >= 0; --k) {
        const int j = c[M];
        M &= ~(1u << j);
        var[k] = xs[j];
        term[k] = ow_beta(T[(uint32_t)j * half + ow_squeeze(M, j)]);
    }
}

// ((0.0 + t_0) + t_1) + ..
ULG_POST_HD double ow_sum(const double *t, int count) {
    double s = 0.0;
    for (int k = 0; k < count; ++k) s = s + t[k];
    return s;
}

// One window, one entry after the other.  order, terms: the whole order and its
// cached terms, rewritten when the window is accepted (the return value).
// T, F, c: ow_lds_bytes(w) of scratch in the kernel's layout.
ULG_POST_HD bool ow_window_serial(const OsHostLists &L, uint8_t *order, double *terms, int a, int w, uint32_t *T, double *F, uint8_t *c) {
    uint8_t bit[64], xs[kWindowMaxWidth], var[kWindowMaxWidth];
    double nt[kWindowMaxWidth];
    uint64_t U = 0, V = 0;
    for (int u = 0; u < 64; ++u) bit[u] = kWindowOutside;
    for (int p = 0; p < a; ++p) U |= 1ull << order[p];
    for (int j = 0; j < w; ++j) xs[j] = order[a + j], bit[xs[j]] = (uint8_t)j, V |= 1ull << xs[j];
    const uint32_t half = 1u << (w - 1);
    for (uint32_t i = 0; i < ow_table_words(w); ++i) T[i] = 0u;
    for (int j = 0; j < w; ++j) {
        const uint64_t allowed = U | (V & ~(1ull << xs[j]));
        for (int64_t i = L.offsets[xs[j]]; i < L.offsets[xs[j] + 1]; ++i) {
            if (L.sets[i] & ~allowed) continue;
            uint32_t bits;
            __builtin_memcpy(&bits, &L.scores[i], 4);
            uint32_t *t = T + (uint32_t)j * half + ow_squeeze(ow_local_mask(L.sets[i] & V, bit), j);
            if (os_float_image(bits) > *t) *t = os_float_image(bits);
        }
    }
    for (int r = 0; r + 1 < w; ++r)
        for (uint32_t q = 0; q < (uint32_t)w * (half >> 1); ++q) ow_butterfly(T, w, r, q);
    F[0] = 0.0, c[0] = 0;
    for (int layer = 1; layer <= w; ++layer)
        for (uint32_t M = 1; M < (1u << w); ++M)
            if (__builtin_popcount(M) == layer) ow_dp_mask(M, w, T, F, c);
    if (!(F[(1u << w) - 1u] > ow_sum(terms + a, w))) return false;
    ow_backtrack(w, T, c, xs, var, nt);
    for (int k = 0; k < w; ++k) order[a + k] = var[k], terms[a + k] = nt[k];
    return true;
}

}  // namespace ulg
