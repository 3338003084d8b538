// order_search_dev.h -- the arithmetic of the order-space tabu search
// (order_search.hip, ulg_order_search_*, ulg_order_best; contract:
// include/ulg.h, "Order search"): the order-preserving integer images of a
// score and of a gain, the 64-bit key whose maximum is both the best score and
// its least list index, the gain, the tabu and admissibility rules, and the
// kick's transpositions.  Host and device, as order_mcmc_dev.h is, whose Philox
// draw and proposal it reuses: it compiles under hipcc and under a plain C++
// compiler (host/order_search_check.cpp).  Every path uses these definitions.
#pragma once

#include "order_mcmc_dev.h"

namespace ulg {

constexpr int64_t kSearchMaxTenure = 1 << 20;
constexpr int64_t kSearchMaxPatience = 2147483647;
constexpr int64_t kSearchMaxSteps = 4294967295ll;  // a pair's stamp is the step as 32 bits, 0 = never swapped
constexpr uint8_t kSearchNoMove = 255;             // trace_pos of a step on which nothing moved
constexpr uint32_t kSearchNoEntry = 0xFFFFFFFFu;   // the chosen entry of a term of -inf

// The image of a float's bits under which unsigned order is the floats' order:
// a < b iff image(a) < image(b) for all non-NaN a, b, and -0 takes +0's image
// (they compare equal).  Never 0 for a finite float.
ULG_POST_HD uint32_t os_float_image(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
ULG_POST_HD uint32_t os_float_bits(uint32_t image) { return (image & 0x80000000u) ? image & 0x7FFFFFFFu : ~image; }

// ... and a double's (a gain's); -0 as +0
ULG_POST_HD uint64_t os_double_image(double x) {
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    if (bits == 0x8000000000000000ull) bits = 0ull;
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}

// An entry's key: the score's image above, 2^32 - 1 - (index in the list)
// below.  The maximum of the keys of the compatible entries is the maximal
// score at its least index; 0 stands for "no compatible entry".
ULG_POST_HD uint64_t os_entry_key(uint32_t score_bits, uint32_t index) {
    return ((uint64_t)os_float_image(score_bits) << 32) | (uint64_t)(0xFFFFFFFFu - index);
}

struct OsBest {
    double b;      // (double) of the maximal score, -inf without a compatible entry
    uint32_t ent;  // its least index in the variable's list, or kSearchNoEntry
};
ULG_POST_HD OsBest os_decode(uint64_t key) {
    OsBest r;
    if (!key) {
        r.b = -INFINITY, r.ent = kSearchNoEntry;
        return r;
    }
    const uint32_t bits = os_float_bits((uint32_t)(key >> 32));
    float s;
    __builtin_memcpy(&s, &bits, 4);
    r.b = (double)s, r.ent = 0xFFFFFFFFu - (uint32_t)key;
    return r;
}

// The key of one variable's entries [b, e) under predecessor set U, one entry
// after the other (the check program; the kernels stride the list by lanes
// and reduce across the wave -- a maximum of integers, the same whatever the order).
ULG_POST_HD uint64_t os_best_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U) {
    uint64_t key = 0;
    for (int64_t i = b; i < e; ++i) {
        uint32_t bits;
        __builtin_memcpy(&bits, &scores[i], 4);
        const uint64_t k = os_entry_key(bits, (uint32_t)(i - b));
        if (!(sets[i] & ~U) && k > key) key = k;
    }
    return key;
}

// gain of the swap of positions p, p+1: c0, c1 the terms the two variables
// would have, t0, t1 the terms they have.  Two adds, one subtract; -inf when a
// new term is (the old ones are finite).
ULG_POST_HD double os_gain(double c0, double c1, double t0, double t1) {
    const double now = c0 + c1, was = t0 + t1;
    return now - was;
}

// stamp: the step at which the pair was last swapped, 0 = not since the last clearing
ULG_POST_HD bool os_tabu(uint32_t stamp, int64_t t, int64_t tenure) { return stamp != 0u && (int64_t)stamp >= t - tenure; }

ULG_POST_HD bool os_admissible(double gain, bool tabu, double S, double S_best) {
    if (!(gain > -INFINITY) || !(gain < INFINITY)) return false;
    return !tabu || S + gain > S_best;
}

// a kick's transpositions
ULG_POST_HD int os_kick_count(int n) { return n / 4 > 2 ? n / 4 : 2; }
ULG_POST_HD void os_kick(uint64_t seed, uint64_t t, uint32_t c, int n, uint8_t *order) {  // n >= 2
    const int K = os_kick_count(n);
    for (int k = 0; k < K; ++k) {
        uint32_t w[4];
        mcmc_draw(seed, t, c, (uint32_t)(1 + k), w);
        const McmcMove mv = mcmc_move(w, n);
        const uint8_t x = order[mv.i];
        order[mv.i] = order[mv.j];
        order[mv.j] = x;
    }
}

// A term straight from lists in host memory (the check program's recompute
// beside the cached terms a search keeps)
struct OsHostLists {
    int n;
    const int64_t *offsets;
    const uint64_t *sets;
    const float *scores;
};
ULG_POST_HD OsBest os_term_serial(const OsHostLists &L, int v, uint64_t U) {
    return os_decode(os_best_serial(L.sets, L.scores, L.offsets[v], L.offsets[v + 1], U));
}

}  // namespace ulg
