// lds_image_check -- the launch images of the cBIC layer kernels on the host
// (csrc/score_plan.h CbicPlan::build_images, option score_lds_image).
//
//   lds_image_check VARIANT CAP MAXP N V:MASK...
//       One scoring call as ulg_cbic_score plans it (score_variant VARIANT,
//       score_unrank_lut CAP, the other options at their defaults) over a
//       Gram matrix of recognisable doubles.  For every layer launch
//       (group, layer, phase) with sets: an image must exist; every region
//       lds_layout names -- Gram matrix, binomials, the launch's work
//       prefixes and unrank offsets, slab offsets, metadata, candidate lists
//       -- must be byte-equal to its source array at the layout's offset;
//       every other byte (alignment gaps, the aliased carve's counters, the
//       offsets' place when the call has no table) must be zero; the size
//       must be lay.stack, a multiple of 16; the images must lie back to back
//       without overlap.  A launch without sets has no image.  Prints
//       "IMG g L ph offset bytes sets aliased" per image for
//       tests/test_lds_image_host.py, which restates which launches exist.
//
// Plain C++17; built with AddressSanitizer + UBSan by `make sanitize`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/score_plan.h"

using namespace ulg;

namespace {

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            std::fprintf(stderr, "lds_image_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

std::vector<uint32_t> table() {
    std::vector<uint32_t> b(64 * kBinomK);
    for (int a = 0; a < 64; ++a)
        for (int k = 0; k < kBinomK; ++k) {
            const uint64_t v = binom64(a, k);
            b[a * kBinomK + k] = v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
        }
    return b;
}

// region [at, at + bytes) of the image equals src; marks it covered
void region(const unsigned char *im, std::vector<char> &covered, int at, const void *src, size_t bytes) {
    CHECK(at >= 0 && (size_t)at + bytes <= covered.size());
    CHECK(std::memcmp(im + at, src, bytes) == 0);
    for (size_t i = 0; i < bytes; ++i) {
        CHECK(!covered[at + i]);  // the layout's regions do not overlap
        covered[at + i] = 1;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: lds_image_check VARIANT CAP MAXP N V:MASK...\n");
        return 2;
    }
    const int variant = std::atoi(argv[1]);
    const long long cap = std::atoll(argv[2]);
    const int maxp = std::atoi(argv[3]), n = std::atoi(argv[4]);
    std::vector<int> vars;
    std::vector<uint64_t> masks;
    for (int a = 5; a < argc; ++a) {
        char *colon = nullptr;
        vars.push_back((int)std::strtol(argv[a], &colon, 10));
        if (!colon || *colon != ':') return 2;
        masks.push_back(std::strtoull(colon + 1, nullptr, 16));
    }
    ScoreLists ls;
    if (ls.build(n, vars.data(), (int)vars.size(), masks.data(), maxp) != ScoreLists::kOk) return 3;
    Options o;
    o.score_variant = variant;
    o.score_unrank_lut = cap;
    CbicPlan p;
    LutCache cache;
    p.build(ls, {}, {}, {}, o, false);
    p.build_luts(ls, cap, cache);
    std::vector<double> gram((size_t)n * n);
    for (size_t i = 0; i < gram.size(); ++i) gram[i] = 1.0 + (double)i / 4096.0;  // no zero byte pattern repeats
    const std::vector<uint32_t> binom = table();

    // off: nothing is built
    p.build_images(ls, gram.data(), binom.data(), false);
    CHECK(!p.image_any && p.image.empty());
    for (int L = 0; L <= p.kmax; ++L)
        for (int ph = 0; ph < 2; ++ph) CHECK(p.image_offset(0, L, ph) < 0);

    p.build_images(ls, gram.data(), binom.data(), true);
    const int nv = p.nv, S = ls.S, top = std::min(p.kmax, kMaxL);
    std::printf("PLAN kmax %d G %d Ls %d Lf %d variant %d vsmall %d lut %d bytes %zu\n", p.kmax, p.G, p.Ls, p.Lf,
                p.variant, p.vsmall, p.lut_any ? 1 : 0, p.image.size());
    CHECK(p.image.size() % 16 == 0);
    int64_t next = 0;  // images lie back to back in launch order
    int images = 0;
    for (int L = 1; L <= p.kmax; ++L)
        for (int ph = 0; ph < 2; ++ph)
            for (int g = 0; g < p.G; ++g) {
                const int64_t at = p.image_offset(g, L, ph);
                const bool layer = L > p.Lf && L <= top && (L > p.Ls || g == 0);
                const uint64_t cnt = !layer ? 0 : (L <= p.Ls ? p.work[p.work_offset(0, L, ph) + nv] : p.launch_count(g, L, ph));
                if (cnt == 0) {
                    CHECK(at < 0);
                    continue;
                }
                CHECK(at == next);
                const int V = L <= p.Ls ? p.vsmall : p.variant;
                CHECK(V == p.launch_variant(L));
                const LdsLayout lay = lds_layout(n, nv, S, L, V);
                const int bytes = p.image_bytes(ls, L);
                CHECK(bytes == lay.stack && bytes % 16 == 0 && at % 16 == 0);
                CHECK((size_t)at + (size_t)bytes <= p.image.size());
                next = at + bytes;
                const bool aliased = lay.gram != 0;
                CHECK(aliased == (ULG_LDS_ALIAS && (V & 208) == 208 && bits_words(L) < 4));
                const unsigned char *im = p.image.data() + at;
                std::vector<char> covered((size_t)bytes, 0);
                const uint64_t *w = L <= p.Ls ? &p.work[p.work_offset(0, L, ph)] : &p.group_work()[p.work_offset(g, L, ph)];
                region(im, covered, lay.gram, gram.data(), (size_t)n * n * 8);
                region(im, covered, lay.binom, binom.data(), binom.size() * 4);
                region(im, covered, lay.work, w, (size_t)(nv + 1) * 8);
                if (p.lut_any) region(im, covered, lay.lutoff, &p.lutoff[p.lut_offset(L, ph)], (size_t)nv * 4);
                region(im, covered, lay.toff, ls.toff.data(), ((size_t)nv * S + 1) * 8);
                region(im, covered, lay.meta, p.meta.data(), (size_t)nv * 16);
                region(im, covered, lay.cand, ls.cand.data(), (size_t)nv * 64);
                size_t zeros = 0;
                for (int i = 0; i < bytes; ++i)
                    if (!covered[i]) {
                        CHECK(im[i] == 0);
                        ++zeros;
                    }
                if (aliased)  // the 16 counter bytes are among the zeros
                    for (int i = 0; i < 16; ++i) CHECK(!covered[lay.cmp + i]);
                std::printf("IMG %d %d %d %lld %d %llu %d %zu\n", g, L, ph, (long long)at, bytes, (unsigned long long)cnt,
                            aliased ? 1 : 0, zeros);
                ++images;
            }
    CHECK((size_t)next == p.image.size());
    CHECK(p.image_any == (images > 0));
    std::printf("lds_image_check ok: %d images\n", images);
    return 0;
}
