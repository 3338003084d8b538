// devbuf_check -- the owning buffers of csrc/dev_buf.h (DevBuf, PinnedBuf,
// ensure, upload) over malloc/free instead of HIP: this program defines the
// header's allocation functions itself, with live-byte and call counters and a
// switch that makes the next allocation fail.  Every case ends with nothing
// live.  Built with AddressSanitizer + UBSan by `make sanitize`
// (tests/test_sanitize.py); LeakSanitizer checks the exit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/dev_buf.h"

struct ulg_ctx {
    std::string err;
};

namespace {

struct Counters {
    long long live = 0;  // bytes
    int allocs = 0, frees = 0;
};
Counters g_dev, g_pin;
bool g_fail_next = false;
int g_uploads = 0;
constexpr int kStatusOom = 2;  // hipErrorOutOfMemory

int fake_alloc(Counters &k, void **p, size_t bytes) {
    if (g_fail_next) {
        g_fail_next = false;
        *p = nullptr;
        return kStatusOom;
    }
    *p = std::malloc(bytes);
    std::memset(*p, 0xA5, bytes);  // the whole block is addressable, slack included
    k.live += (long long)bytes;
    ++k.allocs;
    return 0;
}
int fake_free(Counters &k, void *p, size_t bytes) {
    std::free(p);
    k.live -= (long long)bytes;
    ++k.frees;
    return 0;
}

}  // namespace

namespace ulg {
int dev_alloc(void **p, size_t bytes) { return fake_alloc(g_dev, p, bytes); }
int dev_free(void *p, size_t bytes) { return fake_free(g_dev, p, bytes); }
int pinned_alloc(void **p, size_t bytes) { return fake_alloc(g_pin, p, bytes); }
int pinned_free(void *p, size_t bytes) { return fake_free(g_pin, p, bytes); }
int alloc_failed(ulg_ctx *c, const char *call, int status) {
    c->err = std::string(call) + " failed: status " + std::to_string(status);
    return ULG_ERR_HIP;
}
int dev_upload(ulg_ctx *, void *dst, const void *src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    ++g_uploads;
    return ULG_OK;
}
}  // namespace ulg

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        ++g_checks;                                                                          \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "devbuf_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

// the cases run once per kind of buffer; kSlack is the only difference
template <template <typename> class B>
void check_buffer(Counters &k, const char *call) {
    constexpr long long slack = (long long)B<double>::kSlack;
    ulg_ctx c;
    CHECK(k.live == 0);
    {
        // only-grow, and the slack behind the elements
        B<double> b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(ensure(&c, b, 10) == ULG_OK && b.cap == 10 && b.p);
        CHECK(k.live == 10 * 8 + slack);
        double *first = b.p;
        CHECK(ensure(&c, b, 10) == ULG_OK && ensure(&c, b, 3) == ULG_OK && ensure(&c, b, 0) == ULG_OK);
        CHECK(b.p == first && b.cap == 10 && k.allocs == 1 && k.frees == 0);
        CHECK(ensure(&c, b, 11) == ULG_OK && b.cap == 11);
        CHECK(k.allocs == 2 && k.frees == 1 && k.live == 11 * 8 + slack);  // the old block went first
        b.p[10] = 1.0;
        reinterpret_cast<unsigned char *>(b.p)[11 * 8 + slack - 1] = 0;  // last byte of the slack
        // a failed growth: empty, the old block freed, the message set
        g_fail_next = true;
        CHECK(ensure(&c, b, 100) == ULG_ERR_HIP);
        CHECK(b.p == nullptr && b.cap == 0 && k.live == 0 && k.frees == 2);
        CHECK(c.err == std::string(call) + " failed: status 2");
        // ... and the buffer works again afterwards
        CHECK(ensure(&c, b, 0) == ULG_OK && b.cap == 1 && k.live == 8 + slack);
        // reset() twice
        b.reset();
        CHECK(b.p == nullptr && b.cap == 0 && k.live == 0);
        b.reset();
        CHECK(k.live == 0 && k.allocs == k.frees);
    }
    {
        // move construction, move assignment, self-move: one owner each time
        B<int> a;
        CHECK(ensure(&c, a, 5) == ULG_OK);
        int *pa = a.p;
        B<int> m(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && m.p == pa && m.cap == 5 && k.live == 5 * 4 + slack);
        B<int> t;
        CHECK(ensure(&c, t, 7) == ULG_OK);
        const int frees = k.frees;
        t = std::move(m);  // t's own block is freed, m's moves in
        CHECK(k.frees == frees + 1 && t.p == pa && t.cap == 5 && m.p == nullptr && m.cap == 0);
        CHECK(k.live == 5 * 4 + slack);
        B<int> &self = t;
        t = std::move(self);
        CHECK(t.p == pa && t.cap == 5 && k.frees == frees + 1 && k.live == 5 * 4 + slack);
        a = std::move(m);  // empty into empty
        CHECK(a.p == nullptr && k.live == 5 * 4 + slack);
    }
    CHECK(k.live == 0 && k.allocs == k.frees);
    {
        // a struct of buffers destroyed in a scope, as the context and its states are
        struct State {
            B<double> x, y;
            B<unsigned char> z;
            std::vector<B<float>> more;
        };
        State *s = new State();
        CHECK(ensure(&c, s->x, 100) == ULG_OK && ensure(&c, s->z, 3) == ULG_OK);
        s->more.resize(4);
        for (size_t i = 0; i < s->more.size(); ++i) CHECK(ensure(&c, s->more[i], i + 1) == ULG_OK);
        s->more.resize(9);  // relocation moves the buffers
        CHECK(k.live == 100 * 8 + 3 + (1 + 2 + 3 + 4) * 4 + 6 * slack);
        delete s;
        CHECK(k.live == 0 && k.allocs == k.frees);
    }
    {
        // an early return between two ensures (the second allocation fails)
        auto early = [&](bool fail_second) -> int {
            B<double> first;
            B<int> second;
            if (int rc = ensure(&c, first, 8)) return rc;
            g_fail_next = fail_second;
            if (int rc = ensure(&c, second, 8)) return rc;
            return ULG_OK;
        };
        CHECK(early(true) == ULG_ERR_HIP && k.live == 0 && k.allocs == k.frees);
        CHECK(early(false) == ULG_OK && k.live == 0 && k.allocs == k.frees);
    }
}

void check_upload() {
    ulg_ctx c;
    DevBuf<int> b;
    Mirror m;
    std::vector<int> h = {1, 2, 3};
    CHECK(upload(&c, b, m, h) == ULG_OK && g_uploads == 1 && std::memcmp(b.p, h.data(), 12) == 0);
    CHECK(upload(&c, b, m, h) == ULG_OK && g_uploads == 1);  // same bytes, same block: no copy
    h[1] = 7;
    CHECK(upload(&c, b, m, h) == ULG_OK && g_uploads == 2 && b.p[1] == 7);
    h.assign(50, 4);  // the buffer grows: a new block is never taken for the mirrored one's bytes
    CHECK(upload(&c, b, m, h) == ULG_OK && g_uploads == 3 && b.cap == 50 && b.p[49] == 4);
    g_fail_next = true;
    h.assign(500, 4);
    CHECK(upload(&c, b, m, h) == ULG_ERR_HIP && g_uploads == 3 && b.p == nullptr);
}

}  // namespace

int main() {
    check_buffer<DevBuf>(g_dev, "hipMalloc");
    CHECK(DevBuf<char>::kSlack == 16 && PinnedBuf<char>::kSlack == 0);
    check_buffer<PinnedBuf>(g_pin, "hipHostMalloc");
    CHECK(g_pin.live == 0 && g_dev.allocs > 0 && g_pin.allocs == g_dev.allocs);
    check_upload();
    CHECK(g_dev.live == 0 && g_dev.allocs == g_dev.frees && g_pin.live == 0 && g_pin.allocs == g_pin.frees);
    std::printf("devbuf_check ok: %ld checks\n", g_checks);
    return 0;
}
