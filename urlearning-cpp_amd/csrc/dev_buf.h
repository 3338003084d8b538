// dev_buf.h -- device and pinned host buffers that own their memory.
// Host-only (no HIP header): the memory comes from the functions declared
// below, which ulg_ctx.cpp defines over HIP and host/devbuf_check.cpp over
// malloc.  A buffer frees itself when it goes out of scope, so neither a
// context, a state struct nor an early return keeps a list of what to free.
#pragma once

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ulg.h"

namespace ulg {

// Each returns the HIP status (0: success).  `bytes` of a free is what the
// block was allocated with: the process-wide live counts (ulg_get_info
// "device_bytes_live" / "pinned_bytes_live") go up by it and down by it.
int dev_alloc(void **p, size_t bytes);
int dev_free(void *p, size_t bytes);
int pinned_alloc(void **p, size_t bytes);
int pinned_free(void *p, size_t bytes);
// sets "<call> failed: <the status's text>", returns ULG_ERR_HIP
int alloc_failed(ulg_ctx *c, const char *call, int status);
// host -> device copy on the context's stream; sets the error text on failure
int dev_upload(ulg_ctx *c, void *dst, const void *src, size_t bytes);

// Buffer that only grows (ensure), move-only, freed by its destructor.
template <typename T, bool kPinned>
struct Buf {
    // 16 bytes of slack on the device: kernels read whole 16-byte chunks (the
    // uint4 key loads of walk_bucket_count_kernel, cbic_walk.hip), so the last
    // chunk of an array may read up to 15 bytes past its end
    static constexpr size_t kSlack = kPinned ? 0 : 16;

    T *p = nullptr;
    size_t cap = 0;  // elements

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    void reset() {
        if (p) (void)(kPinned ? pinned_free(p, cap * sizeof(T) + kSlack) : dev_free(p, cap * sizeof(T) + kSlack));
        p = nullptr;
        cap = 0;
    }
    // Frees what it holds, then allocates `elems`; returns the HIP status and
    // stays empty when the allocation fails.
    int alloc(size_t elems) {
        reset();
        void *q = nullptr;
        const size_t bytes = elems * sizeof(T) + kSlack;
        if (int e = kPinned ? pinned_alloc(&q, bytes) : dev_alloc(&q, bytes)) return e;
        p = static_cast<T *>(q);
        cap = elems;
        return 0;
    }
};
template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using PinnedBuf = Buf<T, true>;

template <typename T, bool kPinned>
int ensure(ulg_ctx *c, Buf<T, kPinned> &b, size_t elems) {
    if (elems == 0) elems = 1;
    if (b.cap >= elems) return ULG_OK;
    if (int e = b.alloc(elems)) return alloc_failed(c, kPinned ? "hipHostMalloc" : "hipMalloc", e);
    return ULG_OK;
}

// Host copy of what was last uploaded into a device buffer: repeated calls
// with the same layout metadata skip the pageable H2D copies.
struct Mirror {
    const void *dev = nullptr;
    std::vector<unsigned char> bytes;
};

template <typename T>
int upload(ulg_ctx *c, DevBuf<T> &b, Mirror &m, const std::vector<T> &h) {
    const size_t nbytes = h.size() * sizeof(T);
    if (int rc = ensure(c, b, h.size())) return rc;
    if (m.dev == b.p && m.bytes.size() == nbytes && std::memcmp(m.bytes.data(), h.data(), nbytes) == 0) return ULG_OK;
    if (int rc = dev_upload(c, b.p, h.data(), nbytes)) return rc;
    m.dev = b.p;
    m.bytes.assign(reinterpret_cast<const unsigned char *>(h.data()),
                   reinterpret_cast<const unsigned char *>(h.data()) + nbytes);
    return ULG_OK;
}

}  // namespace ulg
