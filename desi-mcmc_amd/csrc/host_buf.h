// host_buf.h -- the owner of every device and pinned host allocation of the host side (host code only).
//
// A Buf is a grow-only array: grow(need, alloc, stream) does nothing while `need` elements fit, and otherwise synchronises
// `stream`, frees the old block and allocates `alloc` elements.  The capacity rule stays with the caller.  A failed grow
// leaves the buffer empty (capacity 0) and returns the HIP error, for HIP_TRY.  The destructor frees.
//
// A buffer that is a function's local (a per-call temporary) is freed when the function returns, without a synchronise of
// its own: every path out of such a function has synchronised the stream first (the success paths explicitly, HIP_TRY's
// error path with hipDeviceSynchronize).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

static constexpr unsigned BUF_DEVICE = ~0u;      // Flags of a device buffer; anything else is hipHostMalloc's flags

template <class T, unsigned Flags>
class Buf {
public:
    T *p = nullptr;
    int64_t cap = 0;            // elements

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { reset(); }

    operator T *() const { return p; }
    T *operator->() const { return p; }
    T *get() const { return p; }

    // free now (the caller has synchronised whatever used the block)
    void reset() {
        if (p) (void)(Flags == BUF_DEVICE ? hipFree(p) : hipHostFree(p));
        p = nullptr;
        cap = 0;
    }

    hipError_t grow(int64_t need, int64_t alloc, hipStream_t stream) {
        if (need <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            reset();
        }
        const size_t bytes = sizeof(T) * (size_t)alloc;
        hipError_t e = Flags == BUF_DEVICE ? hipMalloc((void **)&p, bytes) : hipHostMalloc((void **)&p, bytes, Flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = alloc;
        return hipSuccess;
    }
};

template <class T> using DevBuf = Buf<T, BUF_DEVICE>;
template <class T, unsigned Flags = hipHostMallocDefault> using PinnedBuf = Buf<T, Flags>;
template <class T> using MappedBuf = PinnedBuf<T, hipHostMallocMapped | hipHostMallocCoherent>;   // pinned, device-mapped, coherent

// Buffers that are grown together and share ONE capacity test: grow_group(stream, a, na, b, nb, ..., z, nz) synchronises, frees
// every one of them and allocates them again in the order given, each with its own element count.  The caller tests the
// capacity of the one named LAST: a failed allocation leaves every later buffer empty, so that test stays false and the next
// call grows the whole group again.
inline void group_reset() {}
template <class B, class... R> void group_reset(B &b, int64_t, R &...rest) { b.reset(); group_reset(rest...); }
inline hipError_t group_alloc(hipStream_t) { return hipSuccess; }
template <class B, class... R> hipError_t group_alloc(hipStream_t stream, B &b, int64_t n, R &...rest) {
    const hipError_t e = b.grow(n, n, stream);
    return e != hipSuccess ? e : group_alloc(stream, rest...);
}
template <class... A> hipError_t grow_group(hipStream_t stream, A &&...bufs_and_counts) {
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    group_reset(bufs_and_counts...);
    return group_alloc(stream, bufs_and_counts...);
}

// One allocation carved into arrays.  The function that names the arrays runs twice over the same code: with no base, to get
// the arena's size (every pointer comes out null), then with the allocation -- the size and the pointers cannot disagree.
struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t n, size_t align = alignof(T)) {
        off = (off + align - 1) & ~(align - 1);
        T *r = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += sizeof(T) * n;
        return r;
    }
};

// ... in a grow-only buffer: `carve(base)` names the arrays over a Carver{base} and returns its `off`.  The buffer grows with a
// quarter to spare; a failed grow leaves every pointer null.
template <class F> hipError_t carved(DevBuf<char> &buf, hipStream_t stream, F &&carve) {
    const size_t need = carve(static_cast<char *>(nullptr));
    const hipError_t e = buf.grow((int64_t)need, (int64_t)(need + need / 4), stream);
    if (e == hipSuccess) carve(buf.get());
    return e;
}
