// Owners of the library's host-side GPU resources (host code only; included by rda_hip.hip after include/rda_hip.h).
// Every device or pinned allocation of the library is made by Group::dev / Group::pin: zero-filled, counted, and on failure
// RDA_ERR_HIP with the caller's view left as it was.  A failed call drops its local Group and so leaks nothing; a call that
// replaces buffers of a handle builds the new Group beside the old one and moves it in only once everything has succeeded.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

namespace hbuf {
inline std::atomic<long long> live_allocs{0}, live_bytes{0};    // what the library holds now (rda_debug_alloc_stats)
inline thread_local long long refuse_in = -1;                   // this thread's allocations to grant before one is refused (rda_debug_alloc_fail; < 0: none)

template <bool PINNED> class Mem {          // one device (or pinned host) allocation, move-only
public:
    Mem() = default;
    Mem(Mem &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Mem &operator=(Mem &&o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
    ~Mem()
    {
        if (!p_) return;
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        live_allocs -= 1; live_bytes -= (long long)bytes_;
    }
    int alloc(size_t bytes)                 // (an empty owner)
    {
        if (refuse_in >= 0 && refuse_in-- == 0) return RDA_ERR_HIP;           // before HIP is asked: the card never runs short
        const hipError_t e = PINNED ? hipHostMalloc(&p_, bytes) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; fprintf(stderr, "librda_hip: %s of %zu bytes failed: %s\n", PINNED ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e)); return RDA_ERR_HIP; }
        if (!p_) return RDA_OK;                                                // (0 bytes)
        bytes_ = bytes; live_allocs += 1; live_bytes += (long long)bytes;
        if (PINNED) memset(p_, 0, bytes);
        else if (hipMemset(p_, 0, bytes) != hipSuccess) return RDA_ERR_HIP;   // (the destructor frees it)
        return RDA_OK;
    }
    void *get() const { return p_; }
private:
    void *p_ = nullptr; size_t bytes_ = 0;
};

struct Group {                              // buffers that live and die together
    std::vector<Mem<false>> d; std::vector<Mem<true>> h;
    template <typename T> int dev(T **view, size_t n) { return add(d, view, n); }    // n T on the device
    template <typename T> int pin(T **view, size_t n) { return add(h, view, n); }    // n T in pinned host memory
private:
    template <typename M, typename T> static int add(std::vector<M> &v, T **view, size_t n)
    {
        M m;
        if (int rc = m.alloc(n * sizeof(T))) return rc;
        *view = (T *)m.get(); v.push_back(std::move(m));
        return RDA_OK;
    }
};

template <typename T> struct Pair {          // n T on the device and their pinned mirror: views into the Group that owns both
    T *h = nullptr, *d = nullptr; size_t n = 0;
    int alloc(Group &g, size_t count) { const int rc = g.dev(&d, count) | g.pin(&h, count); n = rc ? 0 : count; return rc; }     // (refused: n stays 0)
    hipError_t push(hipStream_t s) const { return hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s); }                        // all of the mirror
    hipError_t upload(const T *src, hipStream_t s) const { memcpy((void *)h, src, n * sizeof(T)); return push(s); }                      // n T of the caller's -> mirror -> device
    hipError_t pull(hipStream_t s, size_t count) const { return hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, s); }      // the first count
};

template <typename Hd, hipError_t (*Destroy)(Hd)> class Res {     // a stream or an event, move-only
public:
    Res() = default;
    Res(Res &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Res &operator=(Res &&o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Res() { if (h_) (void)Destroy(h_); }
    operator Hd() const { return h_; }
    Hd *out() { return &h_; }                       // where the create call writes (an empty owner)
private:
    Hd h_ = nullptr;
};
inline hipError_t stream_destroy(hipStream_t s) { (void)hipStreamSynchronize(s); return hipStreamDestroy(s); }     // nothing queued outlives its stream
using Stream = Res<hipStream_t, stream_destroy>;
using Event = Res<hipEvent_t, hipEventDestroy>;
}   // namespace hbuf
