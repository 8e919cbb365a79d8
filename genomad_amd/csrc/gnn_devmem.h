// The one owner of device and pinned host memory in libgenomad_nn_hip.so.  A buffer has exactly one owner, its capacity travels
// with the pointer and is counted in ELEMENTS of T, and it frees itself.  Nothing here synchronises: a caller that re-allocates
// a buffer a stream may still read synchronises that stream first, at the call site, where the reason can be read.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string>
#include <utility>

#include "../../include/genomad_nn.h"

namespace gnn {

void set_error(const std::string& msg);

template <typename T, bool PINNED>
class Buf {
  public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    // Reads as the pointer it owns: a kernel argument, pointer arithmetic, a null test.  The raw pointer is a VIEW: it is never
    // freed and never stored beyond the buffer's next reserve() / reset() (the views in DeviceWeights point into ctx->owned,
    // which only gnn_destroy releases).
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }

    // Grow-only: nothing happens while capacity() >= n; otherwise the old memory is freed and n + headroom elements are allocated
    // (contents are NOT kept).  Failure leaves the buffer empty, clears the runtime's sticky last error (a caller that retries
    // with a smaller size would otherwise read THIS out-of-memory behind its next, successful kernel launch) and answers
    // GNN_ERR_NOMEM; `what` replaces "hipMalloc of <bytes> bytes" in the message.
    int reserve(size_t n, size_t headroom = 0, const char* what = nullptr) {
        if (p_ && cap_ >= n) return GNN_OK;
        reset();
        const size_t bytes = (n + headroom) * sizeof(T);
        void* q = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error((what ? std::string(what) : std::string(PINNED ? "hipHostMalloc of " : "hipMalloc of ") + std::to_string(bytes) + " bytes") +
                      " failed: " + hipGetErrorString(e));
            return GNN_ERR_NOMEM;
        }
        p_ = static_cast<T*>(q);
        cap_ = n + headroom;
        return GNN_OK;
    }
    // reserve(n) + a synchronous copy of n elements from the host (the weight packs)
    int upload(const T* host, size_t n) {
        if (int rc = reserve(n)) return rc;
        const hipError_t e = hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) return GNN_OK;
        set_error(std::string("hipMemcpy of ") + std::to_string(n * sizeof(T)) + " bytes to the device failed: " + hipGetErrorString(e));
        return GNN_ERR_HIP;
    }
    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    T* release() {          // ownership leaves (gnn_dev_alloc hands the memory to the caller)
        cap_ = 0;
        return std::exchange(p_, nullptr);
    }

  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

}  // namespace gnn
