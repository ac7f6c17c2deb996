// te_devbuf.h -- the one owner of a device allocation (every hipMalloc / hipFree of the shim is in here), and the carving of
// one allocation into typed parts.  The device that holds a buffer must be current wherever it is allocated or freed,
// its destructor included.  Allocation and release never happen inside a captured launch (te_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace te {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }

  // A buffer of at least `n` bytes: kept when it is large enough; otherwise `stream` -- the one whose work may still use
  // the buffer -- is drained, the buffer freed and a new one of `n` bytes allocated (its content is NOT carried over).
  // On failure the object is empty, HIP's sticky last-error slot is cleared and the error returned: the caller words it.
  hipError_t reserve(size_t n, hipStream_t stream) {
    if (p && bytes >= n) return hipSuccess;
    if (p) {
      const hipError_t e = hipStreamSynchronize(stream);
      release();
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
    }
    return once(n);
  }
  // `n` bytes allocated if the object is empty (a buffer whose size never changes while it lives); failure as above
  hipError_t once(size_t n) {
    if (p) return hipSuccess;
    const hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return e;
    }
    bytes = n;
    return hipSuccess;
  }
};

// The parts of one allocation: add<T>(n) registers n elements of T at the next 256-byte boundary, `total` is what to
// allocate, and a part's in(buffer) is its typed pointer, bytes() the size of its n elements.
struct Carve {
  template <class T>
  struct Part {
    size_t off, n;
    T* in(const DevBuf& b) const { return (T*)((char*)b.p + off); }
    size_t bytes() const { return n * sizeof(T); }
  };
  size_t total = 0;
  template <class T>
  Part<T> add(size_t n) {
    const Part<T> s = {total, n};
    total += (n * sizeof(T) + 255) & ~(size_t)255;
    return s;
  }
};

}  // namespace te
