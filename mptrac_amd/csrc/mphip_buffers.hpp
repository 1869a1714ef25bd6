// mphip_buffers.hpp -- the one owner of device memory and of page-locked host memory in the host layer.
//
// A Buffer holds a pointer and the capacity that belongs to it, and nothing else knows that capacity: a swap or a
// move carries both, the destructor frees.  Three ways to get memory, none of which keeps the contents:
//   resize(n)       free, then allocate exactly n elements (n == 0: empty afterwards)
//   reserve(n)      grow only: nothing if n <= capacity, else resize(n)
//   try_reserve(n)  reserve for a caller that has another path: on failure HIP's error is cleared, the buffer is
//                   empty and the answer is false
// resize and reserve return HIP's error for the caller's HIPCHK.  Kernel argument structs take the raw pointer, `p`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace mphip {

struct DeviceMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void *p) { (void) hipFree(p); }
};

struct PinnedMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void *p) { (void) hipHostFree(p); }
};

template <typename T, typename Mem>
struct Buffer {
  T *p = nullptr;
  size_t n = 0;   // capacity in elements

  Buffer() = default;
  Buffer(const Buffer &) = delete;
  Buffer &operator=(const Buffer &) = delete;
  Buffer(Buffer &&o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  Buffer &operator=(Buffer &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~Buffer() { release(); }

  explicit operator bool() const { return p != nullptr; }

  void release() {
    if (p)
      Mem::free(p);
    p = nullptr;
    n = 0;
  }

  hipError_t resize(size_t count) {
    release();
    if (count == 0)
      return hipSuccess;
    const hipError_t e = Mem::alloc((void **) &p, count * sizeof(T));
    if (e != hipSuccess)
      p = nullptr;
    else
      n = count;
    return e;
  }

  hipError_t reserve(size_t count) { return count <= n ? hipSuccess : resize(count); }

  bool try_reserve(size_t count) {
    if (reserve(count) == hipSuccess)
      return true;
    (void) hipGetLastError();
    return false;
  }
};

template <typename T>
using DevBuf = Buffer<T, DeviceMem>;
template <typename T>
using PinnedBuf = Buffer<T, PinnedMem>;

}   // namespace mphip
