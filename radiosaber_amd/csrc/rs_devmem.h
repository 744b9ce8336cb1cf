/*
 * rs_devmem.h -- the device memory a batch owns (rs_api.cpp), host only (never embedded for hiprtc): one hipMalloc block per DevBuf,
 * which knows its size and frees itself, and the all-or-none allocation of several of them.  Calls the HIP runtime directly;
 * tests/csrc/devmem_check.cpp links it against a runtime of its own that counts the live blocks and fails on demand.
 */
#ifndef RS_DEVMEM_H_
#define RS_DEVMEM_H_

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <utility>

/* `count` elements of T in device memory, or nothing (null, 0).  Converts to T* wherever a pointer is read. */
template <typename T>
class DevBuf {
  T* p_ = nullptr;
  size_t n_ = 0;

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DevBuf() { release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t count() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }

  /* for the callers that must give the memory back BEFORE they ask for more (the CQI grids, the record block) */
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  /* A block of `count` elements in place of the present one.  The new block first, the old one freed only once it exists: a failure
   * leaves the buffer as it was.  (count 0: a block of one byte -- the pointer says "set", the size says "nothing to copy".) */
  hipError_t alloc(size_t count) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, count ? count * sizeof(T) : 1);
    if (e != hipSuccess) return e;
    release();
    p_ = (T*)q;
    n_ = count;
    return hipSuccess;
  }
  /* the whole buffer from / to `count()` elements of host memory, and all zero bytes */
  hipError_t upload(const void* host) { return n_ ? hipMemcpy(p_, host, bytes(), hipMemcpyHostToDevice) : hipSuccess; }
  hipError_t download(void* host) const { return n_ ? hipMemcpy(host, p_, bytes(), hipMemcpyDeviceToHost) : hipSuccess; }
  hipError_t zero() { return n_ ? hipMemset(p_, 0, bytes()) : hipSuccess; }
  /* alloc(count), then upload(host) / then zero() */
  hipError_t assign(const T* host, size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : upload(host);
  }
  hipError_t alloc_zeroed(size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : zero();
  }
};

/* Several buffers, every one or none: dev_alloc_all(a, na, b, nb, ...) allocates a block of n elements for each buffer into a temporary
 * and commits them on the way back, once the last one exists (a commit is two moves: it cannot fail).  A failure at the k-th block
 * frees the k - 1 new ones and leaves every buffer as it was. */
inline hipError_t dev_alloc_all() { return hipSuccess; }
template <typename T, typename... Rest>
hipError_t dev_alloc_all(DevBuf<T>& buf, size_t count, Rest&&... rest) {
  DevBuf<T> fresh;
  hipError_t e = fresh.alloc(count);
  if (e == hipSuccess) e = dev_alloc_all(std::forward<Rest>(rest)...);
  if (e == hipSuccess) buf = std::move(fresh);
  return e;
}

#endif /* RS_DEVMEM_H_ */
