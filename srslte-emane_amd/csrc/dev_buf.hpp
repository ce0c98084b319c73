// Owners of the objects' device and pinned memory (the pipelines of pdsch.hip, the control and auxiliary modules): an object struct holds
// these, and destroying the object is `delete`.
// None prints: a constructor reports a failed one with its module's own "device allocation failed" / "initialisation failed" line.
#pragma once
#include "common.hpp"
#include "pinned_ring.hpp"
#include <utility>
#include <vector>

// One hipMalloc block of n elements of T
template <typename T> class DevBuf
{
public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    std::swap(p_, o.p_), std::swap(n_, o.n_);
    return *this;
  }
  ~DevBuf() { (void)hipFree(p_); }

  int alloc(size_t n)
  {
    (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
    if (hipMalloc((void**)&p_, sizeof(T) * n) != hipSuccess) return SRSLTE_ERROR;
    n_ = n;
    return SRSLTE_SUCCESS;
  }
  // allocate and copy, synchronously; nothing is held after a failure
  int upload(const T* h, size_t n)
  {
    if (alloc(n)) return SRSLTE_ERROR;
    if (hipMemcpy(p_, h, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess) return SRSLTE_SUCCESS;
    (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
    return SRSLTE_ERROR;
  }
  int upload(const std::vector<T>& h) { return upload(h.data(), h.size()); }

  T*     get() const { return p_; }
  size_t size() const { return n_; }
  // reads like the raw pointer it replaces: a launch argument, pointer arithmetic, a test for "present". Not copyable, so handing the owner
  // itself to a kernel by value does not compile. get() where a cast changes the pointee type
  operator T*() const { return p_; }

private:
  T*     p_ = nullptr;
  size_t n_ = 0;
};

// One hipHostMalloc block of `bytes` bytes
class PinBuf
{
public:
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { (void)hipHostFree(p_); }
  int      alloc(size_t bytes) { return hipHostMalloc((void**)&p_, bytes) == hipSuccess ? SRSLTE_SUCCESS : SRSLTE_ERROR; }
  uint8_t* get() const { return p_; }
  operator uint8_t*() const { return p_; }

private:
  uint8_t* p_ = nullptr;
};

// A call's descriptors on their way to the device: the pinned ring they are built in and the device block the kernels read them from.
//   D* h; begin(&h); fill h[0..n); commit(sizeof(D) * n, st); launch with dev<D>()
// Where a kernel of the call reads the pinned buffer itself and writes the device block (dev_bytes()), that launch stands for the copy:
//   begin(&h); fill; the caller's launch on st; committed(st)
struct DescStage {
  int init(size_t bytes)
  {
    if (dev_.alloc(bytes)) return SRSLTE_ERROR;
    return ring_.init(bytes);
  }
  // the next pinned buffer, once the copy that last read it has completed
  template <typename D> int begin(D** h)
  {
    if (int r = ring_.acquire(&pin_)) return r;
    *h = reinterpret_cast<D*>(pin_);
    return SRSLTE_SUCCESS;
  }
  // queues the copy of the first `bytes` of the buffer begin() handed out to the device block on st
  int commit(size_t bytes, hipStream_t st)
  {
    HIP_TRY(hipMemcpyAsync(dev_.get(), pin_, bytes, hipMemcpyHostToDevice, st));
    return ring_.release(st);
  }
  // the kernel-read variant: what st holds so far is the last reader of the buffer begin() handed out
  int committed(hipStream_t st) { return ring_.release(st); }
  uint8_t* dev_bytes() const { return dev_.get(); }
  template <typename D> const D* dev() const { return reinterpret_cast<const D*>(dev_.get()); }

  DescStage() = default;
  DescStage(const DescStage&) = delete;
  DescStage& operator=(const DescStage&) = delete;
  ~DescStage() { ring_.destroy(); } // leaves alone what init() did not get to

private:
  PinnedRing      ring_;
  DevBuf<uint8_t> dev_;
  uint8_t*        pin_ = nullptr; // the buffer of the begin() under way
};
