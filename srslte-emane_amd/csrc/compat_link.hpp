// Host <-> device traffic of the single-call API (compat.cpp, compat_refsignal.cpp). Every host thread owns a non-blocking stream and a pinned
// bounce arena: a call copies its operands into the arena, queues the copies, the kernels and the copies back on that stream and waits once at
// the end. (hipMemcpy on the callers' pageable buffers costs ~50 us per call and serialises every host thread on the null stream; the
// reference's worker threads - three sf_workers in srsue - call these functions concurrently on distinct objects, SURVEY 8b "Threading".)
// A header, so that tests/link_asan_driver.cpp can compile it alone over stand-ins for the runtime.
#pragma once
#include "dev_buf.hpp"
#include <atomic>
#include <string.h>
#include <vector>

// hidden: one g_link per thread for the library's translation units, and none of this among the library's exported symbols
namespace compat_link __attribute__((visibility("hidden"))) {

// [0] stream waits; [1..3]: compat.cpp (srslte_hip_compat_stats)
inline std::atomic<unsigned long long> g_stats[4];

// Grow-only device staging buffer. Freed with its owner: a state struct behind a caller's object, or the thread for the thread_local ones.
// A thread's locals are destroyed when it ends - the main thread's at exit(), before static destruction - which is when HostLink below
// destroys its stream, so DESIGN.md's caveat about process-lifetime caches (freed after the runtime has gone) does not apply to them.
struct DevStage {
  DevBuf<uint8_t> buf;
  void* get(size_t n)
  {
    if (n > buf.size() && buf.alloc(n)) {
      hip_log("[srslte_hip] hipMalloc(%zu) failed\n", n);
      return nullptr;
    }
    return buf.get();
  }
};

struct HostLink {
  hipStream_t st  = nullptr;
  uint8_t*    pin = nullptr;
  size_t      cap = 0, used = 0;
  struct Back { void* host; const uint8_t* pinned; size_t n; };
  std::vector<Back> back; // device -> host copies queued on the stream: their host-side half happens in flush()
  bool ok = true;
  bool zc = false; // zero-copy regions are out (zc_in / zc_out): a kernel reads or writes the arena itself, so it stays where it is
  hipStream_t stream()
  {
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;
    return st;
  }
  static size_t rounded(size_t n) { return (n + 255) & ~(size_t)255; }
  uint8_t* take(size_t n)
  { // n bytes of the arena; growing it waits for what is queued (the old arena is still being read / written)
    n = rounded(n);
    if (used + n > cap) {
      if (zc) {
        hip_log("[srslte_hip] pinned arena: %zu more bytes do not fit beside zero-copy regions (reserve() the call's whole footprint first)\n", n);
        return nullptr;
      }
      if (!flush()) return nullptr;
      const size_t want = (cap * 2 > n ? cap * 2 : n) + (1u << 20);
      if (pin) (void)hipHostFree(pin);
      pin = nullptr;
      cap = 0;
      if (hipHostMalloc((void**)&pin, want) != hipSuccess) {
        hip_log("[srslte_hip] hipHostMalloc(%zu) failed\n", want);
        return nullptr;
      }
      cap = want;
    }
    uint8_t* p = pin + used;
    used += n;
    return p;
  }
  // room for n more bytes (a sum of rounded() sizes) without growth: a call asks for its whole zero-copy footprint before its first region
  bool reserve(size_t n)
  {
    if (used + n <= cap) return true;
    if (!take(n)) return false;
    used -= n;
    return true;
  }
  // wait for the stream and empty the arena; deliver: hand the results to the caller's buffers (flush), or not (a call that failed)
  bool finish(bool deliver)
  {
    const bool r = (!st || hipStreamSynchronize(st) == hipSuccess) && ok && deliver;
    g_stats[0]++;
    for (const Back& b : back) {
      if (r) memcpy(b.host, b.pinned, b.n);
    }
    back.clear();
    used = 0;
    ok   = true;
    zc   = false;
    return r;
  }
  bool flush() { return finish(true); }
  HostLink() = default;
  HostLink(const HostLink&) = delete;
  HostLink& operator=(const HostLink&) = delete;
  ~HostLink()
  {
    if (st) (void)hipStreamDestroy(st);
    if (pin) (void)hipHostFree(pin);
  }
};
inline thread_local HostLink g_link;

// One per call, at the top of every exported function that uses g_link: whatever path leaves the function, the arena is empty afterwards. A
// call that succeeded has flushed and this does nothing; one that left with operands or copies back still queued waits for the stream (the
// device may still be reading or writing the regions) and drops them, so no later call writes into this call's buffers.
struct LinkScope {
  LinkScope() {}
  LinkScope(const LinkScope&) = delete;
  LinkScope& operator=(const LinkScope&) = delete;
  ~LinkScope()
  {
    if (g_link.used || !g_link.back.empty()) (void)g_link.finish(false);
  }
};

inline bool h2d(void* d, const void* h, size_t n)
{
  if (n == 0) return true;
  uint8_t* p = g_link.take(n);
  if (!p || !g_link.stream()) return false;
  memcpy(p, h, n);
  const bool r = hipMemcpyAsync(d, p, n, hipMemcpyHostToDevice, g_link.st) == hipSuccess;
  g_link.ok    = g_link.ok && r;
  return r;
}
// queues the copy back; the data is in `h` after the next flush (d2h() below does both)
inline bool d2h_later(void* h, const void* d, size_t n)
{
  if (n == 0) return true;
  uint8_t* p = g_link.take(n);
  if (!p || !g_link.stream()) return false;
  const bool r = hipMemcpyAsync(p, d, n, hipMemcpyDeviceToHost, g_link.st) == hipSuccess;
  g_link.ok    = g_link.ok && r;
  if (r) g_link.back.push_back({h, p, n});
  return r;
}
inline bool d2h(void* h, const void* d, size_t n) { return d2h_later(h, d, n) && g_link.flush(); }
// Small operands (a code block: under 1 KB in, 1.5 KB out): the kernel reads and writes the pinned arena itself - device-visible host memory -
// instead of two DMA operations queued around it (each costs more than the kernel: rocprofv3 on phy_dl_test, profiles/r04/dropin_phy_dl_test_trace.txt).
// zc_in: a device-readable copy of h[0, n); zc_out: n device-writable bytes that flush() hands to `h`. Until that flush the arena cannot grow.
inline const uint8_t* zc_in(const void* h, size_t n)
{
  uint8_t* p = g_link.take(n);
  if (!p || !g_link.stream()) return nullptr;
  g_link.zc = true;
  memcpy(p, h, n);
  return p;
}
inline uint8_t* zc_out(void* h, size_t n)
{
  uint8_t* p = g_link.take(n);
  if (!p || !g_link.stream()) return nullptr;
  g_link.zc = true;
  g_link.back.push_back({h, p, n});
  return p;
}

} // namespace compat_link
