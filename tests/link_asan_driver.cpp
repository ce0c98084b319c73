// csrc/compat_link.hpp (the single-call API's per-thread stream, pinned arena and device stages) on the CPU under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_compat_link_sanitizer.py). No HIP library is linked: the few runtime calls the header reaches are
// defined here over malloc / free, with counters and a switch that makes the n-th call of one kind fail, so that ASan sees a write into an
// arena freed through hipHostFree as a heap-use-after-free and every error path can be taken without a device.
#include "compat_link.hpp"
#include <stdarg.h>
#include <stdlib.h>
#include <thread>

using namespace compat_link;

namespace {
enum Kind { HOST_MALLOC, HOST_FREE, DEV_MALLOC, DEV_FREE, STREAM_CREATE, STREAM_DESTROY, STREAM_SYNC, MEMCPY, NKINDS };
std::atomic<int> g_calls[NKINDS];
int              g_fail_kind = -1, g_fail_in = 0; // the g_fail_in-th call of g_fail_kind from now on fails
std::atomic<int> g_log_lines;
// a destination that must hold `watch_pat` by the time pinned memory is freed
const uint8_t* g_watch_dst = nullptr;
uint8_t        g_watch_pat = 0;
int            g_watch_ok  = -1;

bool fails(Kind k)
{ // g_calls counts the calls that went through
  if (g_fail_kind == k && --g_fail_in == 0) return true;
  g_calls[k]++;
  return false;
}
void fail_nth(Kind k, int n) { g_fail_kind = k, g_fail_in = n; }

int g_checks = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    g_checks++;                                                             \
    if (!(cond)) {                                                          \
      printf("check %d failed: %s (line %d)\n", g_checks, #cond, __LINE__); \
      exit(1);                                                              \
    }                                                                       \
  } while (0)

bool all_are(const uint8_t* p, size_t n, uint8_t v)
{
  for (size_t i = 0; i < n; i++) {
    if (p[i] != v) return false;
  }
  return true;
}
bool in_arena(const uint8_t* p, size_t n) { return p >= g_link.pin && p + n <= g_link.pin + g_link.cap; }
} // namespace

void hip_log(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stdout, fmt, ap);
  va_end(ap);
  g_log_lines++;
}

extern "C" {
hipError_t hipHostMalloc(void** p, size_t n, unsigned)
{
  *p = fails(HOST_MALLOC) ? nullptr : malloc(n);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p)
{
  if (p) {
    (void)fails(HOST_FREE);
    if (g_watch_dst) g_watch_ok = all_are(g_watch_dst, 64, g_watch_pat) ? 1 : 0;
  }
  free(p);
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n)
{
  *p = fails(DEV_MALLOC) ? nullptr : malloc(n);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p)
{
  if (p) (void)fails(DEV_FREE);
  free(p);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned)
{
  *s = fails(STREAM_CREATE) ? nullptr : (hipStream_t)malloc(8);
  return *s ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
  (void)fails(STREAM_DESTROY);
  free(s);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return fails(STREAM_SYNC) ? hipErrorUnknown : hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t)
{
  if (fails(MEMCPY)) return hipErrorUnknown;
  memcpy(d, s, n);
  return hipSuccess;
}
}

namespace {

// the shape of srslte_chest_dl_estimate_cfg's tail: three copies back, each refused call ends the function
bool three_copies(void* a, void* b, void* c, const void* dev)
{
  LinkScope scope;
  if (!d2h_later(a, dev, 64) || !d2h_later(b, dev, 64) || !d2h_later(c, dev, 64)) return false;
  return g_link.flush();
}
bool three_copies_into_a_frame(const void* dev)
{
  uint8_t r[64], s[64], t[64];
  memset(r, 0x11, 64);
  const bool ok = three_copies(r, s, t, dev);
  return ok || !all_are(r, 64, 0x11); // false: refused, and r as it was
}

thread_local DevStage g_tl_stage; // an object-less stage, as the demapper's
void worker(bool* ok)
{
  uint8_t in[300], out[300];
  memset(in, 0x77, sizeof(in));
  memset(out, 0, sizeof(out));
  LinkScope scope;
  void*     d = g_tl_stage.get(sizeof(in));
  *ok         = d && h2d(d, in, sizeof(in)) && d2h(out, d, sizeof(out)) && all_are(out, sizeof(out), 0x77);
}

void balance_at_exit()
{ // after the main thread's locals have been destroyed
  const bool ok = g_calls[DEV_MALLOC] == g_calls[DEV_FREE] && g_calls[HOST_MALLOC] == g_calls[HOST_FREE] && g_calls[STREAM_CREATE] == g_calls[STREAM_DESTROY];
  printf("device %d / %d, pinned %d / %d, streams %d / %d\n", g_calls[DEV_MALLOC].load(), g_calls[DEV_FREE].load(), g_calls[HOST_MALLOC].load(),
         g_calls[HOST_FREE].load(), g_calls[STREAM_CREATE].load(), g_calls[STREAM_DESTROY].load());
  if (!ok) {
    printf("allocations and frees do not balance at exit\n");
    fflush(stdout);
    _Exit(1);
  }
  printf("compat link sanitizer run ok: %d checks, balanced at exit\n", g_checks);
}

} // namespace

int main()
{
  atexit(balance_at_exit);
  DevStage dev_stage;
  uint8_t* dev = (uint8_t*)dev_stage.get(4096);
  CHECK(dev != nullptr);
  memset(dev, 0xEE, 4096);

  { // ---- growth with work queued: what is queued is delivered before the old arena goes, and it goes once
    uint8_t src[100], dst[64];
    memset(src, 0xEE, sizeof(src));
    memset(dst, 0, sizeof(dst));
    CHECK(h2d(dev, src, sizeof(src)) && g_calls[HOST_MALLOC] == 1 && g_link.used == 256);
    CHECK(d2h_later(dst, dev, 64) && g_link.back.size() == 1 && all_are(dst, 64, 0));
    const uint8_t* old = g_link.pin;
    g_watch_dst = dst, g_watch_pat = 0xEE;
    uint8_t* p = g_link.take(g_link.cap); // beyond what is left
    g_watch_dst = nullptr;
    CHECK(p != nullptr && g_link.pin != old && p == g_link.pin);
    CHECK(g_watch_ok == 1 && all_are(dst, 64, 0xEE));                 // delivered when the old arena was freed
    CHECK(g_calls[HOST_FREE] == 1 && g_calls[HOST_MALLOC] == 2);      // freed once
    CHECK(g_link.back.empty() && g_link.flush() && g_link.used == 0); // and not delivered again
  }

  { // ---- zero-copy regions from one reservation, on an arena with one 256-byte unit left
    uint8_t in[768], par[1537], tail[1];
    memset(in, 0x42, sizeof(in));
    memset(par, 0, sizeof(par));
    tail[0] = 0;
    CHECK(g_link.take(g_link.cap - 256) && g_link.cap - g_link.used == 256);
    const int mallocs = g_calls[HOST_MALLOC], frees = g_calls[HOST_FREE];
    CHECK(g_link.reserve(HostLink::rounded(sizeof(in)) + HostLink::rounded(sizeof(par)) + HostLink::rounded(1)));
    CHECK(g_calls[HOST_MALLOC] == mallocs + 1 && g_calls[HOST_FREE] == frees + 1); // grown before any region is out
    const uint8_t* di    = zc_in(in, sizeof(in));
    uint8_t *      dpar  = zc_out(par, sizeof(par)), *dtail = zc_out(tail, 1);
    CHECK(di && dpar && dtail && g_calls[HOST_MALLOC] == mallocs + 1 && g_calls[HOST_FREE] == frees + 1);
    CHECK(in_arena(di, sizeof(in)) && in_arena(dpar, sizeof(par)) && in_arena(dtail, 1) && all_are(di, sizeof(in), 0x42));
    memset((void*)di, 0x43, sizeof(in)); // the kernel's side: all three are still memory
    memset(dpar, 0x44, sizeof(par));
    dtail[0] = 0x45;
    const int lines = g_log_lines;
    CHECK(g_link.take(g_link.cap) == nullptr && g_log_lines == lines + 1);          // would have to grow under them: refused, one line
    CHECK(g_calls[HOST_MALLOC] == mallocs + 1 && g_calls[HOST_FREE] == frees + 1); // nothing freed
    CHECK(g_link.flush() && all_are(par, sizeof(par), 0x44) && tail[0] == 0x45 && g_link.used == 0 && !g_link.zc);
    CHECK(g_link.take(g_link.cap + 1) != nullptr && g_link.flush()); // with none outstanding the arena grows again
  }

  { // ---- a failed call leaves nothing: the second of three copies back is refused
    uint8_t* heap = (uint8_t*)malloc(64);
    uint8_t  s[64], t[64];
    memset(heap, 0x22, 64);
    fail_nth(MEMCPY, 2);
    CHECK(!three_copies(heap, s, t, dev));
    CHECK(g_link.used == 0 && g_link.back.empty() && all_are(heap, 64, 0x22));
    free(heap);
    fail_nth(MEMCPY, 2);
    CHECK(!three_copies_into_a_frame(dev));
    CHECK(g_link.used == 0 && g_link.back.empty());
    uint8_t a[64] = {0}, b[64] = {0}, c[64] = {0};
    CHECK(three_copies(a, b, c, dev) && all_are(a, 64, 0xEE) && all_are(b, 64, 0xEE) && all_are(c, 64, 0xEE)); // its own bytes, nobody else's
  }

  { // ---- the stream wait fails: nothing is delivered, the state is reset
    uint8_t dst[64];
    memset(dst, 0x33, 64);
    CHECK(d2h_later(dst, dev, 64));
    fail_nth(STREAM_SYNC, 1);
    CHECK(!g_link.flush() && all_are(dst, 64, 0x33));
    CHECK(g_link.used == 0 && g_link.back.empty() && g_link.ok);
    CHECK(d2h(dst, dev, 64) && all_are(dst, 64, 0xEE));
  }

  { // ---- the grow-only stage
    DevStage  s;
    const int mallocs = g_calls[DEV_MALLOC], frees = g_calls[DEV_FREE];
    void*     p = s.get(1000);
    CHECK(p && s.get(1000) == p && s.get(10) == p && g_calls[DEV_MALLOC] == mallocs + 1);
    void* q = s.get(1001);
    CHECK(q && q != p && g_calls[DEV_MALLOC] == mallocs + 2 && g_calls[DEV_FREE] == frees + 1);
    fail_nth(DEV_MALLOC, 1);
    CHECK(s.get(5000) == nullptr && s.buf.size() == 0 && g_calls[DEV_FREE] == frees + 2); // nothing held after a failure
  }

  { // ---- a worker thread that ends takes its stream, arena and stage with it
    const int before[6] = {g_calls[DEV_MALLOC], g_calls[DEV_FREE], g_calls[HOST_MALLOC], g_calls[HOST_FREE], g_calls[STREAM_CREATE], g_calls[STREAM_DESTROY]};
    bool      ok = false;
    std::thread th(worker, &ok);
    th.join();
    CHECK(ok);
    CHECK(g_calls[DEV_MALLOC] - before[0] == 1 && g_calls[DEV_FREE] - before[1] == 1);
    CHECK(g_calls[HOST_MALLOC] - before[2] == 1 && g_calls[HOST_FREE] - before[3] == 1);
    CHECK(g_calls[STREAM_CREATE] - before[4] == 1 && g_calls[STREAM_DESTROY] - before[5] == 1);
  }
  printf("compat link cases done: %d checks\n", g_checks);
  return 0;
}
