// The pinned host buffers that carry a call's descriptors to the device: the ring inside DescStage (dev_buf.hpp) and of the channel emulator
// (channel.hip).
#pragma once
#include "common.hpp"

// A call's descriptors are built in one of four pinned host buffers and copied asynchronously: the host does not wait for the stream, only,
// four calls later, for the copy that last read the buffer it takes
struct PinnedRing {
  uint8_t*   pin[4]  = {};
  hipEvent_t ev[4]   = {};
  bool       used[4] = {};
  uint32_t   next = 0, cur = 0;
  int init(size_t bytes)
  {
    for (int i = 0; i < 4; i++) {
      HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
      HIP_TRY(hipHostMalloc((void**)&pin[i], bytes));
    }
    return SRSLTE_SUCCESS;
  }
  // the next buffer, once the copy that last read it has completed
  int acquire(uint8_t** h)
  {
    cur = next++ & 3u;
    if (used[cur]) HIP_TRY(hipEventSynchronize(ev[cur]));
    *h = pin[cur];
    return SRSLTE_SUCCESS;
  }
  // the acquired buffer is free again when what st holds so far (the copy that reads it among it) has run
  int release(hipStream_t st)
  {
    HIP_TRY(hipEventRecord(ev[cur], st));
    used[cur] = true;
    return SRSLTE_SUCCESS;
  }
  void destroy()
  {
    for (int i = 0; i < 4; i++) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]); // also when the allocation right after its creation failed
    }
  }
};
