// Per-launch HIP event profile behind latte_profile_forward (engine.cpp) and latte_vae_profile_decode / _encode (vae_engine.cpp):
// a mark records an event behind the launch just issued; collect() gives the time since the previous mark to the mark's class.
#pragma once
#include "common.h"

namespace latte {

struct EventProfile {
  std::vector<hipEvent_t> ev;
  std::vector<int> cls;
  EventProfile() = default;
  EventProfile(const EventProfile&) = delete;
  ~EventProfile() { clear(); }   // (an early return of the profiled call leaks nothing)
  void clear() {
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
  }
  void mark(int c, hipStream_t st) {   // the first mark only opens the first interval: give it a negative class (C_NONE, VC_START)
    hipEvent_t e;
    (void)hipEventCreate(&e);
    (void)hipEventRecord(e, st);
    ev.push_back(e);
    cls.push_back(c);
  }
  // After the stream is synchronised: ms_out[c] / launches_out[c] of the classes c in [0, n).  rc: the profiled call's own result --
  // when it failed the outputs are zero and rc comes back.  The events are destroyed either way.
  int collect(const std::string& name, float* ms_out, int* launches_out, int n, int rc = LATTE_OK) {
    for (int i = 0; i < n; ++i) { ms_out[i] = 0.f; launches_out[i] = 0; }
    for (size_t i = 1; !rc && i < ev.size(); ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i - 1], ev[i]) != hipSuccess) rc = fail(LATTE_ERR_HIP, name + ": event");
      else if (cls[i] >= 0 && cls[i] < n) { ms_out[cls[i]] += ms; launches_out[cls[i]] += 1; }
    }
    clear();
    return rc;
  }
};

}  // namespace latte
