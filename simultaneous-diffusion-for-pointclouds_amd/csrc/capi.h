// Host-side helpers shared by the C entries (extern "C" sdp_* / sdpk_*): the error channel, the status of the
// launches an entry enqueued, workspace layout and the stage-events measurement hook.
#pragma once
#include <cstddef>
#include <string>

#include <hip/hip_runtime.h>

int sdp_fail(const std::string& m);   // net.hip: sets sdp_last_error(), returns -1

namespace sdp {

// the tail of an entry: 0, or "<entry>: <HIP error text>" when one of its launches failed
inline int launch_status(const char* entry) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : sdp_fail(std::string(entry) + ": " + hipGetErrorString(e));
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// bump allocator over the workspace at `base` (0: only count): take() points p at the next 256-byte aligned block
struct Layout {
  uintptr_t base;
  size_t bytes = 0;
  template <class T>
  void take(T*& p, size_t b) {
    p = reinterpret_cast<T*>(base + bytes);
    bytes += align256(b);
  }
};

// Measurement hook of an entry (sdp_*_stage_events): N caller-owned events recorded on the entry's stream between
// its stages.  Per host thread: hold it in a thread_local.
template <int N>
struct StageEvents {
  void* ev[N] = {};
  bool on = false;
  int set(void* const* events, const char* entry) {
    on = false;
    for (int i = 0; i < N; ++i) ev[i] = events ? events[i] : nullptr;
    for (int i = 0; events && i < N; ++i)
      if (!ev[i]) return sdp_fail(std::string(entry) + ": null event");
    on = events != nullptr;
    return 0;
  }
  void mark(int i, hipStream_t st) const {
    if (on) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(ev[i]), st);
  }
};

}  // namespace sdp
