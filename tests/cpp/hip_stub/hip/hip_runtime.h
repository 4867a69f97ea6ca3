// Stand-in for <hip/hip_runtime.h> in tests/cpp/hip_owned_test.cpp: the runtime calls csrc/hip_owned.h uses, backed by malloc / free.
// Every handle handed out is entered in a registry; a release of something that is not live is counted as an error, what is still
// live at the end has leaked.  fail_alloc_at = k makes the k-th allocation from now on (device or pinned) fail.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct ihipEvent_t*  hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };

namespace hip_stub {
struct State {
  std::set<void*>          live;          // everything handed out and not yet given back
  std::vector<std::string> log;           // "malloc", "free", "hostmalloc", "hostfree", "event+", "event-", "stream+", "stream-"
  int                      bad_frees = 0; // releases of something that was not live
  int                      fail_alloc_at = 0, allocs = 0;
  unsigned                 last_flags = 0;
  size_t                   last_bytes = 0;
};
inline State& st() {
  static State s;
  return s;
}
inline hipError_t make(void** out, size_t bytes, const char* what, bool is_alloc) {
  State& s = st();
  if (is_alloc && s.fail_alloc_at && ++s.allocs == s.fail_alloc_at) {
    *out = (void*)0x1;  // (a failing call may leave garbage behind: the owner must not keep it)
    return hipErrorOutOfMemory;
  }
  *out = malloc(bytes ? bytes : 1);
  s.live.insert(*out);
  s.log.push_back(what);
  s.last_bytes = bytes;
  return hipSuccess;
}
inline hipError_t drop(void* p, const char* what) {
  State& s = st();
  if (!s.live.erase(p)) return s.bad_frees++, hipErrorInvalidValue;
  free(p);
  s.log.push_back(what);
  return hipSuccess;
}
}  // namespace hip_stub

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_stub::st().last_flags = 0, hip_stub::make(p, bytes, "malloc", true); }
inline hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned flags) { return hip_stub::st().last_flags = flags, hip_stub::make(p, bytes, "malloc", true); }
inline hipError_t hipFree(void* p) { return hip_stub::drop(p, "free"); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) { return hip_stub::st().last_flags = flags, hip_stub::make(p, bytes, "hostmalloc", true); }
inline hipError_t hipHostFree(void* p) { return hip_stub::drop(p, "hostfree"); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { return hip_stub::st().last_flags = flags, hip_stub::make((void**)e, 1, "event+", false); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub::drop(e, "event-"); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hip_stub::make((void**)s, 1, "stream+", false); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return hip_stub::make((void**)s, 1, "stream+", false); }
inline hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) { return hip_stub::make((void**)s, 1, "stream+", false); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_stub::drop(s, "stream-"); }
