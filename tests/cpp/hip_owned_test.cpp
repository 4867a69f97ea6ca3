// The owners of csrc/hip_owned.h (DevBuf, PinnedBuf, Event, Stream) against a malloc-backed stand-in for the HIP runtime
// (tests/cpp/hip_stub): moves, reserve, failed allocations, idempotent events, order of destruction, the live counters.  No GPU.
#include "../../mrs_multirotor_simulator_amd/csrc/hip_owned.h"

#include <stdio.h>

#include <utility>

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) failures++, printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
  } while (0)

static hip_stub::State& S() { return hip_stub::st(); }
static size_t count(const char* what) {
  size_t n = 0;
  for (auto& l : S().log) n += l == what;
  return n;
}
struct Live {
  long long v[4];
  Live() : v{hip_owned::live_dev.load(), hip_owned::live_pinned.load(), hip_owned::live_events.load(), hip_owned::live_streams.load()} {}
  bool operator==(const Live& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2] && v[3] == o.v[3]; }
};

static void test_moves() {
  const Live start;
  {
    DevBuf<double> a;
    CHECK(a.get() == nullptr && a.capacity() == 0);
    CHECK(a.alloc(10) == hipSuccess && a.get() && a.capacity() == 10 && S().last_bytes == 80);
    double* raw = a;  // implicit conversion
    CHECK(raw == a.get() && a + 3 == raw + 3);
    DevBuf<double> b(std::move(a));
    CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == raw && b.capacity() == 10);
    DevBuf<double> c;
    CHECK(c.alloc(4) == hipSuccess);
    c = std::move(b);  // frees c's own block, takes b's
    CHECK(b.get() == nullptr && b.capacity() == 0 && c.get() == raw && c.capacity() == 10);
    CHECK(count("free") == 1 && hip_owned::live_dev.load() == start.v[0] + 1);
    PinnedBuf<int> p;
    CHECK(p.alloc(3, hipHostMallocMapped) == hipSuccess && S().last_flags == (unsigned)hipHostMallocMapped && S().last_bytes == 12);
    PinnedBuf<int> q(std::move(p));
    CHECK(!p.get() && p.capacity() == 0 && q.get() && q.capacity() == 3);
    Event e;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess);
    Event f(std::move(e));
    CHECK(!e.get() && f.get());
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    Stream t;
    t = std::move(s);
    CHECK(!s.get() && t.get());
  }
  CHECK(count("malloc") == 2 && count("free") == 2 && count("hostmalloc") == 1 && count("hostfree") == 1);
  CHECK(count("event+") == 1 && count("event-") == 1 && count("stream+") == 1 && count("stream-") == 1);
  CHECK(S().live.empty() && S().bad_frees == 0 && Live() == start);
  printf("ok moves\n");
}

static void test_reserve() {
  const Live start;
  S().log.clear();
  {
    DevBuf<void> d;  // counts bytes
    CHECK(d.reserve(100) == hipSuccess && d.capacity() == 100 && S().last_bytes == 100);
    void* first = d;
    CHECK(d.reserve(100) == hipSuccess && d.reserve(7) == hipSuccess && d.reserve(0) == hipSuccess);
    CHECK(d.get() == first && d.capacity() == 100 && S().log.size() == 1);  // nothing happened
    CHECK(d.reserve(101, 3) == hipSuccess && d.capacity() == 101 && S().last_flags == 3u);
    CHECK(S().log.size() == 3 && S().log[1] == "free" && S().log[2] == "malloc");  // frees before it allocates
    CHECK(hip_owned::live_dev.load() == start.v[0] + 1);
    PinnedBuf<double> h;
    CHECK(h.reserve(5) == hipSuccess && h.reserve(5) == hipSuccess && h.reserve(6) == hipSuccess && h.capacity() == 6);
    CHECK(count("hostmalloc") == 2 && count("hostfree") == 1);
    d.reset();
    CHECK(!d.get() && d.capacity() == 0);
    d.reset();  // twice is once
  }
  CHECK(S().live.empty() && S().bad_frees == 0 && Live() == start);
  printf("ok reserve\n");
}

static void test_failed_allocations() {
  const Live start;
  {
    DevBuf<int> d;
    S().allocs = 0, S().fail_alloc_at = 1;
    CHECK(d.alloc(8) != hipSuccess && d.get() == nullptr && d.capacity() == 0);
    CHECK(d.alloc(8) == hipSuccess && d.capacity() == 8);
    S().allocs = 0, S().fail_alloc_at = 1;
    CHECK(d.reserve(8) == hipSuccess && d.capacity() == 8);  // (no allocation, so nothing to fail)
    CHECK(d.reserve(9) != hipSuccess && d.get() == nullptr && d.capacity() == 0);  // the old block is gone, the new one never came
    CHECK(d.reserve(9) == hipSuccess && d.capacity() == 9);
    PinnedBuf<int> h;
    CHECK(h.alloc(2) == hipSuccess);
    S().allocs = 0, S().fail_alloc_at = 1;
    CHECK(h.reserve(3) != hipSuccess && h.get() == nullptr && h.capacity() == 0);
    S().fail_alloc_at = 0;
    CHECK(Live().v[0] == start.v[0] + 1 && Live().v[1] == start.v[1]);
  }
  CHECK(S().live.empty() && S().bad_frees == 0 && Live() == start);
  printf("ok failed_allocations\n");
}

static void test_event_idempotent() {
  const Live start;
  S().log.clear();
  {
    Event e;
    CHECK(e.get() == nullptr);
    CHECK(e.create(hipEventDisableTiming) == hipSuccess);
    hipEvent_t raw = e;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && e.get() == raw);
    CHECK(count("event+") == 1 && hip_owned::live_events.load() == start.v[2] + 1);
    Stream a, b, c;
    const uint32_t mask[2] = {1u, 0u};
    CHECK(a.create(hipStreamNonBlocking) == hipSuccess && b.create_priority(hipStreamNonBlocking, -1) == hipSuccess && c.create_cu_mask(2, mask) == hipSuccess);
    CHECK(hip_owned::live_streams.load() == start.v[3] + 3);
  }
  CHECK(count("event-") == 1 && count("stream+") == 3 && count("stream-") == 3);
  CHECK(S().live.empty() && S().bad_frees == 0 && Live() == start);
  printf("ok event_idempotent\n");
}

// the shape of mrs_swarm: the stream is declared first, so everything that may be in flight on it is released before it
namespace {
struct Holder {
  Stream          stream;
  DevBuf<double>  a;
  PinnedBuf<char> b;
  Event           ev;
};
}  // namespace
static void test_destruction_order() {
  const Live start;
  S().log.clear();
  {
    Holder h;
    CHECK(h.stream.create(hipStreamNonBlocking) == hipSuccess && h.a.alloc(16) == hipSuccess && h.b.alloc(16) == hipSuccess && h.ev.create() == hipSuccess);
    const Live mid;
    for (int k = 0; k < 4; k++) CHECK(mid.v[k] == start.v[k] + 1);
  }
  const std::vector<std::string> want = {"stream+", "malloc", "hostmalloc", "event+", "event-", "hostfree", "free", "stream-"};
  CHECK(S().log == want);  // every allocation freed exactly once, the stream last
  CHECK(S().live.empty() && S().bad_frees == 0 && Live() == start);
  printf("ok destruction_order\n");
}

int main() {
  const Live start;
  test_moves();
  test_reserve();
  test_failed_allocations();
  test_event_idempotent();
  test_destruction_order();
  CHECK(Live() == start && S().live.empty() && S().bad_frees == 0);
  if (failures == 0) printf("ok counters\n");
  return failures ? 1 : 0;
}
