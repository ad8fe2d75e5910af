// ctd_api.hip -- what of the extern "C" surface belongs to no kernel family: the ABI version, the status strings and
// the per-thread kernel-timing state behind ctd_kernel_timing_* (include/ctd_hip_bench.h).  Every other entry point of
// include/ctd_hip.h lives, with its argument validation, in the file of the kernels it launches.
#include "ctd_internal.h"
#include "../../include/ctd_hip_bench.h"

#include <deque>
#include <utility>
#include <vector>

using namespace ctd;

namespace ctd {
// Bench instrumentation (include/ctd_hip_bench.h, ctd_kernel_timing_*): NOT part of the drop-in ABI of
// include/ctd_hip.h.  The state is per calling thread (thread_local): the thread that enables it sees its own launches
// only, other threads of the process launch un-instrumented and race with nothing.
// The events come from a pool created when timing is switched on (no hipEventCreate between launches) and carry
// hipEventDisableSystemFence: a default event makes the queue release to system scope at every record (an L2
// write-back of whatever the previous kernel left dirty), which the un-instrumented path never pays.
static thread_local bool g_timing = false;
static thread_local int g_timing_columns = 0;
static thread_local std::deque<hipEvent_t> g_pool;                                    // free events, reused first-in first-out
static thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>> g_events;          // recorded (start, stop) pairs
static thread_local hipEvent_t g_pending = nullptr;
static hipEvent_t pool_get() {
  if (!g_pool.empty()) {
    hipEvent_t e = g_pool.front();
    g_pool.pop_front();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}
void timing_begin(hipStream_t stream) {
  if (!g_timing) return;
  if (!g_pending) g_pending = pool_get();            // (a launch that failed between begin and end left its event here)
  if (g_pending) (void)hipEventRecord(g_pending, stream);
}
void timing_end(hipStream_t stream, int columns) {
  if (!g_timing || !g_pending) return;
  hipEvent_t stop = pool_get();
  if (!stop) return;
  (void)hipEventRecord(stop, stream);
  g_events.emplace_back(g_pending, stop);
  g_pending = nullptr;
  g_timing_columns = columns;
}
}  // namespace ctd

extern "C" {

int ctd_version(void) { return 5; }

void ctd_kernel_timing_enable(int enable) {
  g_timing = enable != 0;
  if (g_timing) {
    // fill the pool up front (enough for a default bench region) and record every new event once: the runtime
    // allocates an event's signal at its first record, and that must not happen between the start event and the
    // kernel it brackets
    bool fresh = false;
    const size_t want = enable > 128 ? (size_t)enable : 128;          // `enable` doubles as the number of events to hold ready
    while (g_pool.size() < want) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) break;
      (void)hipEventRecord(e, nullptr);
      g_pool.push_back(e);
      fresh = true;
    }
    if (fresh) (void)hipStreamSynchronize(nullptr);
  } else if (g_pending) {
    g_pool.push_back(g_pending);
    g_pending = nullptr;
  }
}

int ctd_kernel_timing_collect(double* avg_ms, int* columns) {
  double total = 0;
  int n = 0;
  for (auto& ev : g_events) {
    float ms = 0.f;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      total += ms;
      ++n;
    }
    g_pool.push_back(ev.first);
    g_pool.push_back(ev.second);
  }
  g_events.clear();
  if (avg_ms) *avg_ms = n ? total / n : 0.0;
  if (columns) *columns = g_timing_columns;
  return n;
}

const char* ctd_status_string(int status) {
  switch (status) {
    case CTD_OK: return "ok";
    case CTD_ERR_INVALID_ARG: return "invalid argument";
    case CTD_ERR_WORKSPACE: return "workspace missing or too small";
    case CTD_ERR_UNSUPPORTED: return "unsupported parameter combination";
    default: break;
  }
  if (status >= CTD_ERR_HIP) return hipGetErrorString((hipError_t)(status - CTD_ERR_HIP));
  return "unknown status";
}

}  // extern "C"
