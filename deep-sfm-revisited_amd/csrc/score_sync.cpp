// Stream coordination around the RANSAC scoring phase (host code only): the
// score fence, the score gate and the reference-half jobs, with their C entry
// points.  The RANSAC driver (ransac5.hip) calls record_score_fence and
// wait_score_gate right before its scoring phase and take_ref_job once per call.
#include <algorithm>
#include <mutex>
#include "common.h"

namespace sfm {

constexpr int kFenceDevices = 64;
static std::mutex g_fence_mu;   // guards everything below

static int stream_device(hipStream_t s, int* dev) {
  if (hipStreamGetDevice(s, dev) != hipSuccess) SFM_HIP(hipGetDevice(dev));
  SFM_REQUIRE(*dev >= 0 && *dev < kFenceDevices, "score fence: device index out of range");
  return SFM_OK;
}

// An event created on device dev, whatever the caller's current device.
static int create_event_on(int dev, hipEvent_t* ev) {
  int cur = 0;
  SFM_HIP(hipGetDevice(&cur));
  SFM_HIP(hipSetDevice(dev));
  const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  SFM_HIP(hipSetDevice(cur));
  SFM_HIP(e);
  return SFM_OK;
}

// The slot of (dev, stream) in a table of slots { int dev (-1: free);
// hipStream_t stream; ... }.  With none and a `better` rule, the slot to take
// instead: the one the rule prefers over every other (null when it accepts none).
template <class Slot, size_t N>
static Slot* slot_of(Slot (&table)[N], int dev, hipStream_t stream,
                     bool (*better)(int dev, const Slot& s, const Slot* pick) = nullptr) {
  for (Slot& t : table)
    if (t.dev == dev && t.stream == stream) return &t;
  Slot* pick = nullptr;
  if (better)
    for (Slot& t : table)
      if (better(dev, t, pick)) pick = &t;
  return pick;
}

// Score fence (sfm_score_fence_enable / _wait): an event recorded on the
// RANSAC stream right before the scoring phase, so that a second stream can
// start pose-independent memory work (the cost volume's reference half) beside
// the compute-bound scorer instead of beside the latency-bound solve.  One
// event per device, created on that device (the device of the stream it is
// recorded on / waited from, never the caller's current device); recording is
// on while any enable(1) is not matched by an enable(0).
static hipEvent_t g_fence[kFenceDevices] = {};
static int g_fence_refs = 0;

// the fence of the stream's device (created there on first use); g_fence_mu held
static int fence_of(hipStream_t s, hipEvent_t* ev) {
  int dev = 0;
  if (int rc = stream_device(s, &dev)) return rc;
  if (!g_fence[dev])
    if (int rc = create_event_on(dev, &g_fence[dev])) return rc;
  *ev = g_fence[dev];
  return SFM_OK;
}

int record_score_fence(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  if (g_fence_refs <= 0) return SFM_OK;
  hipEvent_t ev = nullptr;
  if (int rc = fence_of(s, &ev)) return rc;
  SFM_HIP(hipEventRecord(ev, s));
  return SFM_OK;
}

// Score gate (sfm_score_gate): a library-owned event per (device, waiting
// stream), recorded on the caller's (side) stream; the next RANSAC call issued
// on that waiting stream waits for it right before its scoring phase
// (one-shot), so that a pipelined caller can run the previous step's
// HBM-bound sweep beside this step's latency-bound solve while keeping the
// compute-bound scorer to itself.  RANSAC calls on any other stream -- another
// hot path on the same device, a plain computeP -- neither wait for nor
// consume it.
constexpr int kGates = 32;
struct ScoreGate {
  int dev = -1;                  // -1: free slot
  hipStream_t stream = nullptr;  // the stream whose next scoring phase waits
  hipEvent_t ev = nullptr;       // kept when the slot is freed (reused on evdev)
  int evdev = -1;                // the device ev was created on
  bool armed = false;
};
static ScoreGate g_gates[kGates];

// a free slot, one with this device's event first (none free: no slot)
static bool gate_better(int dev, const ScoreGate& g, const ScoreGate* pick) {
  return g.dev < 0 && (!pick || (g.evdev == dev && pick->evdev != dev));
}

int wait_score_gate(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  int dev = 0;
  if (int rc = stream_device(s, &dev)) return rc;
  ScoreGate* g = slot_of(g_gates, dev, s);
  if (g && g->armed) {
    g->armed = false;
    g->dev = -1;
    SFM_HIP(hipStreamWaitEvent(s, g->ev, 0));
  }
  return SFM_OK;
}

// Reference-half jobs (sfm_score_ref_job): one slot per (device, stream), the
// job handed to the next RANSAC call issued on that stream, which consumes it
// whatever path it takes.  A slot holds no HIP object and nothing waits on it:
// arming again for a stream replaces its job, a job for a stream that never
// issues another RANSAC call is overwritten by the oldest-first reuse of the
// slots (it cannot exhaust them), and calls on other streams never see it.
constexpr int kRefJobs = 32;
struct RefJobSlot {
  int dev = -1;                  // -1: free
  hipStream_t stream = nullptr;
  unsigned long long seq = 0;    // arming order (the oldest slot is reused first)
  RefJob job;
};
static RefJobSlot g_ref_jobs[kRefJobs];
static unsigned long long g_ref_seq = 0;
static int g_ref_armed = 0;      // armed slots

// a free slot, else the oldest armed one (always some slot)
static bool job_better(int, const RefJobSlot& j, const RefJobSlot* pick) {
  return !pick || (pick->dev >= 0 && (j.dev < 0 || j.seq < pick->seq));
}

bool take_ref_job(hipStream_t s, RefJob* job) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  if (g_ref_armed == 0) return false;   // the common case: no HIP call
  int dev = 0;
  if (stream_device(s, &dev)) return false;
  RefJobSlot* j = slot_of(g_ref_jobs, dev, s);
  if (!j) return false;
  *job = j->job;
  j->dev = -1;
  --g_ref_armed;
  return true;
}

// job null: disarm
static int arm_ref_job(hipStream_t s, const RefJob* job) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  int dev = 0;
  if (int rc = stream_device(s, &dev)) return rc;
  RefJobSlot* slot = slot_of(g_ref_jobs, dev, s, job ? job_better : nullptr);
  if (!job) {
    if (slot) {
      slot->dev = -1;
      --g_ref_armed;
    }
    return SFM_OK;
  }
  if (slot->dev < 0) ++g_ref_armed;
  slot->dev = dev;
  slot->stream = s;
  slot->seq = ++g_ref_seq;
  slot->job = *job;
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_score_fence_enable(int on) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  g_fence_refs = on ? g_fence_refs + 1 : std::max(0, g_fence_refs - 1);
  return SFM_OK;
}

int sfm_score_fence_wait(void* stream) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  SFM_REQUIRE(g_fence_refs > 0, "score fence not enabled");
  hipEvent_t ev = nullptr;
  if (int rc = fence_of((hipStream_t)stream, &ev)) return rc;
  SFM_HIP(hipStreamWaitEvent((hipStream_t)stream, ev, 0));
  return SFM_OK;
}

int sfm_score_gate(void* stream, void* waiter, int arm) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  int dev = 0;
  if (int rc = stream_device((hipStream_t)stream, &dev)) return rc;
  ScoreGate* slot = slot_of(g_gates, dev, (hipStream_t)waiter, arm ? gate_better : nullptr);
  if (!arm) {
    if (slot) {
      slot->armed = false;
      slot->dev = -1;
    }
    return SFM_OK;
  }
  SFM_REQUIRE(slot != nullptr, "score gate: too many armed (device, stream) gates");
  if (slot->evdev != dev) {
    if (slot->ev) {                                          // an event of another device
      hipEvent_t old = slot->ev;
      slot->ev = nullptr;
      slot->evdev = -1;
      SFM_HIP(hipEventDestroy(old));
    }
    if (int rc = create_event_on(dev, &slot->ev)) return rc;
    slot->evdev = dev;
  }
  SFM_HIP(hipEventRecord(slot->ev, (hipStream_t)stream));
  slot->dev = dev;
  slot->stream = (hipStream_t)waiter;
  slot->armed = true;
  return SFM_OK;
}

int sfm_score_ref_job(void* stream, const float* ref, void* cost, int batch, int channels, int nlabel, int h, int w,
                      int cost_dtype) {
  if (!ref && !cost) return arm_ref_job((hipStream_t)stream, nullptr);   // disarm
  SFM_REQUIRE(ref && cost, "null pointer argument");
  // (the limits of sfm_plane_sweep_ref_planes, which writes the job when the scorer cannot)
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && channels <= 65535 && h >= 1 && w >= 1 && nlabel >= 1,
              "invalid sweep shape");
  SFM_REQUIRE((int64_t)batch * channels <= 65535, "batch * channels must be <= 65535");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 30), "feature map too large");
  SFM_REQUIRE(cost_dtype == 0 || cost_dtype == 1, "cost_dtype must be 0 (float32) or 1 (bfloat16)");
  RefJob j;
  j.ref = ref; j.cost = cost; j.batch = batch; j.channels = channels; j.nlabel = nlabel; j.h = h; j.w = w;
  j.dtype = cost_dtype;
  return arm_ref_job((hipStream_t)stream, &j);
}

// 0 / 1 ...: the armed jobs (tests: nothing accumulates)
int sfm_score_ref_jobs_armed(void) {
  std::lock_guard<std::mutex> lk(g_fence_mu);
  return g_ref_armed;
}

}  // extern "C"
