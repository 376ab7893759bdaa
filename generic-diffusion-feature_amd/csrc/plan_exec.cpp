// The plan executor every front end runs through (UNet, ControlNet, Flux, PixArt, VAE encoder and decoder): plan_run decides between graph
// replay, timed graph replay, eager launching and the per-op profile; ONE loop (run_ops) walks the op program for all of them.  Also here:
// the explicit graph recorder of launch.h, the hipGraph cache, the timing-event ring of gdf_plan_set_timing and the stream-capture guard.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <shared_mutex>

#include "launch.h"
#include "model.h"

namespace gdf {

static std::shared_mutex& capture_mx() { static std::shared_mutex mx; return mx; }
static bool capture_guard_on() { static const bool on = [] { const char* e = getenv("GDF_CAPTURE_GUARD"); return !e || atoi(e) != 0; }(); return on; }   // 0: diagnostics (tests/test_gpu_dist.py reproduces the invalidation)
CaptureShared::CaptureShared() { if (capture_guard_on()) capture_mx().lock_shared(); }
CaptureShared::~CaptureShared() { if (capture_guard_on()) capture_mx().unlock_shared(); }
CaptureExclusive::CaptureExclusive() { if (capture_guard_on()) capture_mx().lock(); }
CaptureExclusive::~CaptureExclusive() { if (capture_guard_on()) capture_mx().unlock(); }

Plan::~Plan() {
  CaptureExclusive guard;
  for (auto& v : ev) for (auto e : v) hipEventDestroy(e);
  for (auto& g : graphs) { if (g.exec) hipGraphExecDestroy(g.exec); if (g.graph) hipGraphDestroy(g.graph); }
}

// ---- live per-kernel timing (gdf_plan_set_timing): a ring of EV_RING event sets, one forward each -------------------------------------
static void timing_collect(Plan& P, int set) {
  if (!P.ev_used[set]) return;
  auto& v = P.ev[set];
  size_t k = 0;
  long nlab = 0;
  for (auto& op : P.ops) {
    if (op.label != P.timing_label) continue;
    if ((nlab++ % P.timing_stride) != 0) continue;
    float ms = 0.f;
    hipEventSynchronize(v[k + 1]);
    if (hipEventElapsedTime(&ms, v[k], v[k + 1]) == hipSuccess) { P.t_ms += ms; P.t_flops += op.flops; P.t_launches++; }
    k += 2;
  }
  P.ev_used[set] = false;
}

int plan_set_timing(Plan& P, const char* label) {
  for (int s = 0; s < Plan::EV_RING; ++s) timing_collect(P, s);
  P.timing_label = -1; P.t_ms = 0; P.t_flops = 0; P.t_launches = 0;
  if (!label) return GDF_OK;
  for (size_t i = 0; i < P.labels.size(); ++i) if (P.labels[i] == label) P.timing_label = (int)i;
  if (P.timing_label < 0) { set_error(std::string("no op with kernel label ") + label); return GDF_ERR_ARG; }
  size_t n = 0;
  for (auto& op : P.ops) n += op.label == P.timing_label;          // (an upper bound with a stride > 1)
  for (int s = 0; s < Plan::EV_RING; ++s)
    while (P.ev[s].size() < 2 * n) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { set_error("hipEventCreate"); return GDF_ERR_HIP; } P.ev[s].push_back(e); }
  return GDF_OK;
}

int plan_read_timing(Plan& P, double* ms, long* launches, double* flops) {
  for (int s = 0; s < Plan::EV_RING; ++s) timing_collect(P, s);
  if (ms) *ms = P.t_ms;
  if (launches) *launches = P.t_launches;
  if (flops) *flops = P.t_flops;
  return GDF_OK;
}

// ---- explicit graph construction (launch.h): the recorder of the calling thread, kernel / event-record nodes in one chain ----
GraphRecorder*& thread_recorder() { static thread_local GraphRecorder* r = nullptr; return r; }
static hipError_t chain(GraphRecorder& r, hipGraphNode_t node) { r.last = node; ++r.nodes; return hipSuccess; }
hipError_t record_kernel_node(GraphRecorder& r, const void* fn, dim3 grid, dim3 block, void** args, unsigned smem) {
  hipKernelNodeParams kp{};
  kp.func = const_cast<void*>(fn); kp.gridDim = grid; kp.blockDim = block; kp.sharedMemBytes = smem; kp.kernelParams = args; kp.extra = nullptr;
  hipGraphNode_t node = nullptr;
  const hipError_t e = hipGraphAddKernelNode(&node, r.graph, r.last ? &r.last : nullptr, r.last ? 1 : 0, &kp);     // (the argument VALUES are copied here)
  return e != hipSuccess ? e : chain(r, node);
}
// An event-record NODE at the current end of the chain (fires at every replay): the timed replays of bench.py (gdf_plan_set_timing)
hipError_t record_event_node(GraphRecorder& r, hipEvent_t ev) {
  hipGraphNode_t node = nullptr;
  const hipError_t e = hipGraphAddEventRecordNode(&node, r.graph, r.last ? &r.last : nullptr, r.last ? 1 : 0, ev);
  return e != hipSuccess ? e : chain(r, node);
}

// ---- the op loop -----------------------------------------------------------------------------------------------------------------------
// Walks the op program once and ends with the UNet's scheduler update (model.h unet_scheduler_step).
// evset >= 0: the timing events of set `evset` go around every timing_stride-th op of the timed label — as event-record nodes while this
// thread records the plan's graph (they fire at every replay), as plain hipEventRecord calls otherwise.
// ms != nullptr: the per-op profile — each of the first `cap` ops between two events of its own, synchronised per op.
static int run_ops(Plan& P, const Bind& b, hipStream_t s, int evset, float* ms = nullptr, const char** names = nullptr, double* flops = nullptr,
                   int cap = 0) {
  GraphRecorder* const rec = thread_recorder();
  auto record = [&](hipEvent_t ev) { return rec ? record_event_node(*rec, ev) : hipEventRecord(ev, s); };
  struct ProfileEvents {                                  // destroyed on every exit
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~ProfileEvents() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
  } prof;
  if (ms) { hipEventCreate(&prof.e0); hipEventCreate(&prof.e1); }
  size_t evk = 0;
  long nlab = 0;
  int i = 0;
  for (auto& op : P.ops) {
    const bool profiled = ms && i < cap;
    if (profiled) hipEventRecord(prof.e0, s);
    const bool timed = evset >= 0 && op.label == P.timing_label && (nlab++ % P.timing_stride) == 0;
    if (timed) {
      const hipError_t ee = record(P.ev[evset][evk]);
      if (ee != hipSuccess) {
        char buf[160]; snprintf(buf, sizeof buf, "hipEventRecord failed: %s (event %p, stream %p, evk %zu of %zu, recording %d)",
                                hipGetErrorString(ee), (void*)P.ev[evset][evk], (void*)s, evk, P.ev[evset].size(), (int)(rec != nullptr));
        set_error(buf); return GDF_ERR_HIP;
      }
    }
    const hipError_t e = op.fn(b, s);
    if (timed) {
      const hipError_t ee = record(P.ev[evset][evk + 1]);
      if (ee != hipSuccess && e == hipSuccess) { set_error("hipEventRecord failed"); return GDF_ERR_HIP; }
      evk += 2;
    }
    if (e != hipSuccess) { set_error(std::string("op '") + op.name + "' failed: " + hipGetErrorString(e)); return GDF_ERR_HIP; }
    if (profiled) {
      hipEventRecord(prof.e1, s); hipEventSynchronize(prof.e1);
      hipEventElapsedTime(&ms[i], prof.e0, prof.e1);
      if (names) names[i] = op.name;
      if (flops) flops[i] = op.flops;
    }
    ++i;
  }
  return unet_scheduler_step(P, b, s);
}

// hipGraph path: the op program is recorded once per distinct binding table into a hipGraph (explicit kernel nodes, launch.h) and replayed on
// the caller's stream with one hipGraphLaunch; ~2400 kernel launches per SDXL forward become one host call.
static int run_ops_graph(Plan& P, const Bind& b, hipStream_t s, int evset = -1) {
  const size_t nh = P.hooks.size();
  const int label = evset >= 0 ? P.timing_label : -1;
  for (auto& g : P.graphs) {
    bool same = g.evset == evset && g.label == label && memcmp(g.key.base, b.base, sizeof b.base) == 0 && memcmp(g.key.f, b.f, sizeof b.f) == 0 &&
                memcmp(&g.key.mt, &b.mt, sizeof b.mt) == 0 &&
                g.hook_ptrs.size() == nh;
    for (size_t i = 0; same && i < nh; ++i) same = g.hook_ptrs[i] == b.hooks[i];
    if (same) {
      g.stamp = ++P.graph_clock; ++P.graph_launches;
      if (hipGraphLaunch(g.exec, s) != hipSuccess) { set_error("hipGraphLaunch failed"); return GDF_ERR_HIP; }
      return GDF_OK;
    }
  }
  Plan::GraphEntry g;
  g.key = b; g.key.hooks = nullptr; g.evset = evset; g.label = label;
  for (size_t i = 0; i < nh; ++i) g.hook_ptrs.push_back(b.hooks[i]);
  // The graph is BUILT, not captured (launch.h): while this thread's recorder is set, every kernel launch of the op program appends a kernel
  // node (and every timing event an event-record node) to one dependency chain.  No stream is ever in capture mode, so nothing another host
  // thread does — allocating, freeing, synchronising the device, building its own graphs — can invalidate it (one extractor per thread:
  // aggregation_network.py:67-95).
  int rc;
  hipError_t e = hipGraphCreate(&g.graph, 0);
  if (e != hipSuccess) { (void)hipGetLastError(); g.graph = nullptr; rc = GDF_ERR_HIP; }
  else {
    GraphRecorder rec; rec.graph = g.graph;
    thread_recorder() = &rec;
    rc = run_ops(P, b, s, evset);
    thread_recorder() = nullptr;
    e = rec.err;
    if (rc == GDF_OK && e != hipSuccess) { set_error(std::string("graph node creation failed: ") + hipGetErrorString(e)); rc = GDF_ERR_HIP; }
  }
  static const bool dbg = getenv("GDF_DEBUG_GRAPH") != nullptr;
  if (dbg) fprintf(stderr, "[gdf] graph build evset=%d rc=%d err=%s graph=%p (%s)\n", evset, rc, hipGetErrorString(e), (void*)g.graph, rc ? last_error() : "");
  auto failed = [&](const char* what, hipError_t err) {
    // reported once per plan: a persistently failing capture would otherwise silently turn every forward into ~1000 eager launches
    if (P.graph_capture_failures++ == 0)
      fprintf(stderr, "[gdf] hipGraph %s failed (%s%s%s): this forward runs eagerly; gdf_plan_graph_failures() counts such calls\n", what,
              hipGetErrorString(err), rc != GDF_OK ? "; " : "", rc != GDF_OK ? last_error() : "");
  };
  if (rc != GDF_OK || e != hipSuccess || !g.graph) {
    // a recording that failed has executed nothing: drop it and run this forward eagerly (the ops are pure functions of their inputs);
    // the next call tries again
    if (g.graph) hipGraphDestroy(g.graph);
    (void)hipGetLastError();
    failed("construction", e);
    return run_ops(P, b, s, evset);
  }
  hipError_t ie;
  { CaptureExclusive guard; ie = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0); }      // (allocates: not beside another thread's capture)
  if (ie != hipSuccess) {
    hipGraphDestroy(g.graph);
    (void)hipGetLastError();
    failed("instantiate", ie);
    return run_ops(P, b, s, evset);
  }
  ++P.graph_captures;
  if (P.graphs.size() >= 12) {                           // evict the least recently used entry (timed replays: one graph per event set)
    size_t lru = 0;
    for (size_t i = 1; i < P.graphs.size(); ++i) if (P.graphs[i].stamp < P.graphs[lru].stamp) lru = i;
    { CaptureExclusive guard; hipGraphExecDestroy(P.graphs[lru].exec); hipGraphDestroy(P.graphs[lru].graph); }
    P.graphs.erase(P.graphs.begin() + lru);
  }
  g.stamp = ++P.graph_clock; ++P.graph_launches;
  P.graphs.push_back(g);
  if (hipGraphLaunch(P.graphs.back().exec, s) != hipSuccess) { set_error("hipGraphLaunch failed"); return GDF_ERR_HIP; }
  return GDF_OK;
}

// The decision only: profile, eager, graph replay, or their timed forms.
int plan_run(Plan& P, const Bind& b, hipStream_t s, float* ms, const char** names, double* flops, int cap) {
  const bool first = !P.warmed;
  P.warmed = true;
  if (ms) return run_ops(P, b, s, -1, ms, names, flops, cap);
  const bool graph = P.graph_mode && s != nullptr;
  if (graph && first) return run_ops(P, b, s, -1);                   // a graph plan's first forward: eager and untimed (lazy one-time kernel attribute setup)
  if (P.timing_label < 0) return graph ? run_ops_graph(P, b, s) : run_ops(P, b, s, -1);
  // timed: this forward uses event set `evset`; its results are collected when the set comes round again (or on read)
  const int evset = P.ev_next; P.ev_next = (P.ev_next + 1) % Plan::EV_RING;
  timing_collect(P, evset);
  int rc;
  if (graph && !P.timed_graph_broken) {
    const long fails = P.graph_capture_failures;
    rc = run_ops_graph(P, b, s, evset);
    if (P.graph_capture_failures != fails) P.timed_graph_broken = true;     // ran eagerly (with plain events); stay eager from now on
  } else {
    rc = run_ops(P, b, s, evset);
  }
  if (rc == GDF_OK) P.ev_used[evset] = true;
  return rc;
}

}  // namespace gdf
