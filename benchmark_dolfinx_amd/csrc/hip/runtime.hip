// Native CG runtime: the whole timed CG loop of the fused operator in C++.
//
// The reference drives its CG from C++ (src/cg.hpp:89-169) over GPU-aware MPI
// with host round trips per dot product and two halo scatters per iteration
// (SURVEY.md quirks Q2/Q3), overlapping the forward scatter with the
// interior-cell kernel (src/laplacian.hpp:281-349).  This runtime owns one
// rank's iteration on two HIP streams, every scalar device-resident:
//
//   compute stream                     comm stream
//   --------------                     -----------
//   fused op, all interior tiles  ||   pack r faces -> RCCL send/recv -> unpack ghosts
//                                 ||   fused op, ghost-touching tiles (last row / column)
//                                 ||   ghost-plane finalize
//                                 ||   pack y ghosts -> RCCL send/recv
//   (join) unpack-add y faces
//   reduce(p.Ap) -> all-reduce -> r update (+ r.r) -> all-reduce
//
// The tile split needs an unsplit march axis (x): the partition keeps x whole
// on the GPU platform (fem/mesh.py partition_grid), so only the last (y, z)
// tile row / column touches a ghost plane and every other tile can run while
// the halo is in flight.  The whole comm-stream chain -- both exchanges and
// the small boundary launches -- runs under the one large interior launch.  Otherwise (x split, one
// rank) the iteration runs serially on the compute stream.  Halos are
// grouped RCCL point-to-point sends/receives with the <= 7 neighbours over
// xGMI; the steady-state iterations (two parities: the p buffers and the r.r
// slots ping-pong) are captured once into hipGraphs (fork/join over the two
// streams) and replayed.
//
// Failure containment: every blocking RCCL call and host wait runs inside a
// bdx::Watchdog scope (csrc/include/bdx_watchdog.h); past the deadline
// (BDX_RCCL_TIMEOUT_S, default 300 s) or on an asynchronous communicator
// error the communicator is aborted and the call returns an error that
// Python raises.  A second transport runs R ranks as threads of one process
// on one GPU (host barriers + device copies) so the multi-rank orchestration
// is testable on a single-GPU box.
//
// Python (solvers/native.py) builds the problem, runs the CG prologue
// (r0 = b - A x0, rho0) and hands the device buffers to this runtime.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_transport.h"  // Transport and its four implementations, bdx_common.h

// The fused2, fused3 and fused5 operator entry points (lap_fused{2,3,5}_<suf>_p<P>.hip)
// are referenced weakly, here alone, so that experiment builds holding a
// subset of the operator TUs still load (a missing instance resolves to null
// and bdx_rt_create refuses it).
#define BDX_PRAGMA(x) _Pragma(#x)
#define BDX_WEAK_APPLY(PP, V, SUF) BDX_PRAGMA(weak bdx_fused##V##_apply_##SUF##_p##PP)
BDX_FUSED_DEGREES(BDX_WEAK_APPLY, 2, f64)
BDX_FUSED_DEGREES(BDX_WEAK_APPLY, 2, f32)
BDX_FUSED_DEGREES(BDX_WEAK_APPLY, 3, f64)
BDX_FUSED_DEGREES(BDX_WEAK_APPLY, 3, f32)
BDX_FUSED5_DEGREES(BDX_WEAK_APPLY, 5, f64)
BDX_FUSED5_DEGREES(BDX_WEAK_APPLY, 5, f32)

namespace {

// The _f64 / _f32 twin of an entry point for the scalar type T, chosen at
// compile time: BDX_TWIN(T, bdx_xflush)(args...) is a direct call.
template <typename T, typename F64, typename F32>
constexpr auto twin(F64* f64, F32* f32) {
  if constexpr (sizeof(T) == 8)
    return f64;
  else
    return f32;
}
#define BDX_TWIN(T, NAME) twin<T>(NAME##_f64, NAME##_f32)

template <typename T>
using ApplyFn = int(*) BDX_P_FUSED_APPLY(T);

// The fused operator instance of (version, degree); null if the build lacks it.
template <typename T>
ApplyFn<T> apply_fn(int version, int P) {
#define BDX_CASE(PP, V)         \
  if (version == V && P == PP) \
    return twin<T>(bdx_fused##V##_apply_f64_p##PP, bdx_fused##V##_apply_f32_p##PP);
  BDX_FUSED_DEGREES(BDX_CASE, 2)
  BDX_FUSED_DEGREES(BDX_CASE, 3)
  BDX_FUSED5_DEGREES(BDX_CASE, 5)
#undef BDX_CASE
  return nullptr;
}

// ------------------------------------------------------------------ the CG loop
constexpr int kRR0 = 0, kRR1 = 1, kPAP = 2;

// Phase marks of one iteration (bdx_rt_profile).  In the serial schedule the
// marks that belong to the split schedule coincide with their neighbours.
enum Mark {
  kMStart = 0,   // compute stream: iteration start
  kMFwdBeg,      // comm stream: forward exchange start
  kMFwdEnd,      // comm stream: ghost planes of r unpacked
  kMOpA,         // compute: interior tiles / cells done (serial: the whole operator)
  kMBnd,         // comm: ghost-touching tiles / cells (+ ghost finalize) done
  kMRevBeg,      // comm: reverse exchange start
  kMRevEnd,      // comm: reverse send done (serial: + unpack-add)
  kMJoin,        // compute: comm stream joined, received sums added
  kMPap,         // compute: reduce + all-reduce(p.Ap) done
  kMUpd,         // compute: r update (+ r.r) done
  kMEnd,         // compute: all-reduce(r.r) done
  kNMarks
};

// What the fused-structured and the dofmap CG runtimes share: the transport,
// the two streams, the plane halo, the batched / watchdog-bounded iteration
// loop with its graph capture, the phase profiler and the pre-flight.  A
// derived runtime supplies one iteration (`step`) and the final x flush.
struct LoopBase {
  std::unique_ptr<Transport> tr;
  int nranks = 1, rank = 0;
  int esize = 8;  // vector element bytes
  // comm stream priority (hipDeviceGetStreamPriorityRange: least, greatest;
  // the priority cs was created with)
  int prio_least = 0, prio_greatest = 0, prio_cs = 0;
  double* pf_scal = nullptr;  // pre-flight all-reduce slot
  // own non-blocking streams (graph capture is not allowed on the legacy
  // default stream torch may be using); ordered against the caller's stream
  // `ext` with events at the start and end of every iterate()
  hipStream_t st = nullptr, cs = nullptr, ext = nullptr;
  // Split schedule, interior launch: on st (si == nullptr), or on its own
  // stream si whose CU mask leaves `reserve` CUs to the comm stream's chain
  // (BDX_SPLIT=mask; make_interior_stream).  cu_mask_cs: cs was created with
  // the complementary mask (BDX_SPLIT=maskr: the chain on the reserved CUs
  // only).
  hipStream_t si = nullptr;
  hipEvent_t ev_int = nullptr;
  int reserve = 0;
  std::vector<uint32_t> mask_si, mask_cs;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_fork = nullptr, ev_rev = nullptr;
  // halo: owned lower faces <-> ghost planes (parallel/halo.py layout), on
  // the storage layout `wlatd` describes
  bool halo = false, split = false;
  const int64_t* wlatd = nullptr;
  void *hbuf_a = nullptr, *hbuf_b = nullptr;
  const int64_t *face_boxes = nullptr, *ghost_boxes = nullptr;
  int nface_boxes = 0, nghost_boxes = 0;
  int64_t face_total = 0, ghost_total = 0;
  std::vector<int64_t> face_cnt, face_off, ghost_cnt, ghost_off;
  // phase profiling (eager iterations only)
  bool prof = false;
  hipEvent_t pev[kNMarks] = {};
  // state
  long it = 0;
  // Lagged x update: `pend` terms alpha_j p_j are not yet in x (0, 1 or 2).
  // One-term kernels fold alpha_prev p_old into x at every iteration (pend
  // stays 1).  fused5 pairs them (xpair): an iteration
  // with one term pending only saves alpha_prev (kXSave), the next folds
  // both, reading p_prev2 from the p buffer it is about to overwrite (kXPair)
  // -- x is read and written every other iteration, for one extra p read:
  // 5.5 instead of 6 operator streams per iteration, but unevenly spread.
  int pend = 0;
  bool xpair = false;
  // Staggered pairing (xpair on tiled storage, BDX_XSTAGGER): the odd tiles
  // ((ty + tz) odd) run the save / pair cycle one iteration out of phase
  // with their own pending count pend1, so every iteration carries half of
  // the x stream instead of all of it every other iteration.  The saved
  // alpha alternates between two scalar slots (kScalXSave + iteration parity).
  bool stagger = false;
  int pend1 = 0;
  int cur_m1 = kXSingle;  // the odd tiles' mode of the iteration being launched
  bool use_graph = true, graph_ok[4] = {false, false, false, false};
  hipGraphExec_t graph[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_batch[2] = {nullptr, nullptr};  // in-flight bound (iterate_on_stream)
  std::vector<hipEvent_t> tev;                  // per-step timing events

  virtual ~LoopBase() {
    drop_graphs();
    for (auto& e : pev)
      if (e) hipEventDestroy(e);
    for (hipEvent_t e : tev) hipEventDestroy(e);
    for (hipEvent_t e : {ev_in, ev_out, ev_fork, ev_rev, ev_batch[0], ev_batch[1]})
      if (e) hipEventDestroy(e);
    if (si) hipStreamDestroy(si);
    if (ev_int) hipEventDestroy(ev_int);
    if (st) hipStreamDestroy(st);
    if (cs) hipStreamDestroy(cs);
    if (pf_scal) hipFree(pf_scal);
  }
  // One CG iteration with explicit parity / flags (stream-ordered, no sync).
  // xm: kXSingle (pend 0: no x term; else alpha_prev p_old), kXSave, kXPair.
  virtual int step(long k, bool first, bool xlag, int xm) = 0;
  // x += the pending lagged terms (end of iterate() / profile())
  virtual int flush() = 0;
  // bring the prologue's state into the loop's own storage (tiled layouts)
  virtual int import_state() { return 0; }
  // the vector the forward halo carries (the pre-flight exchanges it)
  virtual void* halo_vector() = 0;
  virtual bool tiled() const { return false; }

  void mark(int id, hipStream_t s) {
    if (prof) (void)hipEventRecord(pev[id], s);
  }

  // The interior launch's stream of the split schedule (BDX_SPLIT):
  //   prio  (default) the compute stream st; the comm stream has the
  //         device's greatest priority;
  //   mask  its own stream si whose CU mask excludes BDX_SPLIT_RESERVE CUs
  //         (default 16), so the comm stream's chain -- RCCL kernels,
  //         boundary tiles, ghost fold -- always finds free CUs instead of
  //         queueing behind the interior grid's workgroups;
  //   maskr as mask, and the comm stream is confined to the reserved CUs.
  // The reserved CUs are mask bits 0 .. reserve-1, which the hardware deals
  // round-robin over the XCDs (csrc/micro/dispatch_prio.hip census).
  // hipExtStreamCreateWithCUMask takes no flags or priority: si (mask, maskr)
  // and the re-created cs (maskr) are BLOCKING streams at the DEFAULT
  // priority, unlike the non-blocking greatest-priority cs of init_common.
  // So in maskr the comm chain loses its priority, and both streams
  // synchronise with the legacy null stream: any work the caller submits to
  // the null stream while iterate() runs serialises with them.  The mask /
  // maskr A/Bs (profiles/r5_split_schedule.md) ran with nothing on the null
  // stream; comm_priority() reports the priority cs really has.
  int make_interior_stream() {
    const char* e = std::getenv("BDX_SPLIT");
    const std::string mode = e ? e : "prio";
    if (mode == "prio" || mode.empty()) return 0;
    if (mode != "mask" && mode != "maskr") return static_cast<int>(hipErrorInvalidValue);
    int dev = 0, ncu = 0;
    BDX_CHECK(hipGetDevice(&dev));
    BDX_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const char* r = std::getenv("BDX_SPLIT_RESERVE");
    reserve = r ? std::atoi(r) : 16;
    if (reserve < 1 || reserve >= ncu) return static_cast<int>(hipErrorInvalidValue);
    const int words = (ncu + 31) / 32;
    mask_si.assign(words, 0u);
    mask_cs.assign(words, 0u);
    for (int b = 0; b < ncu; ++b) (b < reserve ? mask_cs : mask_si)[b / 32] |= 1u << (b % 32);
    BDX_CHECK(hipExtStreamCreateWithCUMask(&si, static_cast<uint32_t>(words), mask_si.data()));
    BDX_CHECK(hipEventCreateWithFlags(&ev_int, hipEventDisableTiming));
    if (mode == "maskr") {
      BDX_CHECK(hipStreamDestroy(cs));
      cs = nullptr;
      BDX_CHECK(hipExtStreamCreateWithCUMask(&cs, static_cast<uint32_t>(words), mask_cs.data()));
      BDX_CHECK(hipStreamGetPriority(cs, &prio_cs));
    }
    return 0;
  }
  // interior launch `f(stream)` of the split schedule on si or st; st
  // continues after it (the caller then joins the comm stream)
  template <typename F>
  int interior(F&& f) {
    if (!si) return f(st);
    BDX_CHECK(hipStreamWaitEvent(si, ev_fork, 0));
    if (int rc = f(si)) return rc;
    BDX_CHECK(hipEventRecord(ev_int, si));
    BDX_CHECK(hipStreamWaitEvent(st, ev_int, 0));
    return 0;
  }

  // Streams, events, halo tables and the transport (every runtime kind).
  int init_common(hipStream_t ext_stream, const BdxRtHalo& h) {
    const int n = h.nranks;
    nranks = n;
    rank = h.rank;
    ext = ext_stream;
    // The comm stream runs at the greatest priority the device offers: its
    // chain (RCCL send/recv kernels, the boundary work, the reverse send) is
    // dispatched ahead of the interior launch's queued workgroups as soon as
    // resident ones retire, instead of after the whole interior grid.
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) {
      (void)hipGetLastError();
      prio_least = prio_greatest = 0;
    }
    BDX_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    BDX_CHECK(hipStreamCreateWithPriority(&cs, hipStreamNonBlocking, prio_greatest));
    BDX_CHECK(hipStreamGetPriority(cs, &prio_cs));
    for (hipEvent_t* e : {&ev_in, &ev_out, &ev_fork, &ev_rev, &ev_batch[0], &ev_batch[1]})
      BDX_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    hbuf_a = h.buf_a;
    hbuf_b = h.buf_b;
    face_boxes = h.face_boxes;
    ghost_boxes = h.ghost_boxes;
    nface_boxes = h.nface_boxes;
    face_total = h.face_total;
    nghost_boxes = h.nghost_boxes;
    ghost_total = h.ghost_total;
    face_cnt.assign(h.face_cnt, h.face_cnt + n);
    ghost_cnt.assign(h.ghost_cnt, h.ghost_cnt + n);
    face_off.assign(n, 0);
    ghost_off.assign(n, 0);
    for (int p = 1; p < n; ++p) {
      face_off[p] = face_off[p - 1] + face_cnt[p - 1];
      ghost_off[p] = ghost_off[p - 1] + ghost_cnt[p - 1];
    }
    halo = n > 1 && (face_total + ghost_total) > 0;
    if (h.transport == kBdxTransportRccl && n > 1) {  // connected by bdx_rt_connect
      auto t = std::make_unique<RcclTransport>();
      t->nranks = n;
      tr = std::move(t);
    } else if (h.transport == kBdxTransportThread && n > 1) {  // in-process threads
      auto t = std::make_unique<ThreadTransport>();
      {
        std::lock_guard<std::mutex> lk(g_groups_m);
        // joined while any rank's runtime still holds it: a rank that
        // replaces its runtime (a new DeviceCG on the same operator) before
        // its peers have closed theirs has to end up on the same state
        std::shared_ptr<ThreadGroupState> g = g_groups[h.group_id].lock();
        if (!g) {
          g = std::make_shared<ThreadGroupState>();
          g_groups[h.group_id] = g;
          g->size = n;
          g->sbuf.assign(n, nullptr);
          g->soff.assign(n, nullptr);
          g->packed.assign(n, nullptr);
          g->copied.assign(n, nullptr);
          g->red.assign(n, nullptr);
        }
        t->g = g;
      }
      t->rank = h.rank;
      tr = std::move(t);
    } else if (h.transport == kBdxTransportEmulated && n > 1) {  // emulated links (one rank alone)
      auto t = std::make_unique<LinkEmuTransport>();
      t->nranks = n;
      tr = std::move(t);
    } else {  // single rank: no communication
      tr = std::make_unique<NoTransport>();
      halo = false;
    }
    return 0;
  }

  int box_copy(int mode, void* vec, const int64_t* boxes, int nb, int64_t total, void* buf,
               hipStream_t s) {
    if (esize == 8)
      return bdx_box_copy_lat_f64(mode, static_cast<double*>(vec), wlatd, boxes, nb, total,
                                  static_cast<double*>(buf), s);
    return bdx_box_copy_lat_f32(mode, static_cast<float*>(vec), wlatd, boxes, nb, total,
                                static_cast<float*>(buf), s);
  }
  // forward: owned lower faces of v -> peers' ghost planes (pack, exchange, unpack)
  int halo_forward(void* v, hipStream_t s) {
    int rc = box_copy(0, v, face_boxes, nface_boxes, face_total, hbuf_a, s);
    if (rc || (rc = tr->exchange(hbuf_a, face_cnt, face_off, hbuf_b, ghost_cnt, ghost_off,
                                 esize, s)))
      return rc;
    return box_copy(1, v, ghost_boxes, nghost_boxes, ghost_total, hbuf_b, s);
  }
  // reverse, first half: ghost-plane partial sums of v -> peers (pack, exchange)
  int halo_reverse_send(void* v, hipStream_t s) {
    const int rc = box_copy(0, v, ghost_boxes, nghost_boxes, ghost_total, hbuf_a, s);
    if (rc) return rc;
    return tr->exchange(hbuf_a, ghost_cnt, ghost_off, hbuf_b, face_cnt, face_off, esize, s);
  }
  // reverse, second half: add the received sums into the owned lower faces
  int halo_reverse_add(void* v, hipStream_t s) {
    return box_copy(2, v, face_boxes, nface_boxes, face_total, hbuf_b, s);
  }

  // x mode of the next iteration (kXSingle with pend == 0: no x update)
  int next_xmode() const {
    if (pend == 0 || !xpair) return kXSingle;
    return pend == 1 ? kXSave : kXPair;
  }
  // the odd tiles' mode for an even-tile mode m0 (staggered pairing)
  int next_xmode1(int m0) const {
    if (!stagger) return m0;
    if (m0 == kXSave) return pend1 == 2 ? kXPair : kXSingle;
    if (m0 == kXPair) return kXSave;
    return kXSingle;
  }
  static int advanced(int p, int xm) { return (p == 0 || xm == kXPair) ? 1 : (xm == kXSave ? 2 : 1); }
  void advance_pend(int xm, int xm1) {
    pend = advanced(pend, xm);
    pend1 = stagger ? advanced(pend1, xm1) : pend;
  }
  // the periodic regime, in which one graph per (parity, even-tile mode) holds
  static bool periodic(int m0, int m1) {
    return (m0 == kXSave && m1 == kXPair) || (m0 == kXPair && m1 == kXSave);
  }

  // Capture the steady-state iteration of a parity and x mode (it > 0,
  // lagged x update pending); graph index = parity + 2 * (xm == kXPair).
  bool capture(int parity, int xm) {
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    const int rc = step(parity, false, true, xm);
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc || e != hipSuccess || !g) {
      if (g) hipGraphDestroy(g);
      (void)hipGetLastError();
      return false;
    }
    const int gi = parity + 2 * (xm == kXPair);
    const bool ok = hipGraphInstantiate(&graph[gi], g, nullptr, nullptr, 0) == hipSuccess;
    hipGraphDestroy(g);
    if (!ok) (void)hipGetLastError();
    return ok;
  }

  void drop_graphs() {
    for (int i = 0; i < 4; ++i) {
      if (graph[i]) hipGraphExecDestroy(graph[i]);
      graph[i] = nullptr;
      graph_ok[i] = false;
    }
  }

  // n iterations; step_ms (may be null): n per-step device times from
  // timing events recorded between the iterations (no extra work, no sync)
  int iterate(long n, float* step_ms = nullptr) {
    if (tr->aborted()) return kErrAborted;
    BDX_CHECK(hipEventRecord(ev_in, ext));
    BDX_CHECK(hipStreamWaitEvent(st, ev_in, 0));
    int rc = iterate_on_stream(n, step_ms);
    BDX_CHECK(hipEventRecord(ev_out, st));
    BDX_CHECK(hipStreamWaitEvent(ext, ev_out, 0));
    if (!rc && step_ms) {
      if ((rc = tr->wait(ev_out))) return rc;
      for (long i = 0; i < n; ++i) {
        BDX_CHECK(hipEventElapsedTime(&step_ms[i], tev[i], tev[i + 1]));
      }
    }
    return rc;
  }

  // Iterations are enqueued in batches of kBatch under a watchdog Busy
  // scope, and before each batch the host waits (bounded by the deadline)
  // for the batch before the previous one: at most 2 kBatch iterations are
  // in flight, so an enqueue can never block for long behind a stuck peer
  // outside a deadline-covered scope, and a long run never trips it.
  static constexpr long kBatch = 32;
  int iterate_on_stream(long n, float* step_ms) {
    if (int rc = import_state()) return rc;
    if (step_ms) {
      while (static_cast<long>(tev.size()) < n + 1) {
        hipEvent_t e = nullptr;
        BDX_CHECK(hipEventCreate(&e));
        tev.push_back(e);
      }
      BDX_CHECK(hipEventRecord(tev[0], st));
    }
    for (long i0 = 0; i0 < n; i0 += kBatch) {
      if (i0 >= 2 * kBatch) {
        if (int rc = tr->wait(ev_batch[(i0 / kBatch) % 2])) return rc;
      }
      bdx::Watchdog::Busy busy(tr->watchdog());
      for (long i = i0; i < n && i < i0 + kBatch; ++i) {
        const bool first = (it == 0);
        const int par = static_cast<int>(it % 2);
        const int xm = next_xmode();
        cur_m1 = next_xmode1(xm);
        const int gi = par + 2 * (xm == kXPair);
        const bool steady = !first && pend > 0 && !prof && (!stagger || periodic(xm, cur_m1));
        if (steady && use_graph && tr->capturable() && !graph_ok[gi]) {
          graph_ok[gi] = capture(par, xm);
          if (!graph_ok[gi]) use_graph = false;  // fall back to eager launches
        }
        if (steady && use_graph && graph_ok[gi]) {
          BDX_CHECK(hipGraphLaunch(graph[gi], st));
        } else {
          const int rc = step(it, first, pend > 0, xm);
          if (rc) return rc;
        }
        advance_pend(xm, cur_m1);
        ++it;
        if (step_ms) BDX_CHECK(hipEventRecord(tev[i + 1], st));
      }
      BDX_CHECK(hipEventRecord(ev_batch[(i0 / kBatch) % 2], st));
    }
    bdx::Watchdog::Busy busy(tr->watchdog());
    return flush();
  }

  // n eager iterations with timing events between the phases; *out = mean ms
  // of every interval (BdxRtPhases, bdx_rt_setup.h).
  int profile(long n, BdxRtPhases* out) {
    for (int i = 0; i < kNMarks; ++i)
      if (!pev[i]) BDX_CHECK(hipEventCreate(&pev[i]));
    *out = BdxRtPhases{};
    BDX_CHECK(hipEventRecord(ev_in, ext));
    BDX_CHECK(hipStreamWaitEvent(st, ev_in, 0));
    // prof is cleared on every exit path (an early error return must not
    // leave later iterate() calls eager and recording phase events)
    struct ProfGuard {
      bool& f;
      ~ProfGuard() { f = false; }
    } guard{prof};
    prof = true;
    bdx::Watchdog::Busy busy(tr->watchdog());
    int rc = import_state();
    for (long i = 0; i < n && !rc; ++i) {
      const bool first = (it == 0);
      const int xm = next_xmode();
      cur_m1 = next_xmode1(xm);
      rc = step(it, first, pend > 0, xm);
      if (rc) break;
      advance_pend(xm, cur_m1);
      ++it;
      if ((rc = static_cast<int>(hipEventRecord(ev_out, st)))) break;
      if ((rc = tr->wait(ev_out))) break;
      auto dt = [&](int a, int b) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, pev[a], pev[b]);
        return static_cast<double>(ms);
      };
      out->halo_fwd += dt(kMFwdBeg, kMFwdEnd);
      out->op_interior += dt(kMStart, kMOpA);
      // split: forward-halo end -> boundary work; serial: the boundary work
      // only (kMFwdEnd precedes the whole operator there)
      out->op_boundary += split ? dt(kMFwdEnd, kMBnd) : dt(kMOpA, kMBnd);
      out->halo_rev += dt(kMRevBeg, kMRevEnd);
      out->join_rev_add += dt(kMOpA, kMJoin);
      out->reduce_allreduce_pap += dt(kMJoin, kMPap);
      out->update_rr += dt(kMPap, kMUpd);
      out->allreduce_rr += dt(kMUpd, kMEnd);
      out->iteration += dt(kMStart, kMEnd);
      // timeline offsets from the iteration start: the comm-stream chain is
      // hidden when it completes before the interior work does
      out->t_halo_fwd_done += dt(kMStart, kMFwdEnd);
      out->t_boundary_done += dt(kMStart, kMBnd);
      out->t_halo_rev_done += dt(kMStart, kMRevEnd);
      out->t_op_interior_done += dt(kMStart, kMOpA);
    }
    prof = false;
    if (!rc) rc = flush();
    BDX_CHECK(hipEventRecord(ev_out, st));
    BDX_CHECK(hipStreamWaitEvent(ext, ev_out, 0));
    // the record is doubles and nothing else (tests/test_abi_layouts.py)
    double* const ms = reinterpret_cast<double*>(out);
    for (size_t i = 0; i < sizeof(BdxRtPhases) / sizeof(double) && n > 0; ++i)
      ms[i] /= static_cast<double>(n);
    return rc;
  }

  // Pre-flight of the transport before any timed work (bench.py at N > 1):
  // one forward halo exchange of the loop's halo vector and a device
  // all-reduce of (rank + 1), under a deadline of timeout_s instead of the
  // run's.  out->ms = host ms of both, out->allreduce = the all-reduce result
  // (n (n + 1) / 2 when every rank took part).  A peer that never joins
  // aborts the communicator: the error comes back here instead of a hang
  // inside the warmup.
  int preflight(double timeout_s, BdxRtPreflight* out) {
    if (!pf_scal) BDX_CHECK(hipMalloc(&pf_scal, sizeof(double)));
    const double v = rank + 1.0;
    bdx::Watchdog* wd = tr->watchdog();
    const double old = wd ? wd->timeout_s() : 0.0;
    if (wd && timeout_s > 0) wd->set_timeout(timeout_s);
    struct Restore {
      bdx::Watchdog* w;
      double t;
      ~Restore() {
        if (w) w->set_timeout(t);
      }
    } restore{wd, old};
    BDX_CHECK(hipEventRecord(ev_in, ext));
    BDX_CHECK(hipStreamWaitEvent(st, ev_in, 0));
    const int64_t t0 = bdx::Watchdog::now_ns();
    int rc = 0;
    {
      bdx::Watchdog::Busy busy(wd);
      BDX_CHECK(hipMemcpyAsync(pf_scal, &v, sizeof(double), hipMemcpyHostToDevice, st));
      if (halo) rc = halo_forward(halo_vector(), st);
      if (!rc && nranks > 1) rc = tr->allreduce_sum(pf_scal, 1, st);
      if (!rc) rc = static_cast<int>(hipEventRecord(ev_out, st));
    }
    if (!rc) rc = tr->wait(ev_out);
    if (rc) return rc;
    out->ms = (bdx::Watchdog::now_ns() - t0) * 1e-6;
    BDX_CHECK(hipMemcpy(&out->allreduce, pf_scal, sizeof(double), hipMemcpyDeviceToHost));
    BDX_CHECK(hipStreamWaitEvent(ext, ev_out, 0));
    return 0;
  }
};

// ---------------------------------------------------- fused structured operator
struct RtConfig {
  int64_t latd[kLatticeWords];
  int64_t latdT[kLatticeWords];  // tiled-storage descriptor (tsy = 0: lattice layout)
  int64_t own[3];
  int version, affine, P, nq, nblocks, nty, ntz, sy, sz, nseg;
  double kappa;
  std::vector<double> wts, qpts;
};

template <typename T>
struct CGRuntime final : LoopBase {
  RtConfig cfg;
  ApplyFn<T> apply = nullptr;
  std::vector<T> tabs_host;
  const T* tabs = nullptr;  // host copy (fused2/3: kernarg tables) or device buffer (fused5)
  T *x, *r, *pa, *pb, *y, *yb, *zb, *cb;
  // Tiled storage (a tiled descriptor cfg.latdT): the iteration runs on tiled copies
  // xt, rt, pat, pbt, yt (allocated zeroed by the caller: the padding stays
  // zero); r and x are imported after each prologue and x is exported after
  // every iterate() / profile().  wx .. wy: the buffers the loop works on.
  bool is_tiled = false, need_import = false;
  T *xt = nullptr, *rt_ = nullptr, *pat = nullptr, *pbt = nullptr, *yt = nullptr;
  T *wx, *wr, *wpa, *wpb, *wy;
  const T* xv;
  const T* kc = nullptr;
  double *scal, *partials, *upart;
  // Jacobi preconditioner binding (bdx_rt_set_precond; dinv == nullptr: none).
  // The operator kernels form p = u + beta p_old with alpha and beta as
  // ratios of scalar slots, so PCG is the same loop with u = z = dinv . r and
  // r.z in the slots that carry r.r: the update pass stores z and reduces r.z
  // into the `nxt` slot and the plain r.r into rr_slot, and the forward halo
  // carries z.  dinvt / zt: the tiled copies (zeroed by the caller), wz /
  // wdinv: what the loop works on.
  const T* dinv = nullptr;
  T* z = nullptr;
  T *dinvt = nullptr, *zt = nullptr;
  T* wz = nullptr;
  const T* wdinv = nullptr;
  double* upart_rr = nullptr;
  int rr_slot = -1;
  bool need_dinv_import = false;
  // overlapped schedule: tile rectangles {ty0, ty1, tz0, tz1}
  int rect_a[4], rect_r1[4], rect_r2[4];  // interior, last tile row, last tile column

  bool tiled() const override { return is_tiled; }
  bool precond() const { return dinv != nullptr; }
  // the vector the operator reads as u and the forward halo carries
  T* u_vector() { return precond() ? wz : wr; }
  void* halo_vector() override { return u_vector(); }

  int set_precond(const T* d, T* zz, T* dt, T* ztl, double* prr, int slot) {
    const hipError_t e = hipStreamSynchronize(st);
    drop_graphs();  // they hold the update pass and the halo vector of the old binding
    dinv = nullptr;
    z = dinvt = zt = wz = nullptr;
    wdinv = nullptr;
    upart_rr = nullptr;
    rr_slot = -1;
    need_dinv_import = false;
    if (!d) return static_cast<int>(e);
    if (!zz || !prr || prr == upart || slot < 0 || slot == kRR0 || slot == kRR1 || slot == kPAP ||
        slot == kScalXSave || slot == kScalXSave + 1 || (is_tiled && (!dt || !ztl)))
      return static_cast<int>(hipErrorInvalidValue);
    dinv = d;
    z = zz;
    dinvt = is_tiled ? dt : nullptr;
    zt = is_tiled ? ztl : nullptr;
    wz = is_tiled ? zt : z;
    wdinv = is_tiled ? dinvt : dinv;
    upart_rr = prr;
    rr_slot = slot;
    need_dinv_import = is_tiled;
    return static_cast<int>(e);
  }

  int convert(int dir, T* lat, T* til, hipStream_t s) {
    return BDX_TWIN(T, bdx_layout_convert)(dir, cfg.latdT, lat, til, s);
  }
  // tiled: bring the prologue's r and x (preconditioned: and z; once per
  // binding: dinv) into the tiled copies, p_old = 0
  int import_state() override {
    if (!is_tiled || !need_import) return 0;
    need_import = false;
    int rc;
    if ((rc = convert(0, r, rt_, st)) || (rc = convert(0, x, xt, st))) return rc;
    if (precond()) {
      if ((rc = convert(0, z, zt, st))) return rc;
      if (need_dinv_import && (rc = convert(0, const_cast<T*>(dinv), dinvt, st))) return rc;
      need_dinv_import = false;
    }
    const BdxLattice L = BdxLattice::from(cfg.latdT);
    return static_cast<int>(hipMemsetAsync(pat, 0, L.size() * sizeof(T), st));
  }
  int finalize_ghost(hipStream_t s) {
    return BDX_TWIN(T, bdx_fused_finalize)(wlatd, wy, yb, zb, cb, cfg.nty, cfg.ntz, cfg.sy,
                                           cfg.sz, 1, s);
  }

  // The fused operator of iteration k on the tile rectangle `rect` (null:
  // every tile) on stream s.
  int launch_op(long k, bool first, bool xlag, int xm, const int* rect, hipStream_t s) {
    const int cur = (k % 2 == 0) ? kRR0 : kRR1, nxt = cur == kRR0 ? kRR1 : kRR0;
    T* pold = (k % 2 == 0) ? wpa : wpb;
    T* pnew = (k % 2 == 0) ? wpb : wpa;
    // the saved alpha is written to the slot of this iteration's parity and
    // read from the other
    const int word = fused_mode_pack(kFusedCG, cfg.nseg, xm, stagger ? cur_m1 : -1,
                                     static_cast<int>(k & 1), static_cast<int>((k + 1) & 1));
    return apply(word, cfg.affine, wlatd, cfg.nq, cfg.wts.data(), cfg.qpts.data(), u_vector(),
                 pold, pnew, wx, wy, yb, zb, cb, xv, kc, tabs, cfg.kappa, scal, partials,
                 first ? -1 : cur, first ? -1 : nxt, xlag ? nxt : -1, xlag ? kPAP : -1, cfg.nty,
                 cfg.ntz, rect, s);
  }

  int step(long k, bool first, bool xlag, int xm) override {
    const int cur = (k % 2 == 0) ? kRR0 : kRR1, nxt = cur == kRR0 ? kRR1 : kRR0;
    T* const r = wr;
    T* const y = wy;
    T* const u = u_vector();  // forward halo: r, preconditioned: z
    auto op = [&](const int* rect, hipStream_t s) {
      return launch_op(k, first, xlag, xm, rect, s);
    };
    int rc;
    mark(kMStart, st);
    if (split) {
      // Two streams (reference src/laplacian.hpp:281-349, redesigned):
      //   cs: forward exchange -> boundary tiles (the last tile row and
      //       column, which read the ghost planes) -> ghost-plane fold ->
      //       reverse send;
      //   st: every interior tile, concurrently -- the exchanges and the
      //       small boundary launches all ride under the interior launch, so
      //       none of them is on the critical path as long as the interior
      //       work outlasts them;
      //   st: wait for cs, add the received sums into the owned faces.
      // Write sets are disjoint: a tile writes only its own nodes and its own
      // interface partials, and the ghost-plane fold reads only partials of
      // boundary tiles (fused_finalize_ghost_kernel).
      BDX_CHECK(hipEventRecord(ev_fork, st));
      BDX_CHECK(hipStreamWaitEvent(cs, ev_fork, 0));
      mark(kMFwdBeg, cs);
      if ((rc = halo_forward(u, cs))) return rc;
      mark(kMFwdEnd, cs);
      if ((rc = op(rect_r1, cs)) || (rc = op(rect_r2, cs)) || (rc = finalize_ghost(cs)))
        return rc;
      mark(kMBnd, cs);
      mark(kMRevBeg, cs);
      if ((rc = halo_reverse_send(y, cs))) return rc;
      BDX_CHECK(hipEventRecord(ev_rev, cs));
      mark(kMRevEnd, cs);
      if ((rc = interior([&](hipStream_t s) {
             const int r2 = op(rect_a, s);
             mark(kMOpA, s);
             return r2;
           })))
        return rc;
      BDX_CHECK(hipStreamWaitEvent(st, ev_rev, 0));
      if ((rc = halo_reverse_add(y, st))) return rc;
      mark(kMJoin, st);
    } else {
      mark(kMFwdBeg, st);
      if (halo && (rc = halo_forward(u, st))) return rc;
      mark(kMFwdEnd, st);
      if ((rc = op(nullptr, st))) return rc;
      mark(kMOpA, st);
      if (halo && (rc = finalize_ghost(st))) return rc;
      mark(kMBnd, st);
      mark(kMRevBeg, st);
      if (halo && ((rc = halo_reverse_send(y, st)) || (rc = halo_reverse_add(y, st)))) return rc;
      mark(kMRevEnd, st);
      mark(kMJoin, st);
    }
    if ((rc = bdx_reduce_partials(partials, cfg.nblocks, scal, kPAP, st))) return rc;
    if (nranks > 1 && (rc = tr->allreduce_sum(scal + kPAP, 1, st))) return rc;
    mark(kMPap, st);
    if (precond()) {
      // r update + z = dinv . r; r.z -> nxt, r.r -> rr_slot
      if (is_tiled)
        rc = BDX_TWIN(T, bdx_pcg_update_tiled)(wlatd, cfg.own, r, y, yb, zb, cb, cfg.nty, cfg.ntz,
                                               scal, cur, kPAP, nxt, upart, wdinv, wz, rr_slot,
                                               upart_rr, st);
      else
        rc = BDX_TWIN(T, bdx_pcg_update_iface)(cfg.latd, cfg.own, r, y, yb, zb, cb, cfg.nty,
                                               cfg.ntz, cfg.sy, cfg.sz, scal, cur, kPAP, nxt, upart,
                                               wdinv, wz, rr_slot, upart_rr, st);
    } else if (is_tiled) {
      rc = BDX_TWIN(T, bdx_cg_update_tiled)(wlatd, cfg.own, r, y, yb, zb, cb, cfg.nty, cfg.ntz, scal,
                                            cur, kPAP, nxt, upart, st);
    } else {
      rc = BDX_TWIN(T, bdx_cg_update_iface)(cfg.latd, cfg.own, r, y, yb, zb, cb, cfg.nty, cfg.ntz,
                                            cfg.sy, cfg.sz, scal, cur, kPAP, nxt, upart, st);
    }
    if (rc) return rc;
    mark(kMUpd, st);
    if (nranks > 1 && (rc = tr->allreduce_sum(scal + nxt, 1, st))) return rc;
    if (nranks > 1 && precond() && (rc = tr->allreduce_sum(scal + rr_slot, 1, st))) return rc;
    mark(kMEnd, st);
    return 0;
  }

  // x += alpha_last p_last (and, with two terms pending, the saved
  // alpha_prev p_prev, which is the last iteration's p_old)
  int flush() override {
    if (pend == 0 && pend1 == 0) return 0;
    const int last = ((it - 1) % 2 == 0) ? kRR0 : kRR1;
    T* plast = ((it - 1) % 2 == 0) ? wpb : wpa;  // p_new of the last iteration
    T* pprev = ((it - 1) % 2 == 0) ? wpa : wpb;  // its p_old
    // two terms pending: alpha_prev was saved by the last iteration
    const int slot = kScalXSave + static_cast<int>((it - 1) & 1);
    const bool two = pend == 2, two1 = stagger ? pend1 == 2 : two;
    if (is_tiled) {
      // export x + the pending terms in one pass; the tiled iterate keeps
      // them pending (the next call continues the lagged chain), which saves
      // the write-back of the tiled x (one of five streams of the pass)
      const T* p2 = (two || two1) ? pprev : nullptr;
      const int mask = (two ? 1 : 0) | (two1 ? 2 : 0) | 4;  // tile colours with two terms
      return BDX_TWIN(T, bdx_flush_export)(cfg.latdT, x, wx, plast, p2, scal, last, kPAP, slot, -1,
                                           mask, st);
    }
    pend = pend1 = 0;
    auto one = [&](T* p, int num, int den) {
      return BDX_TWIN(T, bdx_xflush)(cfg.latd, cfg.own, x, p, scal, num, den, st);
    };
    int rc = one(plast, last, kPAP);
    if (!rc && two) rc = one(pprev, slot, -1);
    return rc;
  }

  // Overlap probe (one rank only): does a comm-stream chain get CUs while the
  // interior launch fills the chip?  The chain of the split schedule of a
  // rank with y and z ghost planes (the N = 8 1 x 2 x 4 split) is replayed
  // on cs with a 1-rank RCCL communicator: grouped self send/recv of n
  // doubles (buf[0, n) -> buf[n, 2n)), the last tile row and column, the
  // reverse send/recv; concurrently st runs the interior tile rectangle.
  // *out: medians over reps (BdxRtOverlapProbe).  The CG state is clobbered:
  // the caller restarts CG afterwards.
  int overlap_probe(int64_t n, double* buf, int reps, BdxRtOverlapProbe* out) {
    if (nranks != 1 || cfg.nty < 2 || cfg.ntz < 2 || n <= 0 || reps <= 0)
      return static_cast<int>(hipErrorInvalidValue);
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -10;
    RcclTransport t;
    if (t.connect(id, 1, 0)) return -11;
    const std::vector<int64_t> cnt{n}, off0{0}, offn{n};
    auto xchg = [&](hipStream_t s) {
      return t.exchange(buf, cnt, off0, buf, cnt, offn, sizeof(double), s);
    };
    const int iy = cfg.nty - 1, iz = cfg.ntz - 1;
    const int ra[4] = {0, iy, 0, iz}, r1[4] = {iy, cfg.nty, 0, cfg.ntz}, r2[4] = {0, iy, iz, cfg.ntz};
    // ev (optional): recorded when the forward exchange is done
    auto chain = [&](hipStream_t s, hipEvent_t ev = nullptr) {
      int rc = xchg(s);
      if (!rc && ev) rc = static_cast<int>(hipEventRecord(ev, s));
      if (!rc) rc = launch_op(0, true, false, kXSingle, r1, s);
      if (!rc) rc = launch_op(0, true, false, kXSingle, r2, s);
      if (!rc) rc = xchg(s);
      return rc;
    };
    hipEvent_t e[5] = {};
    struct Free {  // before the creation loop: a failed create leaks nothing
      hipEvent_t* e;
      ~Free() {
        for (int i = 0; i < 5; ++i)
          if (e[i]) hipEventDestroy(e[i]);
      }
    } fr{e};
    for (auto& x : e) BDX_CHECK(hipEventCreate(&x));
    auto ms = [&](int a, int b) {
      float v = 0.f;
      (void)hipEventElapsedTime(&v, e[a], e[b]);
      return static_cast<double>(v);
    };
    BDX_CHECK(hipDeviceSynchronize());
    int rc = chain(cs);  // warm-up: RCCL connection setup, first launches
    if (!rc) rc = launch_op(0, true, false, kXSingle, ra, st);
    if (rc) return rc;
    BDX_CHECK(hipDeviceSynchronize());
    std::vector<double> chain_alone, interior_alone, chain_done, interior_done, exchange_alone,
        fwd_exchange_done;
    bdx::Watchdog::Busy busy(t.watchdog());
    for (int it = 0; it < reps; ++it) {
      // alone: the chain, the interior, one exchange (each drained before the next)
      BDX_CHECK(hipEventRecord(e[0], cs));
      if ((rc = chain(cs))) return rc;
      BDX_CHECK(hipEventRecord(e[1], cs));
      BDX_CHECK(hipDeviceSynchronize());
      BDX_CHECK(hipEventRecord(e[2], st));
      if ((rc = launch_op(0, true, false, kXSingle, ra, st))) return rc;
      BDX_CHECK(hipEventRecord(e[3], st));
      BDX_CHECK(hipDeviceSynchronize());
      chain_alone.push_back(ms(0, 1));
      interior_alone.push_back(ms(2, 3));
      BDX_CHECK(hipEventRecord(e[0], cs));
      if ((rc = xchg(cs))) return rc;
      BDX_CHECK(hipEventRecord(e[1], cs));
      BDX_CHECK(hipDeviceSynchronize());
      exchange_alone.push_back(ms(0, 1));
      // together, enqueued in the runtime's order: fork, cs chain, st interior
      BDX_CHECK(hipEventRecord(e[0], st));
      BDX_CHECK(hipStreamWaitEvent(cs, e[0], 0));
      if ((rc = chain(cs, e[4]))) return rc;
      BDX_CHECK(hipEventRecord(e[1], cs));
      if ((rc = launch_op(0, true, false, kXSingle, ra, st))) return rc;
      BDX_CHECK(hipEventRecord(e[2], st));
      BDX_CHECK(hipDeviceSynchronize());
      chain_done.push_back(ms(0, 1));
      interior_done.push_back(ms(0, 2));
      fwd_exchange_done.push_back(ms(0, 4));
    }
    auto median = [](std::vector<double>& v) {
      std::sort(v.begin(), v.end());
      return v[v.size() / 2];
    };
    out->chain_alone_ms = median(chain_alone);
    out->interior_alone_ms = median(interior_alone);
    out->chain_done_ms = median(chain_done);
    out->interior_done_ms = median(interior_done);
    out->exchange_alone_ms = median(exchange_alone);
    out->fwd_exchange_done_ms = median(fwd_exchange_done);
    return 0;
  }
};

// -------------------------------------------------------------- dofmap operator
// The reference's data model (explicit cell -> dof map, stored or on-the-fly G,
// atomic scatter; csrc/hip/lap_dofmap.h) on the same loop: the interior cells
// run on the compute stream while the comm stream does the forward exchange,
// the boundary cells (those touching a ghost dof) and the reverse send of the
// ghost partial sums -- the reference's scatter_fwd_begin / lcells /
// scatter_fwd_end / bcells schedule (src/laplacian.hpp:281-349), without its
// host syncs and with the boundary cells off the critical path.
struct DofConfig {
  int64_t latd[kLatticeWords];
  int P, nq, geom, n_inner, n_outer, nb_inner, nb_outer;
  int64_t nvec;
  double kappa;
};

template <typename T>
struct DofCGRuntime final : LoopBase {
  DofConfig cfg;
  const T* tab = nullptr;
  const int *inner = nullptr, *outer = nullptr, *cdofs = nullptr, *cverts = nullptr;
  const T *coords = nullptr, *G = nullptr, *kc = nullptr;
  const unsigned char* flags = nullptr;
  T *x, *r, *pa, *pb, *y;
  double *scal, *partials, *upart;
  // y ping-pong: iteration k's operator adds into yk(k) and zeroes yk(k + 1)
  // (consumed by the update pass of iteration k - 1), so the update pass
  // streams r, y and r back and no longer writes y = 0 (one vector stream
  // less per iteration; the zero stores ride in the operator's tail).  y2 is
  // the runtime's own second buffer; y (the caller's) is yk of even k.
  // Invariant: after iterate() the caller's y holds A p of the last even
  // iteration (NOT zero) and y2 may be dirty.  Only reset() (called by
  // DofmapLaplacianGPU.cg_start, which zeroes the caller's y first) makes
  // the loop valid again: iteration 0 then adds into a zero y and zeroes y2
  // before iteration 1 adds into it.  No caller may read y after iterate()
  // or hand the solve to the Python driver mid-way without cg_start
  // (tests/test_gpu_dofmap.py::test_dofmap_native_second_solve_*).
  T* y2 = nullptr;
  T* yk(long k) const { return (k % 2 == 0) ? y : y2; }

  ~DofCGRuntime() override {
    if (y2) (void)hipFree(y2);
  }

  void* halo_vector() override { return r; }

  // zero: this launch also zeroes yk(k + 1)
  int run(const int* cells, int ncl, double* part, long k, bool first, bool xlag, bool zero,
          hipStream_t s) {
    if (ncl <= 0) return 0;
    const int cur = (k % 2 == 0) ? kRR0 : kRR1, nxt = cur == kRR0 ? kRR1 : kRR0;
    T* pold = (k % 2 == 0) ? pa : pb;
    T* pnew = (k % 2 == 0) ? pb : pa;
    T* const yz = zero ? yk(k + 1) : nullptr;
    int nb = 0;
    return BDX_TWIN(T, bdx_dofmap_apply_yz)(
        cfg.P, cfg.nq, cfg.geom, 1, tab, cells, ncl, cfg.nvec, cdofs, cverts, coords, flags, G,
        cfg.kappa, kc, r, pold, pnew, x, yk(k), yz, scal, first ? -1 : cur, first ? -1 : nxt,
        xlag ? nxt : -1, xlag ? kPAP : -1, part, &nb, s);
  }

  int step(long k, bool first, bool xlag, int /*xm*/) override {
    const int cur = (k % 2 == 0) ? kRR0 : kRR1, nxt = cur == kRR0 ? kRR1 : kRR0;
    double* const part_b = partials + cfg.nb_inner;
    T* const yc = yk(k);
    // the interior launch zeroes yk(k + 1); the boundary one when there is none
    const bool z_in = cfg.n_inner > 0, z_out = !z_in;
    int rc;
    mark(kMStart, st);
    if (cfg.n_inner <= 0 && cfg.n_outer <= 0)  // a rank without cells: no launch zeroes it
      BDX_CHECK(hipMemsetAsync(yk(k + 1), 0, static_cast<size_t>(cfg.nvec) * sizeof(T), st));
    if (split) {
      // cs: forward exchange -> boundary cells -> reverse send of the ghost
      // partials; st: the interior cells (they touch no ghost dof), then the
      // received sums are added into the owned faces.  Both kernels add into
      // y with float atomics and write p / x only at their designated dofs
      // (lap_dofmap.h writer marks), so they may run concurrently.
      BDX_CHECK(hipEventRecord(ev_fork, st));
      BDX_CHECK(hipStreamWaitEvent(cs, ev_fork, 0));
      mark(kMFwdBeg, cs);
      if ((rc = halo_forward(r, cs))) return rc;
      mark(kMFwdEnd, cs);
      if ((rc = run(outer, cfg.n_outer, part_b, k, first, xlag, z_out, cs))) return rc;
      mark(kMBnd, cs);
      mark(kMRevBeg, cs);
      if ((rc = halo_reverse_send(yc, cs))) return rc;
      BDX_CHECK(hipEventRecord(ev_rev, cs));
      mark(kMRevEnd, cs);
      if ((rc = interior([&](hipStream_t s) {
             const int r2 = run(inner, cfg.n_inner, partials, k, first, xlag, z_in, s);
             mark(kMOpA, s);
             return r2;
           })))
        return rc;
      BDX_CHECK(hipStreamWaitEvent(st, ev_rev, 0));
      if ((rc = halo_reverse_add(yc, st))) return rc;
      mark(kMJoin, st);
    } else {
      mark(kMFwdBeg, st);
      if (halo && (rc = halo_forward(r, st))) return rc;
      mark(kMFwdEnd, st);
      if ((rc = run(inner, cfg.n_inner, partials, k, first, xlag, z_in, st))) return rc;
      mark(kMOpA, st);
      if ((rc = run(outer, cfg.n_outer, part_b, k, first, xlag, z_out, st))) return rc;
      mark(kMBnd, st);
      mark(kMRevBeg, st);
      if (halo && ((rc = halo_reverse_send(yc, st)) || (rc = halo_reverse_add(yc, st)))) return rc;
      mark(kMRevEnd, st);
      mark(kMJoin, st);
    }
    if ((rc = bdx_reduce_partials(partials, cfg.nb_inner + cfg.nb_outer, scal, kPAP, st)))
      return rc;
    if (nranks > 1 && (rc = tr->allreduce_sum(scal + kPAP, 1, st))) return rc;
    mark(kMPap, st);
    int nu = 0;
    rc = BDX_TWIN(T, bdx_dofmap_cg_update_z)(cfg.nvec, flags, r, yc, scal, cur, kPAP, upart, &nu, 0,
                                             st);
    if (rc || (rc = bdx_reduce_partials(upart, nu, scal, nxt, st))) return rc;
    mark(kMUpd, st);
    if (nranks > 1 && (rc = tr->allreduce_sum(scal + nxt, 1, st))) return rc;
    mark(kMEnd, st);
    return 0;
  }

  int flush() override {
    if (pend == 0) return 0;
    pend = 0;
    const int last = ((it - 1) % 2 == 0) ? kRR0 : kRR1;
    T* plast = ((it - 1) % 2 == 0) ? pb : pa;  // p_new of the last iteration
    return BDX_TWIN(T, bdx_dofmap_xflush)(cfg.nvec, x, plast, scal, last, kPAP, st);
  }
};

template <typename T>
LoopBase* create(const BdxRtFusedSetup& s, hipStream_t st) {
  auto rt = std::make_unique<CGRuntime<T>>();
  rt->esize = sizeof(T);
  RtConfig& c = rt->cfg;
  std::memcpy(c.latd, s.latd, sizeof(c.latd));
  std::memcpy(c.latdT, s.latd_tiled, sizeof(c.latdT));
  std::memcpy(c.own, s.own, sizeof(c.own));
  c.version = s.version;
  c.affine = s.affine;
  c.P = s.P;
  c.nq = s.nq;
  c.nblocks = s.nblocks;
  c.nty = s.nty;
  c.ntz = s.ntz;
  c.sy = s.sy;
  c.sz = s.sz;
  rt->use_graph = s.use_graph != 0;
  c.nseg = s.nseg > 0 ? s.nseg : 1;
  c.kappa = s.kappa;
  c.wts.assign(s.wts, s.wts + c.nq);
  c.qpts.assign(s.qpts, s.qpts + c.nq);
  rt->apply = apply_fn<T>(c.version, c.P);
  // paired lagged x update (fused5 only; BDX_XPAIR=0 folds one term per
  // iteration).  Paired on every tile at once, every other iteration carries
  // x, x and p_prev2 and the FP64 operator does not hide that burst (one
  // term per iteration was 2-4 % faster at Q6 FP64); staggered over the two
  // tile colours (tiled storage, below) the x stream is spread evenly and
  // the paired form is the fastest at Q3, Q6 and Q6 FP32
  // (profiles/r5_xpair_ab.md).
  {
    const char* e = std::getenv("BDX_XPAIR");
    rt->xpair = c.version == 5 && !(e && e[0] == '0');
  }
  if (!rt->apply || !bdx_rt_fused_setup_ok(s)) return nullptr;
  if (c.version == 5) {
    rt->tabs = static_cast<const T*>(s.tabs);  // the operator's device table buffer
  } else {
    const T* tb = static_cast<const T*>(s.tabs);
    rt->tabs_host.assign(tb, tb + kFusedTabMax);
    rt->tabs = rt->tabs_host.data();
  }
  rt->x = static_cast<T*>(s.x);
  rt->r = static_cast<T*>(s.r);
  rt->pa = static_cast<T*>(s.p_a);
  rt->pb = static_cast<T*>(s.p_b);
  rt->y = static_cast<T*>(s.y);
  rt->yb = static_cast<T*>(s.yb);
  rt->zb = static_cast<T*>(s.zb);
  rt->cb = static_cast<T*>(s.cb);
  rt->xv = static_cast<const T*>(s.xv);
  rt->kc = static_cast<const T*>(s.kc);
  rt->scal = s.scal;
  rt->partials = s.partials;
  rt->upart = s.upart;
  rt->is_tiled = BdxLattice::from(c.latdT).tsy != 0;
  if (rt->is_tiled) {
    rt->xt = static_cast<T*>(s.xt);
    rt->rt_ = static_cast<T*>(s.rt);
    rt->pat = static_cast<T*>(s.pat);
    rt->pbt = static_cast<T*>(s.pbt);
    rt->yt = static_cast<T*>(s.yt);
  }
  // staggered pairing needs the flush's per-tile colours (tiled storage);
  // BDX_XSTAGGER=0 pairs every tile on the same iterations
  {
    const char* e = std::getenv("BDX_XSTAGGER");
    rt->stagger = rt->xpair && rt->is_tiled && !(e && e[0] == '0');
  }
  rt->wx = rt->is_tiled ? rt->xt : rt->x;
  rt->wr = rt->is_tiled ? rt->rt_ : rt->r;
  rt->wpa = rt->is_tiled ? rt->pat : rt->pa;
  rt->wpb = rt->is_tiled ? rt->pbt : rt->pb;
  rt->wy = rt->is_tiled ? rt->yt : rt->y;
  rt->wlatd = rt->is_tiled ? c.latdT : c.latd;
  if (rt->init_common(st, s.halo)) return nullptr;
  // overlapped schedule: x whole, so only the last tile row (y ghost plane)
  // and the last tile column (z ghost plane) touch ghosts
  const BdxLattice L = BdxLattice::from(c.latd);
  const int g1 = static_cast<int>(L.gh[1]), g2 = static_cast<int>(L.gh[2]);
  if (s.overlap && rt->halo && L.gh[0] == 0 && (g1 || g2)) {
    const int iy = c.nty - g1, iz = c.ntz - g2;  // interior tile extents
    const int ra[4] = {0, iy, 0, iz};
    const int r1[4] = {iy, c.nty, 0, c.ntz}, r2[4] = {0, iy, iz, c.ntz};
    std::memcpy(rt->rect_a, ra, sizeof(ra));
    std::memcpy(rt->rect_r1, r1, sizeof(r1));
    std::memcpy(rt->rect_r2, r2, sizeof(r2));
    rt->split = true;
    if (rt->make_interior_stream()) return nullptr;
  }
  return rt.release();
}

template <typename T>
LoopBase* create_dofmap(const BdxRtDofmapSetup& s, hipStream_t st) {
  auto rt = std::make_unique<DofCGRuntime<T>>();
  rt->esize = sizeof(T);
  DofConfig& c = rt->cfg;
  std::memcpy(c.latd, s.latd, sizeof(c.latd));
  c.P = s.P;
  c.nq = s.nq;
  c.geom = s.geom;
  c.n_inner = s.n_inner;
  c.n_outer = s.n_outer;
  rt->use_graph = s.use_graph != 0;
  c.nvec = s.nvec;
  c.kappa = s.kappa;
  c.nb_inner = bdx_dofmap_nblocks(c.nq, c.n_inner);
  c.nb_outer = bdx_dofmap_nblocks(c.nq, c.n_outer);
  if (c.nb_inner < 0 || c.nb_outer < 0 || c.nb_inner + c.nb_outer > bdx_hip_partials_size())
    return nullptr;
  if (!bdx_rt_dofmap_setup_ok(s)) return nullptr;
  rt->x = static_cast<T*>(s.x);
  rt->r = static_cast<T*>(s.r);
  rt->pa = static_cast<T*>(s.p_a);
  rt->pb = static_cast<T*>(s.p_b);
  rt->y = static_cast<T*>(s.y);
  rt->scal = s.scal;
  rt->partials = s.partials;
  rt->upart = s.upart;
  rt->tab = static_cast<const T*>(s.tab);
  rt->inner = s.inner;
  rt->outer = s.outer;
  rt->cdofs = s.cdofs;
  rt->cverts = s.cverts;
  rt->coords = static_cast<const T*>(s.coords);
  rt->flags = s.flags;
  rt->G = static_cast<const T*>(s.G);
  rt->kc = static_cast<const T*>(s.kc);
  if (hipMalloc(&rt->y2, static_cast<size_t>(c.nvec) * sizeof(T)) != hipSuccess ||
      hipMemset(rt->y2, 0, static_cast<size_t>(c.nvec) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  rt->wlatd = c.latd;
  if (rt->init_common(st, s.halo)) return nullptr;
  rt->split = s.overlap && rt->halo && c.n_outer > 0;
  if (rt->split && rt->make_interior_stream()) return nullptr;
  return rt.release();
}

template <typename F>
auto with_rt(void* h, F&& f) {
  return f(static_cast<LoopBase*>(h));
}

}  // namespace

extern "C" {

int bdx_rt_nccl_unique_id(void* out128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
  std::memcpy(out128, &id, sizeof(id));
  return static_cast<int>(sizeof(id));
}

// Hardware self-test of the RCCL transport on one GPU (a 1-rank communicator):
// the grouped send/recv of RcclTransport::exchange to itself (buf[0, n) ->
// buf[n, 2n)), the device-scalar all-reduce of buf[2n, 2n+2), then the same
// pair captured into a hipGraph and replayed (into buf[2n+2, 3n+2)).  The
// multi-rank loop issues the identical calls over xGMI.  Returns 0 on success.
int bdx_rt_rccl_selftest(double* buf, int n, hipStream_t st) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -10;
  RcclTransport t;
  if (t.connect(id, 1, 0)) return -11;
  if (t.ranks() != 1) return -19;
  const std::vector<int64_t> cnt{n}, off0{0}, offn{n}, offg{2 * static_cast<int64_t>(n) + 2};
  int rc = t.exchange(buf, cnt, off0, buf, cnt, offn, sizeof(double), st);
  if (!rc) rc = t.allreduce_sum(buf + 2 * n, 2, st);
  if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = -12;
  if (rc) return rc;
  // capture on an own non-blocking stream, as the runtime does (the caller's
  // stream may be the legacy default stream, which cannot be captured)
  hipStream_t cs = nullptr;
  if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return -13;
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    hipStreamDestroy(cs);
    return -14;
  }
  rc = t.exchange(buf, cnt, off0, buf, cnt, offg, sizeof(double), cs);
  if (!rc) rc = t.allreduce_sum(buf + 2 * n, 2, cs);
  if (hipStreamEndCapture(cs, &g) != hipSuccess || !g) rc = rc ? rc : -15;
  if (!rc && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) rc = -16;
  if (!rc && hipGraphLaunch(ge, cs) != hipSuccess) rc = -17;
  hipEvent_t ev = nullptr;
  if (!rc && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) rc = -18;
  if (!rc && hipEventRecord(ev, cs) != hipSuccess) rc = -18;
  if (!rc) rc = t.wait(ev);  // the watchdog-bounded host wait of the runtime
  if (ev) hipEventDestroy(ev);
  if (ge) hipGraphExecDestroy(ge);
  if (g) hipGraphDestroy(g);
  hipStreamDestroy(cs);
  return rc;
}

void* bdx_rt_create(const BdxRtFusedSetup* setup, hipStream_t st) {
  return setup->is_f64 ? create<double>(*setup, st) : create<float>(*setup, st);
}

void* bdx_rt_create_dofmap(const BdxRtDofmapSetup* setup, hipStream_t st) {
  return setup->is_f64 ? create_dofmap<double>(*setup, st) : create_dofmap<float>(*setup, st);
}

int bdx_rt_comm_priority(void* h, BdxRtCommPriority* out) {
  return with_rt(h, [&](LoopBase* rt) {
    *out = {rt->prio_least, rt->prio_greatest, rt->prio_cs};
    return 0;
  });
}

// Transport pre-flight (see LoopBase::preflight).
int bdx_rt_preflight(void* h, double timeout_s, BdxRtPreflight* out) {
  return with_rt(h, [&](LoopBase* rt) { return rt->preflight(timeout_s, out); });
}

// Comm/compute overlap probe on one GPU (see CGRuntime::overlap_probe;
// fused operators only); buf: 2 n doubles.
int bdx_rt_overlap_probe(void* h, int64_t n, double* buf, int reps, BdxRtOverlapProbe* out) {
  return with_rt(h, [&](LoopBase* rt) -> int {
    if (auto* f = dynamic_cast<CGRuntime<double>*>(rt)) return f->overlap_probe(n, buf, reps, out);
    if (auto* f = dynamic_cast<CGRuntime<float>*>(rt)) return f->overlap_probe(n, buf, reps, out);
    return static_cast<int>(hipErrorInvalidValue);
  });
}

// 1 if the loop runs on the tiled storage layout.
int bdx_rt_tiled(void* h) {
  return with_rt(h, [](LoopBase* rt) { return rt->tiled() ? 1 : 0; });
}

// Open the runtime's RCCL communicator (collective over the ranks; every
// rank calls it only after all ranks created their runtime).  Bounded by the
// watchdog deadline.  0 on success (or when the transport is not RCCL).
int bdx_rt_connect(void* h, const void* uid, int rank) {
  return with_rt(h, [&](LoopBase* rt) -> int {
    auto* t = dynamic_cast<RcclTransport*>(rt->tr.get());
    if (!t) return 0;
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    return t->connect(id, t->nranks, rank);
  });
}

// Ranks of the transport (ncclCommCount for RCCL; -1 if not connected).
int bdx_rt_comm_count(void* h) {
  return with_rt(h, [](LoopBase* rt) { return rt->tr->ranks(); });
}

// 1 if the overlapped (split, two-stream) schedule is active.
int bdx_rt_overlap(void* h) {
  return with_rt(h, [](LoopBase* rt) { return rt->split ? 1 : 0; });
}

// Reset the CG state after a new prologue (p_a zeroed by the caller).
int bdx_rt_reset(void* h) {
  return with_rt(h, [](LoopBase* rt) {
    rt->it = 0;
    rt->pend = rt->pend1 = 0;
    if (auto* f = dynamic_cast<CGRuntime<double>*>(rt)) f->need_import = f->is_tiled;
    if (auto* f = dynamic_cast<CGRuntime<float>*>(rt)) f->need_import = f->is_tiled;
    return 0;
  });
}

// Bind a new iterate buffer x (DeviceCG.start with another x): the captured
// graphs hold the old pointer, so they are dropped and re-captured.
int bdx_rt_bind_x(void* h, void* x) {
  return with_rt(h, [&](LoopBase* rt) -> int {
    auto rebind = [&](auto* f) -> int {
      using T = std::remove_pointer_t<decltype(f->x)>;
      if (f->x == static_cast<T*>(x)) return 0;
      const hipError_t e = hipStreamSynchronize(f->st);
      f->drop_graphs();
      f->x = static_cast<T*>(x);
      if constexpr (std::is_same_v<std::remove_pointer_t<decltype(f)>, CGRuntime<T>>) {
        if (!f->is_tiled) f->wx = f->x;
      }
      return static_cast<int>(e);
    };
    if (auto* f = dynamic_cast<CGRuntime<double>*>(rt)) return rebind(f);
    if (auto* f = dynamic_cast<CGRuntime<float>*>(rt)) return rebind(f);
    if (auto* f = dynamic_cast<DofCGRuntime<double>*>(rt)) return rebind(f);
    if (auto* f = dynamic_cast<DofCGRuntime<float>*>(rt)) return rebind(f);
    return static_cast<int>(hipErrorInvalidValue);
  });
}

// Bind (dinv != null) or clear the Jacobi preconditioner of a fused runtime:
// dinv = 1 / diag(A) and z = dinv . r0 (the prologue's) in the lattice layout,
// their tiled copies (zeroed by the caller; needed iff the loop is tiled), a
// second partials buffer of bdx_hip_partials_size() doubles and the scalar
// slot that receives the plain r.r.  The r.r slots of the unpreconditioned
// loop then carry r.z.  Drops the captured graphs; call bdx_rt_reset after it.
int bdx_rt_set_precond(void* h, const void* dinv, void* z, void* dinv_tiled, void* z_tiled,
                       double* partials_rr, int rr_slot) {
  return with_rt(h, [&](LoopBase* rt) -> int {
    auto bind = [&](auto* f) -> int {
      using T = std::remove_pointer_t<decltype(f->x)>;
      return f->set_precond(static_cast<const T*>(dinv), static_cast<T*>(z),
                            static_cast<T*>(dinv_tiled), static_cast<T*>(z_tiled), partials_rr,
                            rr_slot);
    };
    if (auto* f = dynamic_cast<CGRuntime<double>*>(rt)) return bind(f);
    if (auto* f = dynamic_cast<CGRuntime<float>*>(rt)) return bind(f);
    return static_cast<int>(hipErrorInvalidValue);  // the dofmap loop has no such path
  });
}

int bdx_rt_iterate(void* h, long n) {
  return with_rt(h, [&](LoopBase* rt) { return rt->iterate(n); });
}

// iterate() plus the device time of each of the n steps (timing events
// between the steps, read after a bounded host wait): step_ms[n]
int bdx_rt_iterate_timed(void* h, long n, float* step_ms) {
  return with_rt(h, [&](LoopBase* rt) { return rt->iterate(n, step_ms); });
}

// Host wait for everything iterate() queued, bounded by the RCCL deadline
// (a hung peer aborts the communicator instead of blocking forever).
int bdx_rt_wait(void* h) {
  return with_rt(h, [](LoopBase* rt) { return rt->tr->wait(rt->ev_out); });
}

// n eager CG iterations with hipEvent phase timers (BdxRtPhases: mean ms).
int bdx_rt_profile(void* h, long n, BdxRtPhases* out) {
  return with_rt(h, [&](LoopBase* rt) { return rt->profile(n, out); });
}

// it (iterations done) and whether steady-state graphs are in use.
int bdx_rt_state(void* h, long* it, int* graphs) {
  return with_rt(h, [&](LoopBase* rt) {
    *it = rt->it;
    *graphs = rt->use_graph &&
              (rt->graph_ok[0] || rt->graph_ok[1] || rt->graph_ok[2] || rt->graph_ok[3]);
    return 0;
  });
}

void bdx_rt_destroy(void* h) { delete static_cast<LoopBase*>(h); }

// Called by every rank after it destroyed its runtime: the entry goes with
// the last runtime of the group (the runtimes own the state, the map only
// finds it).
void bdx_rt_release_group(int64_t group_id) {
  std::lock_guard<std::mutex> lk(g_groups_m);
  auto it = g_groups.find(group_id);
  if (it != g_groups.end() && it->second.expired()) g_groups.erase(it);
}

}  // extern "C"
