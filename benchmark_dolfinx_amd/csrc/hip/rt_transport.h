// Transports of the native CG runtime (runtime.hip): how one rank's loop
// exchanges halos and all-reduces its device scalars.  RCCL between the ranks
// of a multi-GPU run, an emulated link for timing one rank of N alone, none
// for a single rank, and R threads of one process on one GPU for the tests.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "bdx_common.h"
#include "bdx_watchdog.h"

namespace {


// Error codes returned to Python (besides hipError_t values).
constexpr int kErrAborted = -20;   // the watchdog aborted the communicator
constexpr int kErrNotConnected = -21;

// ------------------------------------------------------------------ transports
struct Transport {
  virtual ~Transport() = default;
  // Grouped point-to-point exchange: rank p receives rcnt[p] elements from
  // each peer (into rbuf + roff[p]) and sends scnt[p] elements to it.
  virtual int exchange(const void* sbuf, const std::vector<int64_t>& scnt,
                       const std::vector<int64_t>& soff, void* rbuf,
                       const std::vector<int64_t>& rcnt, const std::vector<int64_t>& roff,
                       int esize, hipStream_t st) = 0;
  virtual int allreduce_sum(double* dev, int n, hipStream_t st) = 0;
  virtual bool capturable() const = 0;
  virtual int ranks() const = 0;
  // Host wait for `ev` (the end of queued work that may contain
  // communication), bounded by the transport's deadline.
  virtual int wait(hipEvent_t ev) { return static_cast<int>(hipEventSynchronize(ev)); }
  virtual bool aborted() const { return false; }
  // Deadline watchdog whose Busy scopes must cover every host call that can
  // block behind a stuck peer (RCCL only; null otherwise).
  virtual bdx::Watchdog* watchdog() { return nullptr; }
};

double rccl_timeout_s() {
  const char* e = std::getenv("BDX_RCCL_TIMEOUT_S");
  return e ? std::atof(e) : 300.0;
}

struct RcclTransport final : Transport {
  std::atomic<ncclComm_t> comm{nullptr};
  int nranks = 1;
  std::atomic<bool> was_aborted{false};
  std::unique_ptr<bdx::Watchdog> wd;

  RcclTransport() {
    wd = std::make_unique<bdx::Watchdog>(
        rccl_timeout_s(),
        [this] {
          ncclComm_t c = comm.load();
          if (!c || was_aborted.load()) return false;
          ncclResult_t e = ncclSuccess;
          if (ncclCommGetAsyncError(c, &e) != ncclSuccess) return true;
          return e != ncclSuccess && e != ncclInProgress;
        },
        [this] {
          ncclComm_t c = comm.load();
          if (!c) {
            // still inside ncclCommInitRank: nothing to abort, fail fast
            std::fprintf(stderr,
                         "[bdx] RCCL communicator init exceeded %.0f s; a peer never joined. "
                         "Exiting.\n",
                         wd->timeout_s());
            std::fflush(stderr);
            std::_Exit(124);
          }
          std::fprintf(stderr, "[bdx] RCCL %s; aborting the communicator\n",
                       wd->reason() == 1 ? "call exceeded the deadline" : "asynchronous error");
          std::fflush(stderr);
          was_aborted.store(true);
          ncclCommAbort(c);
        });
  }
  ~RcclTransport() override {
    if (wd) wd->stop();
    ncclComm_t c = comm.load();
    if (c && !was_aborted.load()) ncclCommDestroy(c);
  }
  int connect(const ncclUniqueId& id, int n, int rank) {
    nranks = n;
    wd->start();
    bdx::Watchdog::Busy b(wd.get());
    ncclComm_t c = nullptr;
    if (ncclCommInitRank(&c, n, id, rank) != ncclSuccess) return -1;
    comm.store(c);
    return 0;
  }
  bool aborted() const override { return was_aborted.load(); }
  bdx::Watchdog* watchdog() override { return wd.get(); }
  int exchange(const void* sbuf, const std::vector<int64_t>& scnt,
               const std::vector<int64_t>& soff, void* rbuf, const std::vector<int64_t>& rcnt,
               const std::vector<int64_t>& roff, int esize, hipStream_t st) override {
    ncclComm_t c = comm.load();
    if (!c) return kErrNotConnected;
    if (was_aborted.load()) return kErrAborted;
    bdx::Watchdog::Busy b(wd.get());
    const ncclDataType_t dt = esize == 8 ? ncclFloat64 : ncclFloat32;
    if (ncclGroupStart() != ncclSuccess) return -1;
    for (int p = 0; p < nranks; ++p) {
      if (scnt[p] > 0 &&
          ncclSend(static_cast<const char*>(sbuf) + soff[p] * esize, scnt[p], dt, p, c, st) !=
              ncclSuccess)
        return -2;
      if (rcnt[p] > 0 &&
          ncclRecv(static_cast<char*>(rbuf) + roff[p] * esize, rcnt[p], dt, p, c, st) !=
              ncclSuccess)
        return -3;
    }
    const ncclResult_t e = ncclGroupEnd();
    if (was_aborted.load()) return kErrAborted;
    return e == ncclSuccess ? 0 : -4;
  }
  int allreduce_sum(double* dev, int n, hipStream_t st) override {
    ncclComm_t c = comm.load();
    if (!c) return kErrNotConnected;
    if (was_aborted.load()) return kErrAborted;
    bdx::Watchdog::Busy b(wd.get());
    const ncclResult_t e = ncclAllReduce(dev, dev, n, ncclFloat64, ncclSum, c, st);
    if (was_aborted.load()) return kErrAborted;
    return e == ncclSuccess ? 0 : -5;
  }
  int wait(hipEvent_t ev) override {
    bdx::Watchdog::Busy b(wd.get());
    for (;;) {
      const hipError_t e = hipEventQuery(ev);
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotReady) return static_cast<int>(e);
      if (was_aborted.load()) return kErrAborted;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  }
  bool capturable() const override { return true; }
  int ranks() const override {
    ncclComm_t c = comm.load();
    int n = 0;
    if (!c || ncclCommCount(c, &n) != ncclSuccess) return -1;
    return n;
  }
};

// Emulated link (one rank of an N-rank run alone on this device: bench /
// scripts/emulate_rank.py).  Every exchange is a device copy of the send
// buffer into the receive buffer by a few workgroups (RCCL's p2p kernels
// occupy a few CUs the same way) that hold their CUs until the modelled link
// time has passed: max over peers of the bytes to or from that peer /
// link_gbps (one xGMI link per peer) + lat_us.  An all-reduce is a single
// workgroup held for allreduce_us.  The copies carry the rank's own face
// data, not a peer's: the emulation is for timing the schedule, not for
// results.  Bounded: each workgroup waits on the 100 MHz constant clock from
// its own start, nothing else.
__global__ void __launch_bounds__(256)
    bdx_link_emu_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16,
                        int64_t ticks) {
  const long long t0 = wall_clock64();
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n16;
       i += static_cast<int64_t>(gridDim.x) * 256)
    dst[i] = src[i];
  if (threadIdx.x == 0) {
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  }
  __syncthreads();
}

struct LinkEmuTransport final : Transport {
  int nranks = 1;
  double link_gbps = 50.0, lat_us = 10.0, allreduce_us = 20.0;
  int nwg = 8;
  static double env(const char* k, double d) {
    const char* e = std::getenv(k);
    return e ? std::atof(e) : d;
  }
  LinkEmuTransport() {
    link_gbps = env("BDX_EMU_LINK_GBPS", 50.0);
    lat_us = env("BDX_EMU_LINK_LAT_US", 10.0);
    allreduce_us = env("BDX_EMU_ALLREDUCE_US", 20.0);
    nwg = static_cast<int>(env("BDX_EMU_LINK_WG", 8));
    if (nwg < 1) nwg = 1;
  }
  // modelled link time of one exchange, microseconds
  double exchange_us(const std::vector<int64_t>& scnt, const std::vector<int64_t>& rcnt,
                     int esize) const {
    int64_t worst = 0;
    for (size_t p = 0; p < scnt.size() && p < rcnt.size(); ++p)
      worst = std::max(worst, std::max(scnt[p], rcnt[p]) * esize);
    if (worst == 0) return 0.0;
    return worst / (link_gbps * 1e3) + lat_us;  // bytes / (1e3 link_gbps) = us
  }
  int exchange(const void* sbuf, const std::vector<int64_t>& scnt,
               const std::vector<int64_t>& soff, void* rbuf, const std::vector<int64_t>& rcnt,
               const std::vector<int64_t>& roff, int esize, hipStream_t st) override {
    (void)soff;
    (void)roff;
    int64_t ns = 0, nr = 0;
    for (int64_t c : scnt) ns += c;
    for (int64_t c : rcnt) nr += c;
    const double us = exchange_us(scnt, rcnt, esize);
    if (us <= 0.0) return 0;
    const int64_t n16 = std::min(ns, nr) * esize / 16;
    hipLaunchKernelGGL(bdx_link_emu_kernel, dim3(nwg), dim3(256), 0, st,
                       static_cast<const uint4*>(sbuf), static_cast<uint4*>(rbuf), n16,
                       static_cast<int64_t>(us * 100.0));
    return static_cast<int>(hipGetLastError());
  }
  int allreduce_sum(double*, int, hipStream_t st) override {
    hipLaunchKernelGGL(bdx_link_emu_kernel, dim3(1), dim3(256), 0, st, nullptr, nullptr,
                       int64_t{0}, static_cast<int64_t>(allreduce_us * 100.0));
    return static_cast<int>(hipGetLastError());
  }
  bool capturable() const override { return true; }
  int ranks() const override { return nranks; }
};

// Single rank: no communication at all.
struct NoTransport final : Transport {
  int exchange(const void*, const std::vector<int64_t>&, const std::vector<int64_t>&, void*,
               const std::vector<int64_t>&, const std::vector<int64_t>&, int,
               hipStream_t) override {
    return 0;
  }
  int allreduce_sum(double*, int, hipStream_t) override { return 0; }
  bool capturable() const override { return true; }
  int ranks() const override { return 1; }
};

// R ranks = R threads of one process on one device (tests): host barriers,
// device-to-device copies from the peers' posted buffers, fixed-order sums.
struct ThreadGroupState {
  std::mutex m;
  std::condition_variable cv;
  int size = 0, arrived = 0;
  long generation = 0;
  std::vector<const void*> sbuf;
  std::vector<const std::vector<int64_t>*> soff;
  std::vector<hipEvent_t> packed, copied;
  std::vector<double*> red;
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    const long gen = generation;
    if (++arrived == size) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != gen; });
    }
  }
};
std::mutex g_groups_m;
// found by group id while a runtime of the group holds it (runtime.hip:
// init_common joins, bdx_rt_release_group drops the expired entry)
std::map<int64_t, std::weak_ptr<ThreadGroupState>> g_groups;

// The exchange is stream-ordered, as RCCL's: the host only swaps buffer
// pointers and event handles at two barriers and never waits for the device,
// so the compute stream's interior tiles really run while the copies do.
//   1. record `packed` on the caller's stream (after the pack kernel);
//   2. barrier: every rank's send buffer / offsets / `packed` are published;
//   3. per peer: wait for its `packed`, copy its slice into the receive buffer;
//      record `copied`;
//   4. barrier: every `copied` is published; wait for the `copied` of each
//      peer that reads this rank's send buffer, so a later write to it (the
//      next pack, stream-ordered after this) cannot overtake their copies.
// Event reuse is safe: a rank re-records `packed` only after barrier 2 of
// the previous exchange (every peer's wait on it was issued before that
// barrier) and `copied` only after barrier 1 of the next exchange (every
// peer issues its wait on it before arriving there).
struct ThreadTransport final : Transport {
  std::shared_ptr<ThreadGroupState> g;
  int rank = 0;
  hipEvent_t ev_packed = nullptr, ev_copied = nullptr;
  ~ThreadTransport() override {
    if (ev_packed) hipEventDestroy(ev_packed);
    if (ev_copied) hipEventDestroy(ev_copied);
  }
  int exchange(const void* sbuf, const std::vector<int64_t>& scnt,
               const std::vector<int64_t>& soff, void* rbuf, const std::vector<int64_t>& rcnt,
               const std::vector<int64_t>& roff, int esize, hipStream_t st) override {
    if (!ev_packed) {
      BDX_CHECK(hipEventCreateWithFlags(&ev_packed, hipEventDisableTiming));
      BDX_CHECK(hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming));
    }
    BDX_CHECK(hipEventRecord(ev_packed, st));
    g->sbuf[rank] = sbuf;
    g->soff[rank] = &soff;
    g->packed[rank] = ev_packed;
    g->barrier();
    for (int p = 0; p < g->size; ++p) {
      if (rcnt[p] <= 0) continue;
      const char* src = static_cast<const char*>(g->sbuf[p]) + (*g->soff[p])[rank] * esize;
      BDX_CHECK(hipStreamWaitEvent(st, g->packed[p], 0));
      BDX_CHECK(hipMemcpyAsync(static_cast<char*>(rbuf) + roff[p] * esize, src, rcnt[p] * esize,
                               hipMemcpyDeviceToDevice, st));
    }
    BDX_CHECK(hipEventRecord(ev_copied, st));
    g->copied[rank] = ev_copied;
    g->barrier();
    for (int p = 0; p < g->size; ++p)
      if (scnt[p] > 0) BDX_CHECK(hipStreamWaitEvent(st, g->copied[p], 0));
    return 0;
  }
  int allreduce_sum(double* dev, int n, hipStream_t st) override {
    BDX_CHECK(hipStreamSynchronize(st));
    g->red[rank] = dev;
    g->barrier();
    std::vector<double> acc(n, 0.0), v(n);
    for (int p = 0; p < g->size; ++p) {  // fixed rank order: deterministic
      BDX_CHECK(hipMemcpy(v.data(), g->red[p], n * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) acc[i] += v[i];
    }
    g->barrier();
    BDX_CHECK(hipMemcpy(dev, acc.data(), n * sizeof(double), hipMemcpyHostToDevice));
    g->barrier();
    return 0;
  }
  bool capturable() const override { return false; }
  int ranks() const override { return g->size; }
};

}  // namespace
