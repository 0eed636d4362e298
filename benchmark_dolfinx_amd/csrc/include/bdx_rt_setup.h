// Setup and result records of the native CG runtimes (csrc/hip/runtime.hip),
// part of the C ABI of libbdx_hip.so (bdx_hip_api.h includes this file).
//
// Python fills a setup record field by field (solvers/native.py) through the
// ctypes mirrors of ops/hip_api.py; tests/test_abi_layouts.py compares every
// mirror with these structs (names, order, offsets, sizes).  A record only has
// to live for the call: the runtime copies what it keeps.  Field names are
// those of the members of CGRuntime, DofCGRuntime and LoopBase they fill; a
// pointer is void* only where its element type is the runtime's T.  A new
// buffer or flag of a runtime is one field here plus one field of the mirror.
// Readable by g++ without HIP.
#pragma once
#include <cstdint>

#include "bdx_lattice.h"

// Transport of a runtime (BdxRtHalo::transport); with one rank it is none.
enum BdxTransport {
  kBdxTransportNone = 0,
  kBdxTransportRccl = 1,      // one process per GPU; connected by bdx_rt_connect
  kBdxTransportThread = 2,    // ranks are threads of one process on one GPU
  kBdxTransportEmulated = 3,  // one rank alone, modelled links
};

// Geometry of an operator (the `geom` argument and field): factors stored per
// cell, or computed on the fly from the vertex coordinates.
enum { kGeomStored = 0, kGeomOTF = 1 };

// The plane halo and the transport (LoopBase::init_common).
struct BdxRtHalo {
  void* buf_a;  // T: pack / receive buffers
  void* buf_b;
  const int64_t* face_boxes;  // device box tables (bdx_box_copy_lat)
  const int64_t* ghost_boxes;
  const int64_t* face_cnt;  // host, nranks values each: values per peer
  const int64_t* ghost_cnt;
  int nface_boxes;
  int64_t face_total;
  int nghost_boxes;
  int64_t ghost_total;
  int transport;  // BdxTransport
  int nranks;
  int rank;
  int64_t group_id;  // thread transport: the group's key
};

// bdx_rt_create: the fused structured CG loop.
struct BdxRtFusedSetup {
  int64_t latd[kLatticeWords];
  int64_t latd_tiled[kLatticeWords];  // all zero: the loop runs on the lattice layout
  int64_t own[3];
  int is_f64;
  int version, affine, P, nq;
  int nblocks;  // nty * ntz * nseg p.Ap partials
  int nty, ntz, sy, sz;
  int nseg;  // < 1: 1
  int use_graph, overlap;
  double kappa;
  const double* wts;  // host, nq values each
  const double* qpts;
  const void* tabs;  // T: host tables (fused2 / fused3), the device table buffer (fused5)
  void* x;
  void* r;
  void* p_a;
  void* p_b;
  void* y;
  void* yb;
  void* zb;
  void* cb;
  const void* xv;
  const void* kc;  // may be null
  double* scal;
  double* partials;
  double* upart;
  // tiled copies of x, r, p_a, p_b, y (zeroed by the caller); read only with a
  // tiled descriptor
  void* xt;
  void* rt;
  void* pat;
  void* pbt;
  void* yt;
  BdxRtHalo halo;
};

// bdx_rt_create_dofmap: the dofmap data model's CG loop.
struct BdxRtDofmapSetup {
  int64_t latd[kLatticeWords];
  int is_f64;
  int P, nq, geom, n_inner, n_outer;
  int use_graph, overlap;
  int64_t nvec;
  double kappa;
  void* x;
  void* r;
  void* p_a;
  void* p_b;
  void* y;
  double* scal;
  double* partials;
  double* upart;
  const void* tab;
  const int* inner;
  const int* outer;
  const int* cdofs;
  const int* cverts;
  const void* coords;
  const unsigned char* flags;
  const void* G;   // may be null unless the geometry is stored
  const void* kc;  // may be null
  BdxRtHalo halo;
};

// bdx_rt_profile: mean ms per eager iteration.
struct BdxRtPhases {
  double halo_fwd;     // forward halo (comm stream: pack, exchange, unpack)
  double op_interior;  // operator, interior tiles / cells (serial: the first launch)
  // split: ghost-touching tiles / cells (+ ghost fold) after the forward halo;
  // serial: what follows the first launch
  double op_boundary;
  double halo_rev;              // reverse halo (pack, exchange; serial: + unpack-add)
  double join_rev_add;          // interior done -> comm stream joined, received sums added
  double reduce_allreduce_pap;  // reduce + all-reduce(p.Ap)
  double update_rr;             // r update + r.r
  double allreduce_rr;          // all-reduce(r.r)
  double iteration;             // whole iteration
  // offsets from the iteration start: the comm-stream chain (forward exchange,
  // boundary work, reverse send) is hidden when it ends before the interior
  // work on the compute stream does
  double t_halo_fwd_done;
  double t_boundary_done;
  double t_halo_rev_done;
  double t_op_interior_done;
};

// bdx_rt_overlap_probe: medians over the repetitions, ms.
struct BdxRtOverlapProbe {
  double chain_alone_ms;
  double interior_alone_ms;
  double chain_done_ms;  // this and the next: measured from the common fork
  double interior_done_ms;
  double exchange_alone_ms;
  double fwd_exchange_done_ms;
};

// bdx_rt_preflight: host ms of the exchange and the all-reduce of (rank + 1),
// and that sum (n (n + 1) / 2 when every rank took part).
struct BdxRtPreflight {
  double ms;
  double allreduce;
};

// bdx_rt_comm_priority: the device's range and the comm stream's own.
struct BdxRtCommPriority {
  int least;
  int greatest;
  int comm_stream;
};

// What bdx_rt_create refuses without looking at the HIP library: no tables; a
// tiled descriptor for a kernel that does not address tiled storage, with a
// tile other than the kernel's, or without its buffers.  Nothing is
// dereferenced.
inline bool bdx_rt_fused_setup_ok(const BdxRtFusedSetup& s) {
  if (!s.tabs) return false;
  const BdxLattice t = BdxLattice::from(s.latd_tiled);
  if (!t.tsy) return true;
  // only the x-march kernels whose tile is the storage tile address it
  if ((s.version != 3 && s.version != 5) || t.tsy != s.sy || t.tsz != s.sz) return false;
  return s.xt && s.rt && s.pat && s.pbt && s.yt;
}

// The same for bdx_rt_create_dofmap.
inline bool bdx_rt_dofmap_setup_ok(const BdxRtDofmapSetup& s) {
  return s.tab && s.cdofs && s.flags && (s.geom != kGeomStored || s.G);
}
