// The r-update pass of the fused CG loops (bdx_cg_update_*, bdx_pcg_update_*):
//   alpha = s[rn] / s[pap];  r -= alpha (y + interface partials);  partial r.r
// on the lattice layout (flat kernel) and on the tiled storage (two kernels),
// over IfaceLayout (bdx_common.h), TileDecode and UpdSums; one host launcher
// per storage kind (update_flat, update_tiled).
#include <cstdlib>
#include "bdx_common.h"

// kPartialsCap is the partials capacity every caller provides
// (bdx_hip_partials_size).  The flat update pass wants a non-persistent grid (a persistent 8192/16384-block
// grid-stride version measured 1.70 ms vs 1.52 at Q3); its up to 65280 block
// partials are summed in two fixed-order stages (256 slices into the last 256
// slots of the partials buffer, then one block): deterministic like the rest.
constexpr int kPartialsCap = 65536, kStage1 = 256;
constexpr int kUpdGrid = kPartialsCap - kStage1;  // update pass grid cap
constexpr int kUpdU = 2;  // vectors per thread of the tiled update pass
constexpr bool kUpdPre = true;  // cg_update_tiled_pre_kernel (interface loads issued up front)

// The extra arguments of the Jacobi-preconditioned update passes (PC below):
// the update kernels take them as an optional trailing argument, so the
// unpreconditioned instances (no such argument) are the kernels they were.
template <typename T>
struct PcArgs {
  const T* dinv;        // 1 / diag(A), in the layout of r
  T* z;                 // z = dinv . r, in the layout of r
  double* partials_rr;  // block partials of r.r (`partials` carries r.z)
};

// One thread's sums of an update pass, the per-element update that feeds them
// and the block epilogue that stores them.
template <typename T, bool PC>
struct UpdSums {
  double acc = 0.0;     // r.r; PC: r.z
  double acc_rr = 0.0;  // PC: r.r
  // Element w of the vector vr, given its folded t = y + YB + ZB + CB: where
  // `own`, vr[w] -= alpha t and the new value's terms join the sums (PC: vd is
  // the vector's dinv); elsewhere vr[w] stays as read.
  template <typename V>
  __device__ __forceinline__ void elem(V& vr, [[maybe_unused]] const V& vd, int w, T alpha, T t,
                                       bool own = true) {
    const T rn = vr[w] - alpha * t;
    if (!own) return;
    vr[w] = rn;
    if constexpr (PC) {
      const T zn = vd[w] * rn;  // the value the pass stores in z
      acc += static_cast<double>(rn) * static_cast<double>(zn);
      acc_rr += static_cast<double>(rn) * static_cast<double>(rn);
    } else {
      acc += static_cast<double>(rn) * static_cast<double>(rn);
    }
  }
  // block sums -> partials[blockIdx.x] (PC: and pc.partials_rr[blockIdx.x])
  __device__ __forceinline__ void store(double* __restrict__ partials,
                                        [[maybe_unused]] const PcArgs<T>& pc) const {
    __shared__ double lds[16];
    const double t = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if constexpr (PC) {
      __shared__ double lds_rr[16];
      const double t2 = block_sum(acc_rr, lds_rr);
      if (threadIdx.x == 0) pc.partials_rr[blockIdx.x] = t2;
    }
  }
};

// CG update of the fused2..5 paths: alpha = s[rn] / s[pap];
//   r -= alpha (y + interface partials);  partial r.r
// The tile-interface partials (YB/ZB/CB) are folded here on the fly instead of
// by a separate finalize pass over y (same sum as fused_finalize_kernel).
// x is not touched: its update x += alpha p is lagged into the next fused
// launch (staging reads p there anyway) and flushed by bdx_xflush at the end.
// Flat pass (a row-per-wave kernel measured slower): the owned rows j < o1 of an
// x-plane are one contiguous block of o1 * ld elements (row pitch ld, a
// multiple of 16 elements: no 16-byte vector straddles two rows), so the pass
// runs as a plain stream -- one chunk of 256 threads x 2 vectors per block,
// blocks up to the partials capacity (grid-stride beyond), both loads of a
// thread in flight before any arithmetic.  Same arithmetic per element as the
// row kernel above (fold, r update, r.r); columns k >= o2 are left as read.
//
// PC (Jacobi-preconditioned CG, bdx_pcg_update_*): the same fold and r update,
// bit for bit; the pass also streams dinv (loaded with y and r, before any
// arithmetic), stores z = dinv . r for every vector it stores r for (all W
// lanes: the lanes the r update leaves as read carry dinv times the r read,
// ghost planes of z are overwritten by the next forward exchange), and sums
// r.z into `partials` and r.r into `partials_rr` over the owned nodes.
// Without the trailing PcArgs this is the unpreconditioned pass.
template <typename T, typename... PA>
__global__ void __launch_bounds__(256)
    cg_update_flat_kernel(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                          int64_t Lz, T* __restrict__ r, const T* __restrict__ y,
                          const T* __restrict__ yb, const T* __restrict__ zb,
                          const T* __restrict__ cb, int nty, int ntz, int sy, int sz,
                          const double* __restrict__ scal, int rn_slot, int pap_slot,
                          double* __restrict__ partials, PA... pa) {
  constexpr bool PC = sizeof...(PA) != 0;
  [[maybe_unused]] const PcArgs<T> pc{pa...};  // no argument: all null
  const IfaceLayout F{0, L1, Lz, nty, ntz};  // one plane's indices: Lx is not used
  const T alpha = static_cast<T>(scal[rn_slot] / scal[pap_slot]);
  constexpr int W = 16 / sizeof(T), U = 2, CH = 256 * U;
  typedef T V __attribute__((ext_vector_type(W)));
  const int ldv = static_cast<int>(ld / W);
  const int nvp = static_cast<int>(o1) * ldv;
  const int nch = (nvp + CH - 1) / CH;
  const int64_t nwork = o0 * nch;
  const float inv_sz = 1.0f / static_cast<float>(sz);
  const float inv_ldv = 1.0f / static_cast<float>(ldv);
  UpdSums<T, PC> sums;
  for (int64_t c = blockIdx.x; c < nwork; c += gridDim.x) {
    const int64_t i = c / nch;
    const int v0 = static_cast<int>(c - i * nch) * CH + static_cast<int>(threadIdx.x) * U;
    const int64_t pbase = i * L1 * ld;
    V vy[U], vr[U];
    [[maybe_unused]] V vd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (v0 + u < nvp) {
        vy[u] = ld_stream(reinterpret_cast<const V*>(y + pbase + static_cast<int64_t>(v0 + u) * W));
        vr[u] = ld_stream(reinterpret_cast<const V*>(r + pbase + static_cast<int64_t>(v0 + u) * W));
        if constexpr (PC)
          vd[u] = ld_stream(reinterpret_cast<const V*>(pc.dinv + pbase + static_cast<int64_t>(v0 + u) * W));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = v0 + u;
      if (v >= nvp) continue;
      int j = static_cast<int>(static_cast<float>(v) * inv_ldv);
      if (j * ldv > v) --j;
      if ((j + 1) * ldv <= v) ++j;
      const int k0 = (v - j * ldv) * W;
      const int tyy = j / sy;
      const int yrow = (j - tyy * sy == 0 && tyy >= 1 && tyy < nty) ? tyy - 1 : -1;
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const int k = k0 + e;
        if (k >= o2) continue;
        T t = vy[u][e];
        if (yrow >= 0) t += yb[F.yb(i, yrow, k)];
        int zq = static_cast<int>(static_cast<float>(k) * inv_sz);
        if (zq * sz > k) --zq;
        if ((zq + 1) * sz <= k) ++zq;
        if (zq * sz == k && zq >= 1 && zq < ntz) {
          t += zb[F.zb(i, zq - 1, j)];
          if (yrow >= 0) t += cb[F.cb(i, yrow, zq - 1)];
        }
        sums.elem(vr[u], vd[u], e, alpha, t);
      }
      st_stream(reinterpret_cast<V*>(r + pbase + static_cast<int64_t>(v) * W), vr[u]);
      if constexpr (PC)
        st_stream(reinterpret_cast<V*>(pc.z + pbase + static_cast<int64_t>(v) * W), vd[u] * vr[u]);
    }
  }
  sums.store(partials, pc);
}

// Tiled storage (bdx_lattice.h, tsy != 0): where the 16-byte vector that starts
// at element e0 lies.  Chunks of tsy * tsz elements are one tile's patch of one
// x-plane, chunk c = (tY tntz + tZ) L0 + x.  Reciprocals with exact fix-ups:
// the chunk in double (e0 is 64-bit), chunk -> (tile, x) and the in-chunk row
// in 32-bit arithmetic with float reciprocals (chunks < 2^31; round 4: it was
// two 64-bit divisions per vector).
struct TileDecode {
  struct Pos {
    int x, tY, tZ;  // x-plane, storage tile
    int ly, lz;     // (y, z) of the vector's first element within the tile
    bool in;        // x is an owned plane (and, BDX_DEBUG=1, the vector in range)
  };
  int64_t ch, o0, nelem;
  double inv_ch;
  float inv_l0, inv_tntz, inv_tsz;
  int l0, tsz, tntz;
  __device__ __forceinline__ TileDecode(int64_t L0, int tsy, int tsz_, int tntz_, int64_t o0_,
                                        int64_t nelem_)
      : ch(static_cast<int64_t>(tsy) * tsz_), o0(o0_), nelem(nelem_),
        inv_ch(1.0 / static_cast<double>(ch)), inv_l0(1.0f / static_cast<float>(L0)),
        inv_tntz(1.0f / static_cast<float>(tntz_)), inv_tsz(1.0f / static_cast<float>(tsz_)),
        l0(static_cast<int>(L0)), tsz(tsz_), tntz(tntz_) {}
  template <int W>
  __device__ __forceinline__ Pos at(int64_t e0) const {
    int64_t c = static_cast<int64_t>(static_cast<double>(e0) * inv_ch);  // chunk
    if (c * ch > e0) --c;
    if ((c + 1) * ch <= e0) ++c;
    const int ci = static_cast<int>(c);
    int blk = static_cast<int>(static_cast<float>(ci) * inv_l0);
    while (blk * l0 > ci) --blk;
    while ((blk + 1) * l0 <= ci) ++blk;
    const int x = ci - blk * l0;
    int tY = static_cast<int>(static_cast<float>(blk) * inv_tntz);
    while (tY * tntz > blk) --tY;
    while ((tY + 1) * tntz <= blk) ++tY;
    const int tZ = blk - tY * tntz;
    const int ein = static_cast<int>(e0 - c * ch);
    int ly = static_cast<int>(static_cast<float>(ein) * inv_tsz);
    if (ly * tsz > ein) --ly;
    if ((ly + 1) * tsz <= ein) ++ly;
    const bool in = x < o0 && !BDX_OOB(e0 + W - 1, nelem, "tiled update");
    return Pos{x, tY, tZ, ly, ein - ly * tsz, in};
  }
};

// The r update of the tiled storage (bdx_lattice.h, tsy != 0): the same
// arithmetic per node as the flat kernel above, in the layout's element order.
// Chunks of tsy * tsz elements are one tile's patch of one x-plane; a vector
// of W elements never straddles a chunk (tsy * tsz * sizeof(T) is a multiple
// of 16 bytes, checked by the host wrapper).  ROW: tsz is a multiple of W as
// well, so a vector lies in one z-row of its chunk and its position, owned
// mask and y-interface term are resolved once per vector instead of once per
// element.  Used for FP32 (4 elements per 16-byte vector): Q6 FP32 update
// 1.58 -> 1.41 ms, +3 % GDoF/s; FP64 keeps the per-element form (ROW: Q3
// update 1.555 -> 1.583 ms), same box (scripts/r3_updrow.sh).  Blocks stay in
// launch order: an XCD-aware remap (contiguous slabs per XCD) made the pass
// 8-40 % slower (Q6 FP64 update 2.54 -> 3.54 ms, scripts/r3_updxcd.sh).
// Round 4: U = 2 vectors per thread with both loads in flight, and the chunk ->
// (tile, x) split in 32-bit arithmetic (it was two 64-bit divisions per
// vector): update pass Q3 1.79 -> 1.54 ms, Q6 2.76 -> 2.59, Q6 FP32 1.58 ->
// 1.37, same box (U = 1: 1.57 at Q3, U = 4: no gain;
// profiles/r4_update_pass_ab.txt).  The pass's r / y loads and r stores are
// non-temporal (whole 16-byte vectors, full lines; unlike the operator's
// march, nothing here relies on L2 merging partial rows): update Q3 1.53 ->
// 1.46 ms, Q6 FP64 2.50 -> 2.30, +1.6-1.8 % GDoF/s same box (same file).
// PC: the preconditioned pass (see cg_update_flat_kernel): dinv streamed with y
// and r, z = dinv . r stored wherever r is stored, r.z and r.r summed.
template <typename T, bool ROW, int U, typename... PA>
__global__ void __launch_bounds__(256)
    cg_update_tiled_kernel(int64_t L0, int64_t L1, int64_t Lz, int tsy, int tsz, int tntz,
                           int64_t o0, int64_t o1, int64_t o2, int64_t nvec, T* __restrict__ r,
                           const T* __restrict__ y, const T* __restrict__ yb,
                           const T* __restrict__ zb, const T* __restrict__ cb, int nty, int ntz,
                           const double* __restrict__ scal, int rn_slot, int pap_slot,
                           double* __restrict__ partials, PA... pa) {
  constexpr bool PC = sizeof...(PA) != 0;
  [[maybe_unused]] const PcArgs<T> pc{pa...};  // no argument: all null
  const IfaceLayout F{L0, L1, Lz, nty, ntz};
  const T alpha = static_cast<T>(scal[rn_slot] / scal[pap_slot]);
  constexpr int W = 16 / sizeof(T);
  typedef T V __attribute__((ext_vector_type(W)));
  const TileDecode dec(L0, tsy, tsz, tntz, o0, nvec * W);
  UpdSums<T, PC> sums;
  for (int64_t vb = static_cast<int64_t>(blockIdx.x) * (256 * U) + threadIdx.x; vb < nvec;
       vb += static_cast<int64_t>(gridDim.x) * (256 * U)) {
    // U vectors per thread, 256 apart (each load coalesced over the block), all
    // loads in flight before the index math and the arithmetic
    V vyu[U], vru[U];
    [[maybe_unused]] V vdu[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = vb + u * 256;
      if (v < nvec) {
        vyu[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(y + v * W));
        vru[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(r + v * W));
        if constexpr (PC)
          vdu[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(pc.dinv + v * W));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = vb + u * 256;
      if (v >= nvec) break;
      const int64_t e0 = v * W;
      const TileDecode::Pos p = dec.at<W>(e0);
      if (!p.in) continue;
      const int x = p.x, tY = p.tY, tZ = p.tZ;
      V vr = vru[u];
      if constexpr (ROW) {
        const int ly = p.ly, lz0 = p.lz;
        const int64_t gy = static_cast<int64_t>(tY) * tsy + ly, gz0 = static_cast<int64_t>(tZ) * tsz + lz0;
        if (gy >= o1 || gz0 >= o2) continue;
        V t = vyu[u];
        const int yrow = (ly == 0 && tY >= 1 && tY < nty) ? tY - 1 : -1;
        const int nw = o2 - gz0 < W ? static_cast<int>(o2 - gz0) : W;  // owned elements
        if (yrow >= 0) {
          const T* yr = yb + F.yb(x, yrow, gz0);
#pragma unroll
          for (int w = 0; w < W; ++w)
            if (w < nw) t[w] += yr[w];
        }
        if (lz0 == 0 && tZ >= 1 && tZ < ntz) {
          t[0] += zb[F.zb(x, tZ - 1, gy)];
          if (yrow >= 0) t[0] += cb[F.cb(x, yrow, tZ - 1)];
        }
#pragma unroll
        for (int w = 0; w < W; ++w) sums.elem(vr, vdu[u], w, alpha, t[w], w < nw);
        __builtin_nontemporal_store(vr, reinterpret_cast<V*>(r + e0));
        if constexpr (PC) __builtin_nontemporal_store(vdu[u] * vr, reinterpret_cast<V*>(pc.z + e0));
      } else {
        const V vy = vyu[u];
        bool any = false;
        // the other elements step along z
        int ly = p.ly, lz = p.lz - 1;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          if (++lz == tsz) {
            lz = 0;
            ++ly;
          }
          const int64_t gy = static_cast<int64_t>(tY) * tsy + ly, gz = static_cast<int64_t>(tZ) * tsz + lz;
          if (gy >= o1 || gz >= o2) continue;
          any = true;
          const int yrow = (ly == 0 && tY >= 1 && tY < nty) ? tY - 1 : -1;
          T t = vy[w];
          if (yrow >= 0) t += yb[F.yb(x, yrow, gz)];
          if (lz == 0 && tZ >= 1 && tZ < ntz) {
            t += zb[F.zb(x, tZ - 1, gy)];
            if (yrow >= 0) t += cb[F.cb(x, yrow, tZ - 1)];
          }
          sums.elem(vr, vdu[u], w, alpha, t);
        }
        if (any) __builtin_nontemporal_store(vr, reinterpret_cast<V*>(r + e0));
        if constexpr (PC) {
          if (any) __builtin_nontemporal_store(vdu[u] * vr, reinterpret_cast<V*>(pc.z + e0));
        }
      }
    }
  }
  sums.store(partials, pc);
}

// The tiled r update with the tile-interface partials loaded together with
// the vector's y and r (round 5): in cg_update_tiled_kernel they are loaded
// inside the branches that need them, after the wave has waited for y and r,
// so every vector next to a tile interface (a third of them in FP32 at Q6)
// pays a second memory latency.  Here every load of a pass -- y, r and the
// YB / ZB / CB terms of each element -- is issued first, as range-checked
// buffer loads whose offset is out of range (the load returns 0, no memory
// access) where an element has no such term; the arithmetic follows.  Same
// sums in the same order as cg_update_tiled_kernel.
// PC: the preconditioned pass (see cg_update_flat_kernel); dinv is loaded with y
// and r, ahead of the interface loads.
template <typename T, bool ROW, int U, typename... PA>
__global__ void __launch_bounds__(256)
    cg_update_tiled_pre_kernel(int64_t L0, int64_t L1, int64_t Lz, int tsy, int tsz, int tntz,
                               int64_t o0, int64_t o1, int64_t o2, int64_t nvec, T* __restrict__ r,
                               const T* __restrict__ y, const T* yb, const T* zb, const T* cb,
                               int nty, int ntz, const double* __restrict__ scal, int rn_slot,
                               int pap_slot, double* __restrict__ partials, PA... pa) {
  constexpr bool PC = sizeof...(PA) != 0;
  [[maybe_unused]] const PcArgs<T> pc{pa...};  // no argument: all null
  const IfaceLayout F{L0, L1, Lz, nty, ntz};
  const T alpha = static_cast<T>(scal[rn_slot] / scal[pap_slot]);
  constexpr int W = 16 / sizeof(T);
  constexpr int NI = ROW ? W + 2 : 3 * W;  // interface loads per vector
  typedef T V __attribute__((ext_vector_type(W)));
  constexpr unsigned kOOB = 0xfffffff0u;
  auto rsrc = [](const T* ptr, int64_t n) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(ptr), 0,
                                             static_cast<int>(n * static_cast<int64_t>(sizeof(T))),
                                             0x00020000);
  };
  const auto rs_yb = rsrc(yb, F.yb_size()), rs_zb = rsrc(zb, F.zb_size()),
             rs_cb = rsrc(cb, F.cb_size());
  auto ldb = [](__amdgpu_buffer_rsrc_t rs, unsigned off) -> T {
    if constexpr (sizeof(T) == 8)
      return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
    else
      return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
  };
  auto bo = [](bool on, int64_t e) { return on ? static_cast<unsigned>(e * sizeof(T)) : kOOB; };
  const TileDecode dec(L0, tsy, tsz, tntz, o0, nvec * W);
  UpdSums<T, PC> sums;
  for (int64_t vb = static_cast<int64_t>(blockIdx.x) * (256 * U) + threadIdx.x; vb < nvec;
       vb += static_cast<int64_t>(gridDim.x) * (256 * U)) {
    V vyu[U], vru[U];
    [[maybe_unused]] V vdu[U];
    T ia[U][NI];
    int own[U];  // bit w: element w is owned
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = vb + u * 256;
      own[u] = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i) ia[u][i] = T(0);
      if (v >= nvec) continue;
      vyu[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(y + v * W));
      vru[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(r + v * W));
      if constexpr (PC)
        vdu[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(pc.dinv + v * W));
      const TileDecode::Pos p = dec.at<W>(v * W);
      const int x = p.x, tY = p.tY, tZ = p.tZ;
      const bool zt = tZ >= 1 && tZ < ntz;
      if constexpr (ROW) {
        const int ly = p.ly, lz0 = p.lz;
        const int64_t gy = static_cast<int64_t>(tY) * tsy + ly, gz0 = static_cast<int64_t>(tZ) * tsz + lz0;
        const bool row = p.in && gy < o1;
        const int yrow = (ly == 0 && tY >= 1 && tY < nty) ? tY - 1 : -1;
#pragma unroll
        for (int w = 0; w < W; ++w) own[u] |= (row && gz0 + w < o2) ? 1 << w : 0;
        // the vector's YB terms: one 16-byte load when they lie in one YB row
        // (dword-aligned offsets are allowed; the terms of unowned elements
        // are loaded but not applied), else one load per owned element
        const bool yneed = row && gz0 < o2 && yrow >= 0;
        const int64_t ye = F.yb(x, yrow, gz0);
        if (gz0 + W <= Lz) {
          const V yv = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rs_yb, bo(yneed, ye), 0, 0));
#pragma unroll
          for (int w = 0; w < W; ++w) ia[u][w] = yv[w];
        } else {
#pragma unroll
          for (int w = 0; w < W; ++w) ia[u][w] = ldb(rs_yb, bo(yneed && gz0 + w < o2, ye + w));
        }
        const bool z0 = row && gz0 < o2 && lz0 == 0 && zt;
        ia[u][W] = ldb(rs_zb, bo(z0, F.zb(x, tZ - 1, gy)));
        ia[u][W + 1] = ldb(rs_cb, bo(z0 && yrow >= 0, F.cb(x, yrow, tZ - 1)));
      } else {
        int ly = p.ly, lz = p.lz - 1;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          if (++lz == tsz) {
            lz = 0;
            ++ly;
          }
          const int64_t gy = static_cast<int64_t>(tY) * tsy + ly, gz = static_cast<int64_t>(tZ) * tsz + lz;
          const bool on = p.in && gy < o1 && gz < o2;
          own[u] |= on ? 1 << w : 0;
          const int yrow = (ly == 0 && tY >= 1 && tY < nty) ? tY - 1 : -1;
          const bool zf = on && lz == 0 && zt;
          ia[u][3 * w] = ldb(rs_yb, bo(on && yrow >= 0, F.yb(x, yrow, gz)));
          ia[u][3 * w + 1] = ldb(rs_zb, bo(zf, F.zb(x, tZ - 1, gy)));
          ia[u][3 * w + 2] = ldb(rs_cb, bo(zf && yrow >= 0, F.cb(x, yrow, tZ - 1)));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = vb + u * 256;
      if (v >= nvec || !own[u]) continue;
      V vr = vru[u];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        T t = vyu[u][w];
        if constexpr (ROW) {  // the order of cg_update_tiled_kernel: y + YB, + ZB, + CB
          t += ia[u][w];
          if (w == 0) {
            t += ia[u][W];
            t += ia[u][W + 1];
          }
        } else {
          t += ia[u][3 * w];
          t += ia[u][3 * w + 1];
          t += ia[u][3 * w + 2];
        }
        sums.elem(vr, vdu[u], w, alpha, t, own[u] & (1 << w));
      }
      __builtin_nontemporal_store(vr, reinterpret_cast<V*>(r + v * W));
      if constexpr (PC) __builtin_nontemporal_store(vdu[u] * vr, reinterpret_cast<V*>(pc.z + v * W));
    }
  }
  sums.store(partials, pc);
}

// stage 1 of the two-stage sum: block b sums slice b of partials[0, n) into out[b]
__global__ void reduce_partials_slices(const double* __restrict__ partials, int n,
                                       double* __restrict__ out) {
  __shared__ double lds[16];
  const int per = (n + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x);
  const int lo = static_cast<int>(blockIdx.x) * per, hi = lo + per < n ? lo + per : n;
  double acc = 0.0;
  for (int i = lo + static_cast<int>(threadIdx.x); i < hi; i += blockDim.x) acc += partials[i];
  const double t = block_sum(acc, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// Fixed-order sum of the per-tile p.Ap partials into one device scalar slot.
__global__ void reduce_partials_fixed(const double* __restrict__ partials, int n,
                                      double* __restrict__ out, int slot) {
  __shared__ double lds[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  const double t = block_sum(acc, lds);
  if (threadIdx.x == 0) out[slot] = t;
}

// Fixed-order sum of the g block partials of an update pass into scal[slot]
// (two stages above 4 kStage1 partials).
static void reduce_update_partials(double* partials, int g, double* scal, int slot,
                                   hipStream_t st) {
  if (g > 4 * kStage1) {
    double* stage = partials + kPartialsCap - kStage1;
    reduce_partials_slices<<<kStage1, 256, 0, st>>>(partials, g, stage);
    reduce_partials_fixed<<<1, 256, 0, st>>>(stage, kStage1, scal, slot);
  } else {
    reduce_partials_fixed<<<1, 256, 0, st>>>(partials, g, scal, slot);
  }
}

// The tail of both launchers: the pass's block partials -> scal[out_slot]
// (PC: r.z there, and r.r -> scal[rr_slot]).
template <typename T, typename... PA>
static int reduce_update(int g, double* scal, double* partials, int out_slot, int rr_slot,
                         hipStream_t st, PA... pa) {
  reduce_update_partials(partials, g, scal, out_slot, st);
  if constexpr (sizeof...(PA) != 0)
    reduce_update_partials(PcArgs<T>{pa...}.partials_rr, g, scal, rr_slot, st);
  return static_cast<int>(hipGetLastError());
}

static int update_grid(int64_t want) {
  return static_cast<int>(want < kUpdGrid ? (want > 0 ? want : 1) : kUpdGrid);
}

// The update pass on the lattice layout: one block per chunk of 512 vectors of
// an x-plane's owned rows.  pa: nothing (CG) or one PcArgs<T> (Jacobi PCG).
template <typename T, typename... PA>
static int update_flat(const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb,
                       const T* zb, const T* cb, int nty, int ntz, int sy, int sz, double* scal,
                       int rn_slot, int pap_slot, int out_slot, int rr_slot, double* partials,
                       hipStream_t st, PA... pa) {
  const BdxLattice lat = BdxLattice::from(latd);
  const int64_t nvp = own[1] * (lat.ld * static_cast<int64_t>(sizeof(T)) / 16);
  const int g = update_grid(own[0] * ((nvp + 511) / 512));
  cg_update_flat_kernel<T, PA...><<<g, 256, 0, st>>>(
      lat.L[1], lat.ld, own[0], own[1], own[2], lat.L[2], r, y, yb, zb, cb, nty, ntz, sy, sz,
      scal, rn_slot, pap_slot, partials, pa...);
  return reduce_update<T>(g, scal, partials, out_slot, rr_slot, st, pa...);
}

template <typename T, bool ROW, typename... PA>
static auto tiled_kernel(bool pre) {
  return pre ? cg_update_tiled_pre_kernel<T, ROW, kUpdU, PA...>
             : cg_update_tiled_kernel<T, ROW, kUpdU, PA...>;
}

// The update pass on the tiled storage: kUpdU vectors per thread.
template <typename T, typename... PA>
static int update_tiled(const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb,
                        const T* zb, const T* cb, int nty, int ntz, double* scal, int rn_slot,
                        int pap_slot, int out_slot, int rr_slot, double* partials, hipStream_t st,
                        PA... pa) {
  const BdxLattice L = BdxLattice::from(latd);
  if (!L.tsy || (L.tsy * L.tsz * static_cast<int64_t>(sizeof(T))) % 16)
    return static_cast<int>(hipErrorInvalidValue);
  const int64_t nvec = L.size() / (16 / static_cast<int64_t>(sizeof(T)));
  const int g = update_grid((nvec + 256 * kUpdU - 1) / (256 * kUpdU));
  // interface partials prefetched (byte offsets of the YB and ZB buffers, sized
  // for two tile rows at least and 8-byte elements, fit 31 bits); the plain
  // kernel serves larger blocks (BDX_UPD_PLAIN=1 forces it: the test hook of
  // tests/test_gpu_runtime.py::test_tiled_update_plain_path_matches)
  const IfaceLayout F = IfaceLayout::of(L, nty > 1 ? nty : 2, ntz > 1 ? ntz : 2);
  const bool pre = kUpdPre && std::getenv("BDX_UPD_PLAIN") == nullptr &&
                   F.zb_size() * 8 < (1LL << 31) && F.yb_size() * 8 < (1LL << 31);
  // ROW (a vector within one z-row, resolved once per vector): FP32 only, see
  // cg_update_tiled_kernel
  auto kern = tiled_kernel<T, false, PA...>(pre);
  if constexpr (sizeof(T) == 4) {
    if (L.tsz % 4 == 0) kern = tiled_kernel<T, true, PA...>(pre);
  }
  kern<<<g, 256, 0, st>>>(L.L[0], L.L[1], L.L[2], static_cast<int>(L.tsy),
                          static_cast<int>(L.tsz), static_cast<int>(L.tntz), own[0], own[1],
                          own[2], nvec, r, y, yb, zb, cb, nty, ntz, scal, rn_slot, pap_slot,
                          partials, pa...);
  return reduce_update<T>(g, scal, partials, out_slot, rr_slot, st, pa...);
}

extern "C" {

#define BDX_UPD(T, SUF)                                                                       \
  int bdx_cg_update_iface_##SUF BDX_P_CG_UPDATE_IFACE(T) {                                    \
    return update_flat<T>(latd, own, r, y, yb, zb, cb, nty, ntz, sy, sz, scal, rn_slot,       \
                          pap_slot, out_slot, -1, partials, st);                              \
  }                                                                                           \
  int bdx_cg_update_tiled_##SUF BDX_P_CG_UPDATE_TILED(T) {                                    \
    return update_tiled<T>(latd, own, r, y, yb, zb, cb, nty, ntz, scal, rn_slot, pap_slot,    \
                           out_slot, -1, partials, st);                                       \
  }                                                                                           \
  int bdx_pcg_update_iface_##SUF BDX_P_PCG_UPDATE_IFACE(T) {                                  \
    if (!dinv || !z || !partials_rr || partials_rr == partials || rr_slot == out_slot)        \
      return static_cast<int>(hipErrorInvalidValue);                                          \
    return update_flat<T>(latd, own, r, y, yb, zb, cb, nty, ntz, sy, sz, scal, rn_slot,       \
                          pap_slot, out_slot, rr_slot, partials, st,                          \
                          PcArgs<T>{dinv, z, partials_rr});                                   \
  }                                                                                           \
  int bdx_pcg_update_tiled_##SUF BDX_P_PCG_UPDATE_TILED(T) {                                  \
    if (!dinv || !z || !partials_rr || partials_rr == partials || rr_slot == out_slot)        \
      return static_cast<int>(hipErrorInvalidValue);                                          \
    return update_tiled<T>(latd, own, r, y, yb, zb, cb, nty, ntz, scal, rn_slot, pap_slot,    \
                           out_slot, rr_slot, partials, st, PcArgs<T>{dinv, z, partials_rr}); \
  }
BDX_UPD(double, f64)
BDX_UPD(float, f32)
#undef BDX_UPD

}  // extern "C"
