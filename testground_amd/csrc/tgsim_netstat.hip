// tgsim_netstat.hip — per-instance traffic counters accumulated on the device (include/tgsim_netstat.h,
// DESIGN.md 2.15). Two passes per window, both the same primitive: a keyed run reduction over a
// stream, then one update per run.
//   TX  (window start, after the last status writer): (m_src, m_size, status) of the staged messages,
//       keyed by local sender; senders arrive in any order, so a run is whatever stretch of equal
//       senders the stream happens to hold (a storm round: fanout messages; one sender's burst: all).
//   RX  (window end, after every delivery writer): (o_dst, o_size, o_flags, o_t) of the deliveries,
//       which are sorted by receiver, so a receiver is one run - of any length.
// The work is balanced over the stream, not per key: every lane reads kItems consecutive items with
// wide loads (the status bytes as one dword, the 32-bit arrays as 16-byte loads), merges equal
// neighbours in registers, then a wave-wide segmented scan on key equality (shuffles) sums what
// crosses lanes, and the last lane of a run adds the run's non-zero fields to the instance's row with
// device-scope 64-bit atomics. A run that crosses a wave or a workgroup simply ends in several
// updates: all sums are integers (and the time a maximum), so the result does not depend on the cut
// or on the order. No loop here is divergent (tools/loopexit_audit.py has nothing to look at).
//
// The small counts travel packed: a wave holds at most 64 * kItems = 256 items, so a 9-bit field
// holds any count a scan can carry (7 fields per 64-bit word).
#include <algorithm>

#include "tgsim_dev.h"

namespace tgsim {

namespace {

constexpr int kItems = 4;                          // consecutive items per lane
constexpr uint32_t kWaveItems = 64 * kItems;       // 256: a 9-bit field holds a run's count inside a wave
constexpr uint32_t kBlockItems = kBlock * kItems;  // 1024
constexpr uint32_t kNoKey = 0xFFFFFFFFu;           // items past the end (and senders of another shard)
constexpr int kFieldBits = 9;
constexpr uint64_t kFieldMask = (1ull << kFieldBits) - 1;
static_assert(kWaveItems <= kFieldMask, "a wave's run must fit a packed field");

__device__ __forceinline__ uint64_t field(uint64_t w, int f) { return (w >> (f * kFieldBits)) & kFieldMask; }
__device__ __forceinline__ uint64_t one(int f) { return 1ull << (f * kFieldBits); }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) {
  const uint32_t lo = __shfl_up((uint32_t)v, o), hi = __shfl_up((uint32_t)(v >> 32), o);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// TX partial of one run: w0 = codes 0..6, w1 = codes 7, 8, any other code, then the four flags.
struct TxAcc {
  uint64_t w0, w1, bytes, qbytes;
  __device__ __forceinline__ static TxAcc item(uint32_t st, uint32_t size) {
    const uint32_t code = st & 0x0Fu;
    TxAcc a;
    a.w0 = code < 7 ? one((int)code) : 0;
    a.w1 = code < 7 ? 0 : one(code <= 8 ? (int)code - 7 : 2);
    a.w1 += (uint64_t)((st >> 4) & 1u) << (3 * kFieldBits);
    a.w1 += (uint64_t)((st >> 5) & 1u) << (4 * kFieldBits);
    a.w1 += (uint64_t)((st >> 6) & 1u) << (5 * kFieldBits);
    a.w1 += (uint64_t)((st >> 7) & 1u) << (6 * kFieldBits);
    a.bytes = size;
    a.qbytes = code == TGSIM_ST_QUEUED ? size : 0;
    return a;
  }
  __device__ __forceinline__ void add(const TxAcc& o) { w0 += o.w0; w1 += o.w1; bytes += o.bytes; qbytes += o.qbytes; }
  __device__ __forceinline__ TxAcc up(int o) const {
    return TxAcc{shfl_up64(w0, o), shfl_up64(w1, o), shfl_up64(bytes, o), shfl_up64(qbytes, o)};
  }
  __device__ __forceinline__ void flush(const NetstatDev& ns, uint32_t row) const {
    if (row >= ns.nloc) return;
    uint64_t msgs = field(w1, 2);
    uint64_t* st = ns.tx_status + (size_t)row * TGSIM_NETSTAT_CODES;
#pragma unroll
    for (int c = 0; c < 7; ++c) { const uint64_t k = field(w0, c); msgs += k; add64(st + c, k); }
#pragma unroll
    for (int c = 7; c < 9; ++c) { const uint64_t k = field(w1, c - 7); msgs += k; add64(st + c, k); }
    add64(ns.tx_msgs + row, msgs);
    add64(ns.tx_bytes + row, bytes);
    add64(ns.tx_queued_bytes + row, qbytes);
    add64(ns.tx_dup + row, field(w1, 3));
    add64(ns.tx_clone_lost + row, field(w1, 4));
    add64(ns.tx_dup_cancel + row, field(w1, 5));
    add64(ns.tx_orig_overlimit + row, field(w1, 6));
  }
};

// RX partial of one run: w = packets, corrupt, clones, reordered, local.
struct RxAcc {
  uint64_t w, bytes;
  int64_t t;
  __device__ __forceinline__ static RxAcc item(uint32_t size, uint32_t flags, int64_t t) {
    RxAcc a;
    a.w = 1u;
    a.w += (uint64_t)((flags >> 1) & 1u) << (1 * kFieldBits);  // TGSIM_F_CORRUPT
    a.w += (uint64_t)((flags >> 0) & 1u) << (2 * kFieldBits);  // TGSIM_F_CLONE
    a.w += (uint64_t)((flags >> 2) & 1u) << (3 * kFieldBits);  // TGSIM_F_REORDERED
    a.w += (uint64_t)((flags >> 7) & 1u) << (4 * kFieldBits);  // TGSIM_F_LOCAL
    a.bytes = size;
    a.t = t;
    return a;
  }
  __device__ __forceinline__ void add(const RxAcc& o) { w += o.w; bytes += o.bytes; t = o.t > t ? o.t : t; }
  __device__ __forceinline__ RxAcc up(int o) const {
    return RxAcc{shfl_up64(w, o), shfl_up64(bytes, o), (int64_t)shfl_up64((uint64_t)t, o)};
  }
  __device__ __forceinline__ void flush(const NetstatDev& ns, uint32_t row) const {
    if (row >= ns.nloc) return;
    add64(ns.rx_packets + row, field(w, 0));
    add64(ns.rx_bytes + row, bytes);
    add64(ns.rx_corrupt + row, field(w, 1));
    add64(ns.rx_clones + row, field(w, 2));
    add64(ns.rx_reordered + row, field(w, 3));
    add64(ns.rx_local + row, field(w, 4));
    atomicMax(reinterpret_cast<long long*>(ns.rx_t_last + row), (long long)t);
  }
};
static_assert((TGSIM_F_CLONE | TGSIM_F_CORRUPT | TGSIM_F_REORDERED | TGSIM_F_LOCAL) == 0x87u, "delivery flag bits");
static_assert(TGSIM_ST_FLAG_DUP == 0x10 && TGSIM_ST_FLAG_OVERLIMIT == 0x80, "status flag bits");

// One wave's kItems * 64 consecutive items (lane l holds items l * kItems ..), keys k, partials it.
// Every lane of the wave calls it.
template <class A>
__device__ __forceinline__ void run_reduce(const uint32_t (&k)[kItems], const A (&it)[kItems], const NetstatDev& ns) {
  const uint32_t lane = lane_id();
  // lane-local merge: `head` is the lane's first run when it ends inside the lane (split), `acc` ends
  // as its last run; a run wholly inside the lane is complete and goes out at once
  A acc = it[0], head = it[0];
  bool split = false;
#pragma unroll
  for (int j = 1; j < kItems; ++j) {
    if (k[j] == k[j - 1]) {
      acc.add(it[j]);
    } else {
      if (split) acc.flush(ns, k[j - 1]);
      else head = acc;
      split = true;
      acc = it[j];
    }
  }
  const uint32_t kf = k[0], kl = k[kItems - 1];
  const uint32_t kprev = __shfl_up(kl, 1), knext = __shfl_down(kf, 1);
  const bool joins = lane != 0 && kprev == kf;  // the lane's first run continues the previous lane's last
  // segmented inclusive scan of the lanes' last runs: a lane opens a segment unless it is one run
  // (no split) that continues its neighbour's
  A s = acc;
  uint32_t open = (!joins || split) ? 1u : 0u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const A y = s.up(o);
    const uint32_t oy = __shfl_up(open, o);
    if ((int)lane >= o && !open) {
      s.add(y);
      open = oy;
    }
  }
  const A before = s.up(1);  // the previous lane's run so far
  if (split) {               // the lane's first run ends here: with what led up to it
    if (joins) head.add(before);
    head.flush(ns, kf);
  }
  if (lane == 63 || knext != kl) s.flush(ns, kl);  // the last lane of a run (or of the wave's share of it)
}

struct TxArgs {
  const uint32_t *src, *size;
  const uint8_t* status;
  const uint32_t* n_dev;  // non-null: the staged count is read here (device-counted staging)
  uint32_t n, cap, lo;
};

// VEC: src / size are 16-byte aligned (the library's own arrays always; a caller's in-place batch when
// its pointers are). The status bytes are the library's.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_netstat_tx(TxArgs a, NetstatDev ns) {
  uint32_t n = a.n;
  if (a.n_dev) n = min(*a.n_dev, a.cap);
  const uint32_t t = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlockItems; base < n; base += (uint64_t)gridDim.x * kBlockItems) {
    const uint64_t wbase = base + (uint64_t)__builtin_amdgcn_readfirstlane(t >> 6) * kWaveItems;
    if (wbase >= n) continue;  // wave-uniform: nothing of this wave's share is staged
    const uint64_t i0 = base + (uint64_t)t * kItems;
    uint32_t k[kItems], sz[kItems], st[kItems];
    if (i0 + kItems <= n) {
      const uint32_t s4 = *reinterpret_cast<const uint32_t*>(a.status + i0);
      if (VEC) {
        const uint4 ks = *reinterpret_cast<const uint4*>(a.src + i0), zs = *reinterpret_cast<const uint4*>(a.size + i0);
        k[0] = ks.x; k[1] = ks.y; k[2] = ks.z; k[3] = ks.w;
        sz[0] = zs.x; sz[1] = zs.y; sz[2] = zs.z; sz[3] = zs.w;
      } else {
#pragma unroll
        for (int j = 0; j < kItems; ++j) { k[j] = a.src[i0 + j]; sz[j] = a.size[i0 + j]; }
      }
#pragma unroll
      for (int j = 0; j < kItems; ++j) st[j] = (s4 >> (8 * j)) & 0xFFu;
    } else {
#pragma unroll
      for (int j = 0; j < kItems; ++j) {
        const bool in = i0 + j < n;
        k[j] = in ? a.src[i0 + j] : kNoKey;
        sz[j] = in ? a.size[i0 + j] : 0u;
        st[j] = in ? a.status[i0 + j] : 0u;
      }
    }
    TxAcc it[kItems];
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      // a sender outside [lo, lo + nloc) (refused by the window with ERR_BAD_MSG) has no row
      const uint32_t l = k[j] - a.lo;
      k[j] = (k[j] != kNoKey && l < ns.nloc) ? l : kNoKey;
      it[j] = TxAcc::item(st[j], sz[j]);
    }
    run_reduce<TxAcc>(k, it, ns);
  }
}

struct RxArgs {
  const uint32_t *dst, *size, *flags;
  const int64_t* t;
  const DevScalars* sc;
  uint32_t cap, lo;
};

__global__ void __launch_bounds__(kBlock) k_netstat_rx(RxArgs a, NetstatDev ns) {
  const uint32_t n = min(a.sc->n_out, a.cap);
  const uint32_t t = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlockItems; base < n; base += (uint64_t)gridDim.x * kBlockItems) {
    const uint64_t wbase = base + (uint64_t)__builtin_amdgcn_readfirstlane(t >> 6) * kWaveItems;
    if (wbase >= n) continue;  // wave-uniform: nothing of this wave's share is staged
    const uint64_t i0 = base + (uint64_t)t * kItems;
    uint32_t k[kItems], sz[kItems], fl[kItems];
    int64_t tt[kItems];
    if (i0 + kItems <= n) {
      const uint4 ks = *reinterpret_cast<const uint4*>(a.dst + i0), zs = *reinterpret_cast<const uint4*>(a.size + i0),
                  fs = *reinterpret_cast<const uint4*>(a.flags + i0);
      const longlong2 t0 = *reinterpret_cast<const longlong2*>(a.t + i0), t1 = *reinterpret_cast<const longlong2*>(a.t + i0 + 2);
      k[0] = ks.x; k[1] = ks.y; k[2] = ks.z; k[3] = ks.w;
      sz[0] = zs.x; sz[1] = zs.y; sz[2] = zs.z; sz[3] = zs.w;
      fl[0] = fs.x; fl[1] = fs.y; fl[2] = fs.z; fl[3] = fs.w;
      tt[0] = t0.x; tt[1] = t0.y; tt[2] = t1.x; tt[3] = t1.y;
    } else {
#pragma unroll
      for (int j = 0; j < kItems; ++j) {
        const bool in = i0 + j < n;
        k[j] = in ? a.dst[i0 + j] : kNoKey;
        sz[j] = in ? a.size[i0 + j] : 0u;
        fl[j] = in ? a.flags[i0 + j] : 0u;
        tt[j] = in ? a.t[i0 + j] : INT64_MIN;
      }
    }
    RxAcc it[kItems];
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const uint32_t l = k[j] - a.lo;
      k[j] = (k[j] != kNoKey && l < ns.nloc) ? l : kNoKey;
      it[j] = RxAcc::item(sz[j], fl[j], tt[j]);
    }
    run_reduce<RxAcc>(k, it, ns);
  }
}

__global__ void k_netstat_fill_tlast(int64_t* t_last, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) t_last[i] = INT64_MIN;
}

unsigned netstat_grid(uint64_t items) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + kBlockItems - 1) / kBlockItems, 1), kStreamBlocks);
}

}  // namespace

void netstat_bind(NetstatDev& ns, uint64_t* base, uint32_t nloc) {
  const size_t n = std::max<uint32_t>(nloc, 1);
  ns.base = base;
  ns.nloc = nloc;
  uint64_t* p = base;
  for (uint64_t** f : {&ns.tx_msgs, &ns.tx_bytes, &ns.tx_queued_bytes, &ns.tx_dup, &ns.tx_clone_lost, &ns.tx_dup_cancel,
                       &ns.tx_orig_overlimit, &ns.rx_packets, &ns.rx_bytes, &ns.rx_corrupt, &ns.rx_clones,
                       &ns.rx_reordered, &ns.rx_local}) {
    *f = p;
    p += n;
  }
  ns.tx_status = p;
  p += n * TGSIM_NETSTAT_CODES;
  ns.rx_t_last = reinterpret_cast<int64_t*>(p);
}

hipError_t launch_netstat_reset(Dev& d, NetstatDev& ns) {
  const hipError_t e = hipMemsetAsync(ns.base, 0, netstat_bytes(ns.nloc), d.stream);
  if (e != hipSuccess) return e;
  if (ns.nloc)
    hipLaunchKernelGGL(k_netstat_fill_tlast, dim3((ns.nloc + kBlock - 1) / kBlock), dim3(kBlock), 0, d.stream,
                       ns.rx_t_last, ns.nloc);
  return hipGetLastError();
}

hipError_t launch_netstat_tx(Dev& d, NetstatDev& ns, uint32_t n_staged, const uint32_t* n_dev) {
  if (!n_dev && !n_staged) return hipSuccess;
  TxArgs a;
  a.src = d.m_src; a.size = d.m_size; a.status = d.status; a.n_dev = n_dev; a.n = n_staged; a.cap = d.cap_msgs;
  a.lo = d.lo;
  const bool vec = (((uintptr_t)a.src | (uintptr_t)a.size) & 15u) == 0;
  ProfScope ps_(d, KID_NETSTAT);
  hipLaunchKernelGGL(vec ? k_netstat_tx<true> : k_netstat_tx<false>, dim3(netstat_grid(n_dev ? d.cap_msgs : n_staged)),
                     dim3(kBlock), 0, d.stream, a, ns);
  return hipGetLastError();
}

hipError_t launch_netstat_rx(Dev& d, NetstatDev& ns) {
  RxArgs a;
  a.dst = d.o_dst; a.size = d.o_size; a.flags = d.o_flags; a.t = d.o_t; a.sc = d.sc;
  a.cap = (uint32_t)std::min<uint64_t>((uint64_t)kNSub * d.subcap, 0xFFFFFFFFull);
  a.lo = d.lo;
  ProfScope ps_(d, KID_NETSTAT);
  hipLaunchKernelGGL(k_netstat_rx, dim3(netstat_grid(a.cap)), dim3(kBlock), 0, d.stream, a, ns);
  return hipGetLastError();
}

}  // namespace tgsim
