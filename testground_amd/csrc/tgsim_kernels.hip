// tgsim_kernels.hip — gfx950 kernels of the simulator's window pipeline.
//
//  (1) k_shape        fused route (CIDR LPM over per-sender rule CSR) + netem Philox draws
//                     (duplicate, loss, corrupt, reorder, jitter) per message -> copy records,
//                     appended with wave64 ballot/prefix compaction into 64-way sharded queues.
//  (2) token bucket   copies grouped by sender (stable LSD radix group-by), ordered by
//                     (netem time, seq, clone-first) in LDS (rank sort for short segments, bitonic
//                     otherwise), then the HTB GCRA recurrence as a max-plus block scan in LDS.
//  (3) deliveries     due copies grouped by receiver, ordered (t, src, seq, clone-first) in LDS,
//                     written as the inbox SoA; future events go to a timing-wheel region:
//                     a counting (radix) sort on integer-ns slot, extracted by slot prefix later.
//  (4) sync service   signal batches ordered by (state, t, instance) -> 1-based sequence numbers,
//                     per-state counters and a signal log; barrier waiters resolved on device.
// Segments longer than kTile go through a merge-path chunk sort (k_large_*).
#include <algorithm>

#include "tgsim_dev.h"

namespace tgsim {

const char* const kKernelNames[KID_COUNT] = {
    "k_extract_shape", "k_extract", "k_tb_bucket", "k_emit_bucket", "k_radix_hist", "k_radix_rows", "k_radix_scatter",
    "k_keys", "k_bounds", "k_wheel_scatter", "k_gen_storm", "sync_signal", "large_segments",
    "k_bkt_hist", "k_bkt_scatter", "k_bkt_sort", "seg_rest", "k_flood_count", "k_flood_emit",
    "k_shape_seq", "k_probe", "k_seg_small", "k_storm", "exchange", "allreduce", "k_shape_seq_wide", "k_copy_n",
    "k_netstat"};

// after a stream synchronisation: fold completed event pairs into the per-kernel totals
static void prof_resolve(Dev& d) {
  size_t keep = 0;
  for (auto& p : d.prof.pending) {
    if (hipEventQuery(p.b) == hipErrorNotReady) {  // a scope on the side stream still running
      d.prof.pending[keep++] = p;
      continue;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      d.prof.ms[p.kid] += ms;
      d.prof.n[p.kid] += 1;
    }
    d.prof.pool.push_back(p.a);
    d.prof.pool.push_back(p.b);
  }
  d.prof.pending.resize(keep);
}

// ============================================================================================
// small device helpers
// ============================================================================================

typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));

// Stores of the records and arrays one launch writes and the next reads. TG_NT_STORES (experiment
// builds) makes them non-temporal, so fewer dirty L2 lines are left for the write-back at the
// launch boundary (MI355X_MICROARCH.md: + B / 6 TB/s behind a predecessor that leaves B dirty).
__device__ __forceinline__ void st4(void* p, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  const v4u32 v = {x, y, z, w};
#ifdef TG_NT_STORES
  __builtin_nontemporal_store(v, reinterpret_cast<v4u32*>(p));
#else
  *reinterpret_cast<v4u32*>(p) = v;
#endif
}
template <class T>
__device__ __forceinline__ void stn(T* p, T v) {
#ifdef TG_NT_STORES
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

__device__ __forceinline__ void load_rec(const tgsim_record* p, tgsim_record& r) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  r.t = (int64_t)(((uint64_t)a.y << 32) | a.x);
  r.src = a.z; r.dst = a.w; r.seq = b.x; r.size = b.y; r.meta = b.z; r.corrupt_off = b.w;
}
__device__ __forceinline__ void store_rec(tgsim_record* p, const tgsim_record& r) {
  uint4* q = reinterpret_cast<uint4*>(p);
  st4(q, (uint32_t)(uint64_t)r.t, (uint32_t)((uint64_t)r.t >> 32), r.src, r.dst);
  st4(q + 1, r.seq, r.size, r.meta, r.corrupt_off);
}

// Wave64 compaction onto per-lane counters: lanes whose counter pointer is equal share one
// atomicAdd (ballot -> leader atomic -> broadcast -> mbcnt rank). nullptr = nothing to append.
__device__ __forceinline__ uint32_t wave_append(uint32_t* ctr) {
  uint32_t pos = 0xFFFFFFFFu;
  bool pending = ctr != nullptr;
  const uint64_t me = (uint64_t)(uintptr_t)ctr;
  for (;;) {
    const uint64_t m = __ballot(pending);
    if (m == 0) break;
    const int leader = __ffsll((unsigned long long)m) - 1;
    const uint32_t lo = __shfl((uint32_t)me, leader), hi = __shfl((uint32_t)(me >> 32), leader);
    const uint64_t lp = ((uint64_t)hi << 32) | lo;
    const bool mine = pending && me == lp;
    const uint64_t mm = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane_id() == leader)
      base = __hip_atomic_fetch_add(reinterpret_cast<__attribute__((address_space(1))) uint32_t*>(lp),
                                    (uint32_t)__popcll(mm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader);
    if (mine) { pos = base + mask_rank(mm); pending = false; }
  }
  return pos;
}

// Batches A (token-bucket input), D (deliveries), L (wheel insert) are split into kNSub
// sub-queues, each with its own counter on its own 128-B line, so that 10^5-10^6 appends per
// window do not serialise on one address. X are the per-peer exchange blocks.
// A pointer held in scalar registers as an opaque value. A queue base chosen per lane from kernel
// arguments (isD ? D : L) is otherwise turned into a vector load from the kernel-argument segment
// at a lane-varying offset, and the wait for that load (stores count in vmcnt too) drains the wave's
// stores before every record.
template <class T>
__device__ __forceinline__ T* pin_scalar(T* p) {
  // through a global-address-space pointer: behind the asm the compiler no longer sees a kernel
  // argument, and a generic pointer would make every store through it a flat store
  typedef __attribute__((address_space(1))) T* GlobalPtr;
  GlobalPtr o;
  asm volatile("s_mov_b64 %0, %1" : "=s"(o) : "s"((GlobalPtr)p));
  return (T*)o;
}
// A wave-uniform 64-bit value that came through a vector load, moved to scalar registers.
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  return (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32)) << 32) |
                   __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v));
}

struct Queues {
  DevScalars* sc;
  uint32_t* qc;
  uint32_t* xq;              // exchange cursors: (peer p, slice g) at xq[(p * kXSlices + g) << 5] (qc lines 3 kNSub..)
  tgsim_record *A, *D, *L, *X;
  uint32_t *KA, *KD, *KL;    // group-by key of each appended record, same physical index as in A / D / L
  uint32_t subcap, xcap, lo, slots;
  uint32_t xg, xcs;          // exchange slices per peer block and records per slice (x_slices / x_slice_cap)
  int64_t slot_ns;
  SlotDiv sdiv;              // t / slot_ns without a division (tgsim_slotdiv.h; made at context creation)
  // consumer groups of A / D keys: the fused consumers give XCD x a contiguous run of buckets
  // (xcd_major), i.e. keys [gb[x-1], gb[x]); producers order each wave's A / D slots by group, so a
  // line of records is read by one XCD (whose L2 then serves its other records)
  uint32_t gb[7];
  __device__ __forceinline__ uint32_t group_of(uint32_t key) const {
    uint32_t g = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) g += key >= gb[j] ? 1u : 0u;
    return g;
  }
  // Exchange cursor of peer p for this workgroup's slice: a 128-B line of its own after the A / D / L
  // sub-queue counters (round 4 kept every peer's cursor in one DevScalars line; one per wave and
  // item serialised a sharded token bucket on that address: k_tb_bucket 20 -> 165 us per 50k shard,
  // VERDICT r4 item 1; one line per peer still took every workgroup's reservation in turn)
  __device__ __forceinline__ uint32_t xslice() const {  // xg is 1 or 8
    return __builtin_amdgcn_readfirstlane(blockIdx.x & (xg - 1u));
  }
  __device__ __forceinline__ uint32_t* xctr(uint32_t p, uint32_t g) const { return xq + ((p * kXSlices + g) << 5); }
  // (32-bit offsets: S * xcap < 2^32 is checked at create)
  __device__ __forceinline__ tgsim_record* xslot(uint32_t p, uint32_t g) const { return X + (p * xcap + 1u + g * xcs); }
  // A: local sender; D: local receiver; L: timing-wheel slot relative to this window's end
  __device__ __forceinline__ uint32_t key_of(int q, const tgsim_record& r) const {
    if (q == Q_A) return r.src - lo;
    if (q == Q_D) return r.dst - lo;
    return slot_key(sdiv, r.t, sc->base_slot, slots);
  }
  // Wave-collective: every lane of the wave calls it; salt must be wave-uniform.
  __device__ __forceinline__ void push(int q, const tgsim_record& r, uint32_t salt) const {
    const bool loc = q >= 0 && q < Q_X0;
    uint32_t* ctr = nullptr;
    tgsim_record* buf = nullptr;
    if (loc) {
      // sub-queue: blocks b and b+8 share an XCD under round-robin dispatch, so counters
      // 8x..8x+7 are only touched from one XCD's L2 (a speed choice; any mapping is correct)
      const uint32_t sub = ((blockIdx.x & 7u) << 3) | ((salt + (blockIdx.x >> 3) * 4u + (threadIdx.x >> 6)) & 7u);
      ctr = qc + (((uint32_t)q * kNSub + sub) << 5);
      buf = (q == Q_A ? A : (q == Q_D ? D : L)) + (size_t)sub * subcap;
    }
    const uint32_t pos = wave_append(ctr);
    if (loc) {
      if (pos < subcap) {
        store_rec(buf + pos, r);
        (q == Q_A ? KA : (q == Q_D ? KD : KL))[(size_t)(buf - (q == Q_A ? A : (q == Q_D ? D : L))) + pos] = key_of(q, r);
      } else {
        atomicOr(&sc->err, q == Q_A ? ERR_CAP_A : (q == Q_D ? ERR_CAP_D : ERR_CAP_L));
      }
    }
    if (__ballot(q >= Q_X0)) push_x(q, r, salt);
  }

  // Exchange append (wave-collective; lanes with q < Q_X0 take no part). The salt (the caller's
  // round / item) turns a workgroup's successive pushes to successive slices, so one busy workgroup
  // does not fill one slice alone; a lane whose slice is full goes on through the peer's other
  // slices, so the per-peer bound is the whole block, xg * xcs records (a skewed
  // producer overflowed its one slice far below it). The slice is a scalar (readfirstlane) and the
  // offsets 32-bit: anything else spilled k_extract_shape's registers at its 96-VGPR cap. A full
  // slice's cursor runs past xcs; k_xheaders clamps the counts.
  __device__ __forceinline__ void push_x(int q, const tgsim_record& r, uint32_t salt) const {
    bool pend = q >= Q_X0;
    const uint32_t p = pend ? (uint32_t)(q - Q_X0) : 0u;
    const uint32_t g0 = __builtin_amdgcn_readfirstlane((blockIdx.x + salt) & (xg - 1u));
    for (uint32_t a = 0; a < xg && __ballot(pend); ++a) {
      const uint32_t g = (g0 + a) & (xg - 1u);
      const uint32_t pos = wave_append(pend ? xq + ((p * kXSlices + g) << 5) : nullptr);
      if (pend && pos < xcs) {
        store_rec(X + (p * xcap + (1u + g * xcs)) + pos, r);
        pend = false;
      }
    }
    if (pend) atomicOr(&sc->err, ERR_CAP_X);
  }

  // Wave-collective append of U records per lane (q[u] < 0: none). The local queues A / D / L take
  // one sub-queue per wave for the whole batch and at most three independent atomics (one round
  // trip) reserve it, instead of a dependent atomic per record and distinct counter. L slots go
  // record-major, lane-minor (one ballot per record), so each store instruction covers consecutive
  // records; A and D slots go by consumer group (a per-wave counting sort in LDS), so each line is
  // read by one XCD. Exchange records (sharded runs) take the per-record path.
  // spread: the salt alone picks the sub-queue (any of the 64), for a producer whose one workgroup
  // may append far more than a sub-queue's share (k_shape_seq: one sender per workgroup, every one
  // of its chunks in turn; with the XCD-pinned choice a 10k-reply sender filled one sub-queue)
  template <int U, int Waves = kBlock / 64>
  __device__ __forceinline__ void push_batch(const int (&q)[U], const tgsim_record (&r)[U], uint32_t salt,
                                             bool spread = false) const {
    __shared__ uint32_t gcnt[Waves][16];  // per wave: [A groups 0..7 | D groups 0..7]
    const uint32_t lane = lane_id();
    uint32_t* cnt = gcnt[threadIdx.x >> 6];
    const uint32_t sub = spread ? (salt & (kNSub - 1u))
                                : ((blockIdx.x & 7u) << 3) | ((salt + (blockIdx.x >> 3) * 4u + (threadIdx.x >> 6)) & 7u);
    // any lanes may be active (grid-stride tails): the first active one keeps the 16 counters
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)__ballot(true)) - 1u;
    if (lane == leader)
      for (int i = 0; i < 16; ++i) cnt[i] = 0;
    __builtin_amdgcn_wave_barrier();
    uint64_t mL[U];
    uint32_t rk[U];
    bool any_x = false;
    uint32_t tL = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      mL[u] = __ballot(q[u] == Q_L);
      tL += (uint32_t)__popcll(mL[u]);
      any_x |= q[u] >= Q_X0;
      rk[u] = 0;
      if (q[u] == Q_A || q[u] == Q_D)
        rk[u] = ((q[u] == Q_D ? 8u : 0u) + group_of(key_of(q[u], r[u]))) << 24 |
                atomicAdd(&cnt[(q[u] == Q_D ? 8u : 0u) + group_of(key_of(q[u], r[u]))], 1u);
    }
    __builtin_amdgcn_wave_barrier();
    // group counts -> exclusive offsets inside each queue's reservation
    uint32_t sA = 0, sD = 0;
    if (lane == leader) {
      for (int i = 0; i < 8; ++i) { const uint32_t v = cnt[i]; cnt[i] = sA; sA += v; }
      for (int i = 8; i < 16; ++i) { const uint32_t v = cnt[i]; cnt[i] = sD; sD += v; }
    }
    const uint32_t tA = __shfl(sA, (int)leader), tD = __shfl(sD, (int)leader);
    __builtin_amdgcn_wave_barrier();
    uint32_t rA = 0, rD = 0, rL = 0;
    if (lane == leader) {  // three independent atomics: one round trip
      if (tA) rA = atomicAdd(qc + (((uint32_t)Q_A * kNSub + sub) << 5), tA);
      if (tD) rD = atomicAdd(qc + (((uint32_t)Q_D * kNSub + sub) << 5), tD);
      if (tL) rL = atomicAdd(qc + (((uint32_t)Q_L * kNSub + sub) << 5), tL);
    }
    const uint32_t pA = __shfl(rA, (int)leader), pD = __shfl(rD, (int)leader);
    uint32_t pL = __shfl(rL, (int)leader);
#pragma unroll
    for (int u = 0; u < U; ++u) {  // no runtime-indexed private arrays (they would live in scratch)
      const int k = q[u];
      if (k >= 0 && k < Q_X0) {
        const uint32_t pos = k == Q_L ? pL + mask_rank(mL[u])
                                      : (k == Q_A ? pA : pD) + cnt[rk[u] >> 24] + (rk[u] & 0xFFFFFFu);
        if (pos < subcap) {
          const size_t at = (size_t)sub * subcap + pos;
          store_rec((k == Q_A ? A : (k == Q_D ? D : L)) + at, r[u]);
          stn((k == Q_A ? KA : (k == Q_D ? KD : KL)) + at, key_of(k, r[u]));
        } else {
          atomicOr(&sc->err, k == Q_A ? ERR_CAP_A : (k == Q_D ? ERR_CAP_D : ERR_CAP_L));
        }
      }
      pL += (uint32_t)__popcll(mL[u]);
    }
    if (__ballot(any_x)) {  // per item: one reservation per (wave, peer) on the peer's cursor
#pragma unroll
      for (int u = 0; u < U; ++u) push(q[u] >= Q_X0 ? q[u] : -1, r[u], salt + u);
    }
  }
};

struct Geo {
  uint32_t N, S, shard;
  uint64_t inv;  // shard_inv(N)
};
static Geo make_geo(const Dev& d) { return Geo{d.N, d.S, d.shard, shard_inv(d.N)}; }

// Queue of a stage-D record (its t is the delivery time): delivered now (here, or on the receiver's
// shard through the exchange) or later from this shard's wheel. A record crosses shards only in the
// window it is due, so every queued copy of a local sender waits on its sender's shard,
// where its queue occupancy is counted.
__device__ __forceinline__ int qid_stage_d(const Geo& g, uint32_t dst, int64_t t, int64_t t_end) {
  if (t >= t_end) return Q_L;
  if (g.S > 1) {
    const uint32_t p = shard_of_inv(dst, g.S, g.inv);
    if (p != g.shard) return Q_X0 + (int)p;
  }
  return Q_D;
}

__device__ __forceinline__ uint32_t clamp_n(const uint32_t* n_ptr, uint32_t cap) {
  const uint32_t n = *n_ptr;
  return n < cap ? n : cap;
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t v) {
  v = v < 2 ? 2 : v;
  return 1u << (32 - __clz(v - 1));
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ============================================================================================
// window control
// ============================================================================================

__device__ void plan_regions(RegionDev* regions, const uint32_t* dirs, uint32_t slots, int64_t slot_ns,
                             uint32_t* plan_start, uint32_t* plan_off, DevScalars* sc, int64_t t_end);

// Window start (one block): the window's end — explicit, a barrier waiter's release + offset
// (decided on the device, no host round trip), or a device value + offset — then the per-window
// counters zeroed and the timing-wheel extraction plan of the window.
enum { WIN_EXPLICIT = 0, WIN_BARRIER = 1, WIN_DEVICE = 2 };
// The window starts where the previous one ended (H = its start, T = its end), read on the device,
// so a run of barrier- or device-ended windows needs no host round trip at all.
struct WindowArgs {
  DevScalars* sc;
  uint32_t* qc;
  int mode;
  int64_t t_end_arg;
  const int64_t* src;
  int64_t offset;
  int64_t slot_ns;
  RegionDev* regions;
  const uint32_t* dirs;
  uint32_t slots;
  uint32_t* plan_start;
  uint32_t* plan_off;
};

__device__ __forceinline__ void window_start_block(const WindowArgs& a) {
  DevScalars* sc = a.sc;
  uint32_t* qc = a.qc;
  const int mode = a.mode;
  const int64_t t_end_arg = a.t_end_arg, offset = a.offset, slot_ns = a.slot_ns;
  const int64_t* src = a.src;
  __shared__ int64_t s_tend;
  for (uint32_t i = threadIdx.x; i < kQcLines; i += kBlock) qc[i << 5] = 0;  // one counter per 128-B line
  uint32_t* w = sc->q;  // the per-window block [q, err) of DevScalars
  const uint32_t nw = (uint32_t)((offsetof(DevScalars, err) - offsetof(DevScalars, q)) / sizeof(uint32_t));
  for (uint32_t i = threadIdx.x; i < nw; i += kBlock) w[i] = 0;
  if (threadIdx.x == 0) {
    const int64_t H = sc->T, T = sc->t_end;
    int64_t e = t_end_arg;
    if (mode == WIN_BARRIER) {
      const int64_t rel = *src;
      if (rel < 0) {
        atomicOr(&sc->err, ERR_UNRELEASED);
        e = T;
      } else {
        e = rel + offset;
      }
    } else if (mode == WIN_DEVICE) {
      e = *src + offset;
    }
    e = e < T ? T : e;
    sc->H = H;
    sc->T = T;
    sc->t_end = e;
    sc->base_slot = e / slot_ns;
    s_tend = e;
  }
  __syncthreads();
  plan_regions(a.regions, a.dirs, a.slots, slot_ns, a.plan_start, a.plan_off, sc, s_tend);
}

__global__ __launch_bounds__(kBlock) void k_window_start(WindowArgs a) { window_start_block(a); }

__global__ void k_set_u32(uint32_t* p, uint32_t v) { *p = v; }

__global__ void k_reset_tb(int64_t* X, const uint32_t* locals, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) X[locals[i]] = kNegInf;
}

// Close a sharded queue for reading: prefix over its sub-queues (one wave).
__device__ __forceinline__ void queue_final(DevScalars* sc, const uint32_t* qc, int q, uint32_t subcap) {
  const uint32_t s = threadIdx.x;  // one wave
  const uint32_t raw = qc[(((uint32_t)q * kNSub) + s) << 5];
  if (raw > subcap) atomicOr(&sc->err, q == Q_A ? ERR_CAP_A : (q == Q_D ? ERR_CAP_D : ERR_CAP_L));
  const uint32_t c = raw < subcap ? raw : subcap;
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if ((int)s >= o) x += y;
  }
  sc->qpre[q][s] = x - c;
  if (s == 63) { sc->qpre[q][kNSub] = x; sc->qn[q] = x; }
}

// ============================================================================================
// (1) route + netem: one thread per staged message
// ============================================================================================

enum { R_NONE = 0, R_DATA, R_DEFAULT, R_DROP, R_REJECT };

struct ShapeArgs {
  const uint32_t *src, *dst, *seq, *size;
  const int64_t* t;
  uint32_t n;
  const uint32_t* n_dev;      // non-null: the staged count is device-side (sc->n_msgs_dev), n unused
  uint8_t* status;
  const ShapeDev* shape;
  const uint64_t* ipf;         // [N] ip | flags << 32
  const uint32_t* en_bits;     // [N / 32] link enabled per instance (the destination test, L2-resident)
  const uint32_t* rule_off;
  const RuleDev* rules;
  uint32_t lo, nloc, data_net, data_mask, data_len, key0, key1;
  Geo geo;
  Queues Q;
  unsigned long long* stats;  // [kNSub][16] sharded counters
  uint32_t* corr_idx;         // deferred messages of correlated / queue-heavy senders: kDeferSub sub-lists of
                              // defer_seg_cap(n) entries, counted on qc lines kQcDefer + s (k_keys_corr joins them)
  Heavy heavy;                // the window's queue-limit test
  uint32_t may_defer;         // some shape is correlated or the queue-limit test is on
};

// Longest-prefix match over the sender's routing table: rule groups by prefix
// length (descending), each a sorted run searched by bisection; the data network's connected
// route and the control network's default route compete at their own prefix lengths.
__device__ int route_lookup(const ShapeArgs& a, uint8_t f, uint32_t pos, uint32_t end, uint32_t dip) {
  const bool data_ok = (f & 1u) && ((dip & a.data_mask) == a.data_net);
  while (pos < end) {
    const uint32_t plen = a.rules[pos].plen_action & 0xFFu;
    if (data_ok && a.data_len > plen) return R_DATA;
    uint32_t lo = pos + 1, hi = end;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((a.rules[mid].plen_action & 0xFFu) == plen) lo = mid + 1; else hi = mid;
    }
    const uint32_t gend = lo;
    const uint32_t mask = plen ? 0xFFFFFFFFu << (32 - plen) : 0u;
    const uint32_t target = dip & mask;
    lo = pos; hi = gend;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.rules[mid].prefix < target) lo = mid + 1; else hi = mid;
    }
    if (lo < gend && a.rules[lo].prefix == target)
      return ((a.rules[lo].plen_action >> 8) & 0xFFu) == TGSIM_FILTER_DROP ? R_DROP : R_REJECT;
    pos = gend;
  }
  if (data_ok) return R_DATA;
  if (f & 2u) return R_DEFAULT;
  return R_NONE;
}

// netem tabledist() uniform branch [EXT].
__device__ __forceinline__ int64_t tabledist(int64_t mu, int32_t sigma, uint32_t rnd) {
  if (sigma == 0) return mu;
  const uint32_t m = 2u * (uint32_t)sigma;
  if (m == 0) return mu;
  return (int64_t)(rnd % m) + mu - (int64_t)sigma;
}

// The part of netem_enqueue [EXT] after the duplicate/loss decision, for one copy. r0 is the
// copy's block-0 draw (loss, delay, reorder words).
__device__ __forceinline__ bool netem_copy(const ShapeDev& sh, const uint32_t r0[4], uint32_t src, uint32_t dst,
                                           uint32_t seq, uint32_t size, int64_t ts, uint32_t clone, uint32_t k0,
                                           uint32_t k1, tgsim_record& rec) {
  if (clone && sh.loss_t && sh.loss_t >= r0[1]) return false;
  rec.src = src; rec.dst = dst; rec.seq = seq; rec.size = size;
  rec.meta = clone ? TGSIM_F_CLONE : 0u;
  rec.corrupt_off = 0;
  if (sh.corrupt_t) {
    uint32_t r1[4];
    philox4x32_10(seq, src, clone | 2u, kNetemSalt, k0, k1, r1);
    if (sh.corrupt_t >= r1[0] && size > 0) {
      rec.meta |= TGSIM_F_CORRUPT | ((r1[2] % 8u) << TGSIM_F_BIT_SHIFT);
      rec.corrupt_off = r1[1] % size;
    }
  }
  if (sh.reorder_t && !(sh.reorder_t < r0[3])) {
    rec.meta |= TGSIM_F_REORDERED;
    rec.t = ts;
  } else {
    const int64_t delay = tabledist(sh.mu, sh.sigma, r0[2]);
    rec.t = ts + (delay > 0 ? delay : 0);
  }
  if (!(sh.flags & kShLimited)) rec.meta |= TGSIM_F_STAGE_D;
  return true;
}

// netem get_crandom [EXT sch_netem.c]: the next answer leans on the last one by rho / 2^32 (the
// u64 sum cannot overflow: (2^32-1)(2^32-r) + (2^32-1) r < 2^64).
__device__ __forceinline__ uint32_t crandom(uint32_t& last, uint32_t rho, uint32_t value) {
  if (rho == 0) return value;
  const uint64_t r = (uint64_t)rho + 1;
  const uint32_t ans = (uint32_t)(((uint64_t)value * ((1ull << 32) - r) + (uint64_t)last * r) >> 32);
  last = ans;
  return ans;
}

// netem_copy with the sender's correlated corrupt / reorder draws (rho[1], rho[2]; state cl).
__device__ __forceinline__ bool netem_copy_corr(const ShapeDev& sh, const uint32_t rho[3], uint32_t cl[3],
                                                const uint32_t r0[4], uint32_t src, uint32_t dst, uint32_t seq,
                                                uint32_t size, int64_t ts, uint32_t clone, uint32_t k0, uint32_t k1,
                                                tgsim_record& rec) {
  if (clone && sh.loss_t && sh.loss_t >= r0[1]) return false;
  rec.src = src; rec.dst = dst; rec.seq = seq; rec.size = size;
  rec.meta = clone ? TGSIM_F_CLONE : 0u;
  rec.corrupt_off = 0;
  if (sh.corrupt_t) {
    uint32_t r1[4];
    philox4x32_10(seq, src, clone | 2u, kNetemSalt, k0, k1, r1);
    if (sh.corrupt_t >= crandom(cl[1], rho[1], r1[0]) && size > 0) {
      rec.meta |= TGSIM_F_CORRUPT | ((r1[2] % 8u) << TGSIM_F_BIT_SHIFT);
      rec.corrupt_off = r1[1] % size;
    }
  }
  if (sh.reorder_t && !(sh.reorder_t < crandom(cl[2], rho[2], r0[3]))) {
    rec.meta |= TGSIM_F_REORDERED;
    rec.t = ts;
  } else {
    const int64_t delay = tabledist(sh.mu, sh.sigma, r0[2]);
    rec.t = ts + (delay > 0 ? delay : 0);
  }
  if (!(sh.flags & kShLimited)) rec.meta |= TGSIM_F_STAGE_D;
  return true;
}

__device__ __forceinline__ int qid_copy(const Geo& geo, const tgsim_record& r, int64_t t_end) {
  if (r.meta & TGSIM_F_STAGE_D) return qid_stage_d(geo, r.dst, r.t, t_end);
  return r.t < t_end ? Q_A : Q_L;
}

// The deferred messages' list (a.may_defer): kSharded, kDeferSub sub-lists (a queue-limit window,
// where an all-to-all round defers every message); else one list behind one counter (sc->n_corr:
// correlated senders only, few messages). Both are complete forms; the host picks by the window.
template <bool kSharded>
__device__ __forceinline__ void shape_body(const ShapeArgs& a, uint32_t bid, uint32_t nblocks) {
  DevScalars* sc = a.Q.sc;
  const int64_t H = sc->H, t_end = sc->t_end;
  uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t stride = nblocks * blockDim.x;
  uint32_t it = 0;
  // device-counted: a.n is the staged capacity, and the count never exceeds it (appenders clamp)
  const uint32_t n = a.n_dev ? min(*a.n_dev, a.n) : a.n;
  // Every load of a message is issued up front with clamped indices: one round trip for the SoA
  // record and one for the table gathers instead of a branch-serialised chain. The next message's
  // SoA record is loaded beside this one's gathers (software pipelining across the grid stride), so
  // an iteration pays one load round trip, not two.
  // Deferred messages (correlated / queue-heavy senders) are listed with one reservation per block
  // and round: an all-to-all round defers every message, and a reservation per wave serialised ~16k
  // atomics on one counter (~160 us); one per block still made a chain of ~4k memory-side atomics
  // on one line (~11 ns each: most of config 2's netem launch), so the round's chunk picks one of
  // kDeferSub sub-lists, each counter on a line of its own. The loop is block-uniform for it; lanes
  // past n idle.
  __shared__ uint32_t s_cred[kBlock / 64];
  __shared__ uint32_t s_cbase;
  uint32_t i = bid * blockDim.x + threadIdx.x;
  uint32_t n_src = 0, n_dst = 0, n_seq = 0, n_size = 0;
  int64_t n_ts = 0;
  if (i < n) { n_src = a.src[i]; n_dst = a.dst[i]; n_seq = a.seq[i]; n_size = a.size[i]; n_ts = a.t[i]; }
  for (uint32_t b0 = bid * blockDim.x; b0 < n; b0 += stride, ++it) {  // block-uniform
    i = b0 + threadIdx.x;
    const bool act = i < n;
    const uint32_t src = n_src, dst = n_dst, seq = n_seq, size = n_size;
    const int64_t ts = n_ts;
    asm volatile("" ::"v"(src), "v"(dst), "v"(seq), "v"(size), "v"((uint32_t)ts), "v"((uint32_t)((uint64_t)ts >> 32)));  // stage 1: SoA record
    {
      // clamped: the last iteration reloads itself, an idle lane message 0 (n >= 1 here)
      const uint32_t i2 = act ? (i + stride < n ? i + stride : i) : 0u;
      n_src = a.src[i2]; n_dst = a.dst[i2]; n_seq = a.seq[i2]; n_size = a.size[i2]; n_ts = a.t[i2];
    }
    const uint32_t sl = src - a.lo;
    const bool src_ok = sl < a.nloc;
    const uint32_t slc = src_ok ? sl : 0u;
    const uint32_t dstc = dst < a.geo.N ? dst : 0u;
    const uint8_t fsrc = (uint8_t)(a.ipf[src_ok ? src : a.lo] >> 32);
    // the destination's link bit from a bitmap (N bits: L2-resident even at 1M instances); its
    // address only when the sender has rules to match it against (every instance address lies in
    // the data network, so without rules any of them routes the same)
    const uint32_t fdst = (a.en_bits[dstc >> 5] >> (dstc & 31u)) & 1u;
    const uint32_t r_lo = a.rule_off[slc], r_hi = a.rule_off[slc + 1];
    const ShapeDev sh = a.shape[slc];
    asm volatile("" ::"v"((uint32_t)fsrc), "v"(fdst), "v"(r_lo), "v"(r_hi),
                 "v"((uint32_t)sh.mu), "v"((uint32_t)sh.tau), "v"(sh.sigma), "v"(sh.loss_t), "v"(sh.dup_t),
                 "v"(sh.corrupt_t), "v"(sh.reorder_t), "v"(sh.mult), "v"(sh.flags));  // stage 2: gathers
    tgsim_record r1, r2;
    int q1 = -1, q2 = -1;
    uint8_t st = 0;
    bool deferred = false;
    cnt[ST_MSGS] += act ? 1u : 0u;
    if (!act) {
      // past the staged count: nothing to decide, nothing to append
    } else if (!src_ok || (dst >= a.geo.N && dst != TGSIM_DST_EXTERNAL) || size >= 0x80000000u) {
      atomicOr(&sc->err, ERR_BAD_MSG);
      st = TGSIM_ST_UNREACHABLE;
      cnt[ST_UNREACH]++;
    } else if (ts < H || ts >= t_end) {
      atomicOr(&sc->err, ERR_CAUSAL);
      st = TGSIM_ST_UNREACHABLE;
      cnt[ST_UNREACH]++;
    } else if (dst == src) {  // loopback: unshaped
      r2.t = ts; r2.src = src; r2.dst = dst; r2.seq = seq; r2.size = size;
      r2.meta = TGSIM_F_LOCAL | TGSIM_F_STAGE_D; r2.corrupt_off = 0;
      q2 = qid_stage_d(a.geo, dst, ts, t_end);
      st = TGSIM_ST_LOCAL;
      cnt[ST_LOCAL]++;
    } else {
      const bool ext = dst == TGSIM_DST_EXTERNAL;
      const uint32_t dip = ext ? kExternalIp : (r_hi > r_lo ? (uint32_t)a.ipf[dstc] : a.data_net);
      const int rt = route_lookup(a, fsrc, r_lo, r_hi, dip);
      if (rt == R_DROP) { st = TGSIM_ST_DROPPED; cnt[ST_DROPPED]++; }
      else if (rt == R_REJECT) { st = TGSIM_ST_REJECTED; cnt[ST_REJECTED]++; }
      else if (rt == R_DEFAULT && ext) { st = TGSIM_ST_EXTERNAL; cnt[ST_EXTERNAL]++; }
      else if (rt != R_DATA) { st = TGSIM_ST_UNREACHABLE; cnt[ST_UNREACH]++; }
      else if (!(fdst & 1u)) { st = TGSIM_ST_DEST_DOWN; cnt[ST_DESTDOWN]++; }
      else if ((sh.flags & kShCorr) || a.heavy.of(sl)) { st = 0; deferred = true; }  // (t_send, seq) order: k_shape_seq
      else {
        uint32_t r0[4];
        philox4x32_10(seq, src, 0u, kNetemSalt, a.key0, a.key1, r0);
        int count = 1;
        const bool dup = sh.dup_t && sh.dup_t >= r0[0];
        if (dup) ++count;
        const bool lost = sh.loss_t && sh.loss_t >= r0[1];
        if (lost) --count;
        if (count == 0) {
          st = TGSIM_ST_LOST;
          cnt[ST_LOST]++;
        } else {
          st = TGSIM_ST_QUEUED;
          if (dup && lost) st |= TGSIM_ST_FLAG_DUP_CANCEL;
          if (count == 2) {
            st |= TGSIM_ST_FLAG_DUP;
            uint32_t c0[4];
            philox4x32_10(seq, src, 1u, kNetemSalt, a.key0, a.key1, c0);
            if (netem_copy(sh, c0, src, dst, seq, size, ts, 1u, a.key0, a.key1, r1)) {
              q1 = qid_copy(a.geo, r1, t_end);
              cnt[ST_COPIES]++;
            } else {
              st |= TGSIM_ST_FLAG_CLONE_LOST;
            }
          }
          netem_copy(sh, r0, src, dst, seq, size, ts, 0u, a.key0, a.key1, r2);
          q2 = qid_copy(a.geo, r2, t_end);
          cnt[ST_COPIES]++;
        }
      }
    }
    if (act && !deferred) a.status[i] = st;
    if (a.may_defer) {  // launch-uniform
      uint32_t tot;
      const uint32_t pos = block_excl_scan(deferred ? 1u : 0u, s_cred, tot);
      if (tot) {  // block-uniform
        if (!kSharded) {
          if (threadIdx.x == 0) s_cbase = atomicAdd(&sc->n_corr, tot);
        } else if (threadIdx.x == 0) {  // the sub-list holds its chunks of the n messages (defer_seg_cap)
          const uint32_t ds = (b0 >> 8) % (uint32_t)kDeferSub;
          s_cbase = ds * defer_seg_cap(n) + atomicAdd(a.Q.qc + ((uint32_t)(kQcDefer + ds) << 5), tot);
        }
        __syncthreads();
        if (deferred) a.corr_idx[s_cbase + pos] = i;
        __syncthreads();  // s_cbase is rewritten by the next round
      }
    }
    const int qs[2] = {q1, q2};
    const tgsim_record rs[2] = {r1, r2};
    a.Q.push_batch<2>(qs, rs, it);
  }
  // statistics: wave sums -> LDS -> one add per block into one of kNSub counter rows (128 B each),
  // so the ~8k waves of a launch do not serialise on one cache line (rows summed on read)
  __shared__ uint32_t wcnt[kBlock / 64][9];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const uint32_t v = wave_sum(cnt[c]);
    if (lane_id() == 0) wcnt[threadIdx.x >> 6][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) v += wcnt[w][threadIdx.x];
    if (v) atomicAdd(&a.stats[(blockIdx.x & (kNSub - 1)) * 16 + threadIdx.x], (unsigned long long)v);
  }
}

__global__ __launch_bounds__(kBlock) void k_shape(ShapeArgs a) { shape_body<false>(a, blockIdx.x, gridDim.x); }

// ============================================================================================
// timing wheel: plan (which slot prefixes of which live regions are due), extract, insert
// ============================================================================================

// The due slot prefix of every live region (records with time < t_end), and region retirement.
__device__ void plan_regions(RegionDev* regions, const uint32_t* dirs, uint32_t slots, int64_t slot_ns,
                             uint32_t* plan_start, uint32_t* plan_off, DevScalars* sc, int64_t t_end) {
  __shared__ uint32_t part[kBlock / 64];
  uint32_t carry = 0;  // block-uniform
  const uint32_t tid = threadIdx.x;
  const uint32_t tail = sc->reg_tail, head = sc->reg_head, nlive = head - tail;
  const int64_t kabs = t_end > 0 ? (t_end - 1) / slot_ns : -1;
  for (uint32_t base = 0; base < nlive; base += kBlock) {
    const uint32_t k = base + tid;
    uint32_t len = 0;
    if (k < nlive) {
      RegionDev& r = regions[(tail + k) % kMaxRegions];
      const uint32_t start = r.consumed;
      uint32_t hi = start;
      if (kabs >= 0) {
        const int64_t krel = kabs - r.base_slot;
        if (krel >= (int64_t)slots - 1) hi = r.n;
        else if (krel >= 0) hi = dirs[(size_t)r.dir * (slots + 1) + (uint32_t)krel + 1];
      }
      if (hi < start) hi = start;
      len = hi - start;
      r.consumed = hi;
      plan_start[k] = start;
    }
    uint32_t total;
    const uint32_t ex = block_excl_scan(len, part, total);
    if (k < nlive) plan_off[k] = carry + ex;
    carry += total;
  }
  if (tid == 0) {
    plan_off[nlive] = carry;
    sc->n_extract = carry;
    sc->plan_tail = tail;
    sc->plan_n = nlive;
    uint32_t t = tail;
    uint64_t freed = 0;
    while (t != head) {
      const RegionDev& r = regions[t % kMaxRegions];
      if (r.consumed != r.n) break;
      freed += r.n;
      ++t;
    }
    sc->reg_tail = t;
    sc->arena_used -= freed;
    sc->arena_tail = (t == head) ? sc->arena_head : regions[t % kMaxRegions].arena_off;
  }
}

constexpr uint32_t kPlanLds = 1024;  // extraction plans up to this many live regions are searched in LDS
constexpr int kExtractUnroll = 4;     // records in flight per thread

// Copies every due wheel record into A (token bucket now) / D (deliver now) / L (not yet due). The
// plan (each live region's due prefix and its place in the output) is staged in LDS, so locating
// a record costs no global round trip; kExtractUnroll records per thread are loaded before the
// wave appends.
// The extraction's share of the queue limit: due records of queue-heavy senders are also copied to
// the H list (with their sender as the group-by key) for k_shape_seq.
struct HeavyOut {
  Heavy hv;
  Geo geo;
  tgsim_record* H;
  uint32_t *hkeys, *hvals;
  uint32_t hcap, lo;
};

__device__ __forceinline__ void extract_body(const RegionDev* regions, const uint32_t* plan_start,
                                             const uint32_t* plan_off, const tgsim_record* arena, const Queues& Q,
                                             uint32_t bid, uint32_t nblocks, const HeavyOut& ho) {
  __shared__ uint32_t s_off[kPlanLds];
  __shared__ uint64_t s_src[kPlanLds];
  __shared__ uint32_t s_hred[kBlock / 64];
  __shared__ uint32_t s_hbase;
  DevScalars* sc = Q.sc;
  const uint32_t total = sc->n_extract, tail = sc->plan_tail, nl = sc->plan_n;
  const int64_t t_end = sc->t_end;
  const bool lds = nl <= kPlanLds;
  if (lds) {
    for (uint32_t k = threadIdx.x; k < nl; k += kBlock) {
      s_off[k] = plan_off[k];
      s_src[k] = regions[(tail + k) % kMaxRegions].arena_off + plan_start[k];
    }
    __syncthreads();
  }
  const uint32_t step = nblocks * kBlock * kExtractUnroll;
  uint32_t it = 0;
  for (uint32_t base = bid * kBlock * kExtractUnroll; base < total; base += step, ++it) {  // block-uniform
    tgsim_record rec[kExtractUnroll];
    // every record's place first, then every gather: a search loop after a gather starts with a wait
    // for all loads in flight (s_waitcnt vmcnt(0) at its header), which made the kExtractUnroll
    // gathers one round trip each
    uint64_t at[kExtractUnroll];
#pragma unroll
    for (int u = 0; u < kExtractUnroll; ++u) {
      uint32_t j = base + u * kBlock + threadIdx.x;
      j = j < total ? j : total - 1;  // clamped: the load stays valid, the push is skipped
      uint32_t lo = 0, hi = nl;
      if (lds) {
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_off[mid] <= j) lo = mid; else hi = mid;
        }
        at[u] = s_src[lo] + (j - s_off[lo]);
      } else {
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (plan_off[mid] <= j) lo = mid; else hi = mid;
        }
        at[u] = regions[(tail + lo) % kMaxRegions].arena_off + plan_start[lo] + (j - plan_off[lo]);
      }
    }
#pragma unroll
    for (int u = 0; u < kExtractUnroll; ++u) load_rec(arena + at[u], rec[u]);
    int qs[kExtractUnroll];
#pragma unroll
    for (int u = 0; u < kExtractUnroll; ++u) {
      const uint32_t j = base + u * kBlock + threadIdx.x;
      const bool due = j < total && rec[u].t < t_end;
      qs[u] = j >= total ? -1
                         : (due ? ((rec[u].meta & TGSIM_F_STAGE_D) ? qid_stage_d(ho.geo, rec[u].dst, rec[u].t, t_end) : Q_A)
                                : Q_L);
    }
    Q.push_batch<kExtractUnroll>(qs, rec, it);
    if (ho.hv.pend) {  // launch-uniform
      // one reservation on the H counter per block and round: every due record of an all-to-all
      // round is a heavy sender's, and a reservation per wave serialised ~16k atomics on one
      // address (~170 us of the extraction)
      bool h[kExtractUnroll];
      uint32_t nh = 0;
#pragma unroll
      for (int u = 0; u < kExtractUnroll; ++u) {
        const uint32_t j = base + u * kBlock + threadIdx.x;
        h[u] = j < total && rec[u].t < t_end && ho.hv.of(rec[u].src - ho.lo);
        nh += h[u] ? 1u : 0u;
      }
      uint32_t tot_h;
      uint32_t pos = block_excl_scan(nh, s_hred, tot_h);
      if (tot_h) {  // block-uniform
        if (threadIdx.x == 0) s_hbase = atomicAdd(&sc->n_hrec, tot_h);
        __syncthreads();
        pos += s_hbase;
#pragma unroll
        for (int u = 0; u < kExtractUnroll; ++u) {
          if (!h[u]) continue;
          if (pos < ho.hcap) {
            store_rec(ho.H + pos, rec[u]);
            ho.hkeys[pos] = rec[u].src - ho.lo;
            ho.hvals[pos] = pos;
          } else {
            atomicOr(&sc->err, ERR_QUEUE_CAP);
          }
          ++pos;
        }
        __syncthreads();  // s_hbase is rewritten by the next round
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_extract(const RegionDev* regions, const uint32_t* plan_start,
                                                    const uint32_t* plan_off, const tgsim_record* arena,
                                                    Queues Q, HeavyOut ho) {
  extract_body(regions, plan_start, plan_off, arena, Q, blockIdx.x, gridDim.x, ho);
}

// The wheel extraction and netem of the staged messages are independent (both only append to the
// A / D / L queues, through reservations), so a window with staged messages runs them as one
// launch: blocks [0, ne) extract, the rest shape. ne is a multiple of 8, so every block keeps the
// XCD (blockIdx mod 8) its sub-queue choice assumes.
// five waves per SIMD (<= 96 VGPRs, as before the exchange cursors moved; 98 made it four)
template <bool kSharded>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5))) void k_extract_shape(const RegionDev* regions, const uint32_t* plan_start,
                                                          const uint32_t* plan_off, const tgsim_record* arena,
                                                          Queues Q, ShapeArgs a, uint32_t ne, HeavyOut ho) {
  if (blockIdx.x < ne) extract_body(regions, plan_start, plan_off, arena, Q, blockIdx.x, ne, ho);
  else shape_body<kSharded>(a, blockIdx.x - ne, gridDim.x - ne);
}

// Allocate this window's region in the arena ring (one thread).
__device__ void region_alloc(DevScalars* sc, RegionDev* regions, uint64_t cap_arena, int64_t slot_ns) {
  const uint32_t n = sc->qn[Q_L];
  if (sc->reg_head - sc->reg_tail >= (uint32_t)kMaxRegions) {
    atomicOr(&sc->err, ERR_REGIONS);
    sc->ins_off = ~0ull;
    return;
  }
  uint64_t head = sc->arena_head, tail = sc->arena_tail, off;
  if (sc->arena_used == 0) {
    head = tail = 0;
    sc->arena_tail = 0;
    off = 0;
    if (n > cap_arena) { atomicOr(&sc->err, ERR_ARENA); sc->ins_off = ~0ull; return; }
  } else if (head > tail) {
    if (head + n <= cap_arena) off = head;
    else if (n <= tail) off = 0;
    else { atomicOr(&sc->err, ERR_ARENA); sc->ins_off = ~0ull; return; }
  } else {
    if (head + n <= tail) off = head;
    else { atomicOr(&sc->err, ERR_ARENA); sc->ins_off = ~0ull; return; }
  }
  const uint32_t slot = sc->reg_head % kMaxRegions;
  RegionDev r;
  r.arena_off = off; r.n = n; r.consumed = 0;
  r.base_slot = sc->t_end / slot_ns;
  r.dir = slot; r.pad = 0;
  regions[slot] = r;
  sc->reg_head += 1;
  sc->arena_head = off + n;
  sc->arena_used += n;
  if (sc->reg_head - sc->reg_tail == 1) sc->arena_tail = off;
  sc->ins_off = off;
}

// ============================================================================================
// stable LSD radix group-by on u32 keys: digits of <= 11 bits, per-block histograms, one block
// per digit to scan its per-block counts, wave64 ballot ranking in the scatter (stable).
// ============================================================================================

// Bijection of [0, n): block i -> the (i / 8)-th item of XCD i % 8's contiguous share.
__device__ __forceinline__ uint32_t xcd_major(uint32_t i, uint32_t n) {
  const uint32_t q = n >> 3, r = n & 7u, x = i & 7u;
  return x * q + (x < r ? x : r) + (i >> 3);
}

__device__ __forceinline__ void radix_range(uint32_t n, uint32_t& start, uint32_t& end, uint32_t bid) {
  uint32_t chunk = (n + kRadixBlocks - 1) / kRadixBlocks;
  chunk = (chunk + kBlock - 1) & ~(uint32_t)(kBlock - 1);
  start = bid * chunk;
  if (start > n) start = n;
  end = min(start + chunk, n);
}

__global__ __launch_bounds__(kBlock) void k_keys_sig(const uint32_t* states, const uint32_t* n_ptr, uint32_t kmin,
                                                     uint32_t* keys, uint32_t* vals) {
  const uint32_t n = *n_ptr;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    keys[i] = states[i] - kmin;
    vals[i] = i;
  }
}

// ============================================================================================
// bucketed group-by (unstable): the batch is partitioned on the bucket b = key >> bs (<= 2048
// buckets: per-block LDS histograms, one scan per bucket row, LDS-atomic ranks in the scatter),
// then one workgroup per bucket counting-sorts its <= 2^bs keys in LDS and writes the key-grouped
// (keys, vals), the segment offsets and the medium / large segment lists. Four launches and no
// per-digit ballot loop; order inside a segment is arbitrary, which is safe because every consumer
// re-sorts a segment by a key that is unique per item.
// ============================================================================================

constexpr int kBktMaxKeyBits = 13;  // keys per bucket <= 8192 (32 KB of LDS counters)
constexpr int kGlobUnroll = 8;      // items in flight per thread where one workgroup walks a whole bucket
#ifndef TGSIM_OVER_UNROLL
#define TGSIM_OVER_UNROLL 8
#endif
constexpr int kOverUnroll = TGSIM_OVER_UNROLL;  // the same in a fused consumer's oversized bucket

// Bucket of a key: b = k / w by a multiply-shift. m = ceil(2^32 / w) is exact when w is a power of
// two, and for any w while k * w < 2^32 (nloc <= 2^20, w <= 512 on the fused path).
struct BktDiv {
  uint32_t w;  // keys per bucket
  uint64_t m;
  __device__ __forceinline__ uint32_t of(uint32_t k) const { return (uint32_t)(((uint64_t)k * m) >> 32); }
};

// Input of a partition pass: a sharded record queue whose keys the producers wrote beside the
// records (Queues::key_of; block b covers a quarter of sub-queue b / 4, so no index search), or a
// precomputed (keys, vals) array (mode 3).
struct BktSrc {
  const uint32_t* keys;      // physical-index keys of queue q, or mode-3 keys
  const uint32_t* vals;      // mode 3 only
  const uint32_t* qc;        // sub-queue counters
  int q, mode;
  uint32_t subcap;
  const uint32_t* n_ptr;     // mode 3: element count
  uint32_t cap;
  RegionDev* regions;        // q == Q_L: the window's wheel region is allocated by the first block
  uint64_t cap_arena;
  int64_t slot_ns;
};

static_assert(kRadixBlocks == 4 * kNSub, "partition blocks map onto sub-queue quarters");

// This block's element range [start, end) in the physical index space of the source.
// bid: the partition block (blockIdx.x unless the pass shares its launch; queue mode only then)
__device__ __forceinline__ void bkt_block_range(const BktSrc& s, uint32_t& start, uint32_t& end,
                                                uint32_t bid = 0xFFFFFFFFu) {
  if (bid == 0xFFFFFFFFu) bid = blockIdx.x;
  if (s.mode == 3) {
    radix_range(clamp_n(s.n_ptr, s.cap), start, end, bid);
    return;
  }
  const uint32_t sub = bid >> 2, part = bid & 3;
  uint32_t c = s.qc[((uint32_t)s.q * kNSub + sub) << 5];
  c = c < s.subcap ? c : s.subcap;
  start = sub * s.subcap + (uint32_t)(((uint64_t)c * part) >> 2);
  end = sub * s.subcap + (uint32_t)(((uint64_t)c * (part + 1)) >> 2);
}

constexpr int kBktUnroll = 8;

// pass 1: per-block bucket histogram. The first block also closes the queue (prefix over its
// sub-queues, totals, overflow bit: the former k_qfinal) and, for the wheel batch, allocates the
// window's region (the former k_region_alloc).
__device__ __forceinline__ void bkt_hist_body(const BktSrc& src, DevScalars* sc, const BktDiv& bd, uint32_t B,
                                              uint32_t* hist, uint32_t bid) {
  __shared__ uint32_t h[kMaxBins];
  for (uint32_t d = threadIdx.x; d < B; d += kBlock) h[d] = 0;
  if (bid == 0) {
    // the segment lists belong to the group-bys; the wheel insert (Q_L) leaves them alone
    const bool wheel = src.mode != 3 && src.q == Q_L;
    if (threadIdx.x == 0 && !wheel) { sc->n_large = 0; sc->max_large = 0; sc->n_chunks = 0; sc->n_medium = 0; }
    if (src.mode != 3) {
      if (threadIdx.x < kNSub) queue_final(sc, src.qc, src.q, src.subcap);
      if (src.q == Q_L) {
        __syncthreads();
        if (threadIdx.x == 0) region_alloc(sc, src.regions, src.cap_arena, src.slot_ns);
      }
    }
  }
  __syncthreads();
  uint32_t start, end;
  bkt_block_range(src, start, end, bid);
  if (start == end) return;  // the scans read no row of an empty block (radix_rows_body)
  for (uint32_t j0 = start + threadIdx.x; j0 < end; j0 += kBlock * kBktUnroll) {
    uint32_t k[kBktUnroll];
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      const uint32_t j = j0 + u * kBlock;
      k[u] = j < end ? src.keys[j] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u)
      if (k[u] != 0xFFFFFFFFu) atomicAdd(&h[bd.of(k[u])], 1u);
  }
  __syncthreads();
  uint32_t* row = hist + (size_t)bid * B;
  for (uint32_t d = threadIdx.x; d < B; d += kBlock) row[d] = h[d];
}

__global__ __launch_bounds__(kBlock) void k_bkt_hist(BktSrc src, DevScalars* sc, BktDiv bd, uint32_t B,
                                                     uint32_t* hist) {
  bkt_hist_body(src, sc, bd, B, hist, blockIdx.x);
}

// Element range of partition block p (as bkt_block_range for blockIdx.x == p).
__device__ __forceinline__ void bkt_range_of(const BktSrc& s, uint32_t p, uint32_t& start, uint32_t& end) {
  const uint32_t sub = p >> 2, part = p & 3;
  uint32_t c = s.qc[((uint32_t)s.q * kNSub + sub) << 5];
  c = c < s.subcap ? c : s.subcap;
  start = sub * s.subcap + (uint32_t)(((uint64_t)c * part) >> 2);
  end = sub * s.subcap + (uint32_t)(((uint64_t)c * (part + 1)) >> 2);
}

// Partition block p's element range is non-empty.
__device__ __forceinline__ bool bkt_block_nonempty(const BktSrc& s, uint32_t p) {
  uint32_t a, e;
  bkt_block_range(s, a, e, p);
  return a < e;
}

// Per-block histograms are rows, hist[block * B + bin] (a partition block writes its own row, whole
// lines, and only when its element range is non-empty); the scan of bin d reads that column from the
// non-empty blocks only and writes the exclusive per-block offsets as row d of histx[bin *
// kRadixBlocks + block], only when the bin has items (nothing reads the offsets of an empty bin).
// Round 4 wrote every block's counts into [bin][block] columns, 4 B per line from blocks on eight
// XCDs: 8.9 MB of partial-line write-back per splitbrain window for a nearly empty wheel batch
// (VERDICT r4 item 4). bid / nbid: the scan's block index and count; bins go to XCDs in contiguous
// runs, so a line of the rows is read by one XCD.
__device__ __forceinline__ void radix_rows_body(const BktSrc& src, const uint32_t* hist, uint32_t* histx, uint32_t* tot,
                                                uint32_t B, uint32_t bid, uint32_t nbid) {
  __shared__ uint32_t ws[kRadixBlocks / 64];
  const uint32_t d = xcd_major(bid, nbid);
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t v = bkt_block_nonempty(src, t) ? hist[(size_t)t * B + d] : 0u;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if ((int)lane >= o) x += y;
  }
  if (lane == 63) ws[wave] = x;
  __syncthreads();
  uint32_t pre = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kRadixBlocks / 64; ++w) { pre += w < wave ? ws[w] : 0u; all += ws[w]; }
  if (all) histx[(size_t)d * kRadixBlocks + t] = pre + x - v;
  if (t == kRadixBlocks - 1) tot[d] = all;
}

__global__ __launch_bounds__(kRadixBlocks) void k_radix_rows(BktSrc src, const uint32_t* hist, uint32_t* histx,
                                                             uint32_t* tot, uint32_t B) {
  radix_rows_body(src, hist, histx, tot, B, blockIdx.x, gridDim.x);
}

// One-kernel partition for the fused consumers (queue sources only): each block counting-sorts
// its own element range by bucket in place of the physical index space - (key, index) to
// kv[start + rank] - and writes its exclusive bucket offsets poff[block][0..B]. No global
// scan and no cross-block scatter: a block's writes stay inside its own ~25 KB range (whole lines,
// one XCD's L2). The consumer of bucket b finds its items as 256 chunks and its global start as
// sum_p poff[p][b] (every block's offsets are prefix sums of its own counts). The first block
// also closes the queue (queue_final) and resets the segment lists.
// bid: the partition block (blockIdx.x unless the pass shares its launch).
__device__ __forceinline__ void bkt_local_body(const BktSrc& src, DevScalars* sc, const BktDiv& bd, uint32_t B,
                                               uint2* kv, uint32_t* poff, uint32_t bid = 0xFFFFFFFFu) {
  __shared__ uint32_t h[kMaxBins + 1];
  __shared__ uint32_t red[kBlock / 64];
  if (bid == 0xFFFFFFFFu) bid = blockIdx.x;
  for (uint32_t d = threadIdx.x; d <= B; d += kBlock) h[d] = 0;
  if (bid == 0) {
    if (threadIdx.x == 0) { sc->n_large = 0; sc->max_large = 0; sc->n_chunks = 0; sc->n_medium = 0; }
    if (threadIdx.x < kNSub) queue_final(sc, src.qc, src.q, src.subcap);
  }
  __syncthreads();
  uint32_t start, end;
  bkt_block_range(src, start, end, bid);
  if (start == end) return;  // no row: the consumers take an empty block's offsets as 0 (bkt_fused_load)
  for (uint32_t j0 = start + threadIdx.x; j0 < end; j0 += kBlock * kBktUnroll) {
    uint32_t k[kBktUnroll];
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      const uint32_t j = j0 + u * kBlock;
      k[u] = j < end ? src.keys[j] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u)
      if (k[u] != 0xFFFFFFFFu) atomicAdd(&h[bd.of(k[u])], 1u);
  }
  __syncthreads();
  // exclusive offsets (each thread a contiguous run of buckets), published to poff
  const uint32_t per = (B + kBlock - 1) / kBlock, d0 = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per && d0 + i < B; ++i) sum += h[d0 + i];
  uint32_t total;
  uint32_t run = block_excl_scan(sum, red, total);
  uint32_t* row = poff + (size_t)bid * (B + 1);
  for (uint32_t i = 0; i < per && d0 + i < B; ++i) {
    const uint32_t c = h[d0 + i];
    h[d0 + i] = run;
    row[d0 + i] = run;
    run += c;
  }
  if (threadIdx.x == 0) row[B] = total;
  __syncthreads();
  for (uint32_t j0 = start + threadIdx.x; j0 < end; j0 += kBlock * kBktUnroll) {
    uint32_t k[kBktUnroll];
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      const uint32_t j = j0 + u * kBlock;
      k[u] = j < end ? src.keys[j] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      if (k[u] == 0xFFFFFFFFu) continue;
      const uint32_t pos = start + atomicAdd(&h[bd.of(k[u])], 1u);
      kv[pos] = make_uint2(k[u], j0 + u * kBlock);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_bkt_local(BktSrc src, DevScalars* sc, BktDiv bd, uint32_t B,
                                                      uint2* kv, uint32_t* poff) {
  bkt_local_body(src, sc, bd, B, kv, poff);
}

// Window end, first pass: the deliveries' partition (blocks [0, kRadixBlocks), k_bkt_local on D)
// and the wheel insert's histogram (the next kRadixBlocks, k_bkt_hist on L) read different queues
// and write different buffers, so they share one launch.
__global__ __launch_bounds__(kBlock) void k_local_hist(BktSrc srcD, DevScalars* sc, BktDiv bdD, uint32_t BD,
                                                       uint2* kv, uint32_t* poff, BktSrc srcL, BktDiv bdL,
                                                       uint32_t BL, uint32_t* hist) {
  if (blockIdx.x == 0 && threadIdx.x == 0) sc->rest_tb_last = sc->rest_tb;  // 0 here unless k_rest<TB> ran alone
  if (blockIdx.x < (uint32_t)kRadixBlocks) bkt_local_body(srcD, sc, bdD, BD, kv, poff);
  else bkt_hist_body(srcL, sc, bdL, BL, hist, blockIdx.x - kRadixBlocks);
}

// Bucket bases for this block: exclusive scan of the bucket totals + this block's offset in each.
__device__ __forceinline__ void bkt_bases(uint32_t B, const uint32_t* histx, const uint32_t* tot, uint32_t* base,
                                          uint32_t* part, uint32_t bid = 0xFFFFFFFFu) {
  if (bid == 0xFFFFFFFFu) bid = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (B + kBlock - 1) / kBlock;
  const uint32_t d0 = tid * per;
  uint32_t s = 0;
  for (uint32_t k = 0; k < per && d0 + k < B; ++k) s += tot[d0 + k];
  uint32_t total;
  uint32_t run = block_excl_scan(s, part, total);
  for (uint32_t k = 0; k < per && d0 + k < B; ++k) {
    const uint32_t tk = tot[d0 + k];
    base[d0 + k] = run + (histx && tk ? histx[(size_t)(d0 + k) * kRadixBlocks + bid] : 0u);
    run += tk;
  }
  __syncthreads();
}

// One key per bucket (a fine group-by of <= 2^kMaxDigitBits keys): pass 2's buckets are the groups,
// so the scatter writes the final arrays and block 0 the key offsets and segment lists that pass 3
// (k_bkt_sort, then skipped) would have written.
struct BktDirect {
  uint32_t *off = nullptr, *off2 = nullptr, *vout2 = nullptr, *medium = nullptr;
  LargeSeg* large = nullptr;
  DevScalars* sc = nullptr;
  uint32_t medium_above = 0, on = 0, lists = 1;  // lists = 0: no medium / large segment lists
};

// pass 2: scatter (key, physical index) into bucket order (kout, vout); ranks from LDS atomics.
// bid: the partition block (the pass may share its launch).
__device__ __forceinline__ void bkt_scatter_body(const BktSrc& src, uint32_t* kout, uint32_t* vout, const BktDiv& bd,
                                                 uint32_t B, const uint32_t* histx, const uint32_t* tot,
                                                 uint32_t* bstart, const BktDirect& g, uint32_t bid) {
  __shared__ uint32_t base[kMaxBins];
  __shared__ uint32_t part[kBlock];
  uint32_t start, end;
  bkt_block_range(src, start, end, bid);
  if (start == end && bid != 0) return;  // block-uniform: nothing to place
  bkt_bases(B, histx, tot, base, part, bid);
  if (bid == 0) {  // block 0's bases are the bucket starts (its per-block offsets are 0)
    const uint32_t total = base[B - 1] + tot[B - 1];
    for (uint32_t d = threadIdx.x; d < B; d += kBlock) bstart[d] = base[d];
    if (threadIdx.x == 0) bstart[B] = total;
    if (g.on) {  // the key offsets and segment lists (bkt_global_offsets' outputs)
      for (uint32_t k = threadIdx.x; k < B; k += kBlock) {
        const uint32_t run = base[k], len = tot[k];
        g.off[k] = run;
        if (g.off2) g.off2[k] = run;
        if (!g.lists) continue;
        if (len > (uint32_t)kTile) {
          LargeSeg L;
          L.seg = k; L.start = run; L.len = len; L.pad = 0;
          g.large[atomicAdd(&g.sc->n_large, 1u)] = L;
          atomicMax(&g.sc->max_large, len);
        } else if (len > g.medium_above) {
          g.medium[atomicAdd(&g.sc->n_medium, 1u)] = k;
        }
      }
      if (threadIdx.x == 0) {
        g.off[B] = total;
        if (g.off2) g.off2[B] = total;
      }
    }
    __syncthreads();  // every base read above before the placement's atomics move them
  }
  for (uint32_t j0 = start + threadIdx.x; j0 < end; j0 += kBlock * kBktUnroll) {
    uint32_t k[kBktUnroll], v[kBktUnroll];
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      const uint32_t j = j0 + u * kBlock;
      k[u] = j < end ? src.keys[j] : 0xFFFFFFFFu;
      v[u] = src.mode == 3 ? (j < end ? src.vals[j] : 0u) : j;
    }
#pragma unroll
    for (int u = 0; u < kBktUnroll; ++u) {
      if (k[u] == 0xFFFFFFFFu) continue;
      const uint32_t pos = atomicAdd(&base[bd.of(k[u])], 1u);
      kout[pos] = k[u];
      vout[pos] = v[u];
      if (g.vout2) g.vout2[pos] = v[u];
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_bkt_scatter(BktSrc src, uint32_t* kout, uint32_t* vout, BktDiv bd, uint32_t B,
                                                        const uint32_t* histx, const uint32_t* tot, uint32_t* bstart,
                                                        BktDirect g) {
  bkt_scatter_body(src, kout, vout, bd, B, histx, tot, bstart, g, blockIdx.x);
}

// Two independent one-key-per-bucket group-bys sharing their three launches (blocks split by
// index): the queue-limit lane's deferred messages and due wheel records, both by local sender
// (six dependent launches became three).
struct BktPass {
  BktSrc src;
  BktDiv bd;
  uint32_t B;
  uint32_t *hist, *histx, *tot, *bstart, *kout, *vout;
  BktDirect g;
};
__global__ __launch_bounds__(kBlock) void k_bkt_hist_pair(BktPass a, BktPass b, DevScalars* sc) {
  if (blockIdx.x < (uint32_t)kRadixBlocks) bkt_hist_body(a.src, sc, a.bd, a.B, a.hist, blockIdx.x);
  else bkt_hist_body(b.src, sc, b.bd, b.B, b.hist, blockIdx.x - kRadixBlocks);
}
__global__ __launch_bounds__(kRadixBlocks) void k_radix_rows_pair(BktPass a, BktPass b) {
  if (blockIdx.x < a.B) radix_rows_body(a.src, a.hist, a.histx, a.tot, a.B, blockIdx.x, a.B);
  else radix_rows_body(b.src, b.hist, b.histx, b.tot, b.B, blockIdx.x - a.B, b.B);
}
__global__ __launch_bounds__(kBlock) void k_bkt_scatter_pair(BktPass a, BktPass b) {
  if (blockIdx.x < (uint32_t)kRadixBlocks)
    bkt_scatter_body(a.src, a.kout, a.vout, a.bd, a.B, a.histx, a.tot, a.bstart, a.g, blockIdx.x);
  else
    bkt_scatter_body(b.src, b.kout, b.vout, b.bd, b.B, b.histx, b.tot, b.bstart, b.g, blockIdx.x - kRadixBlocks);
}

// pass 3 pieces. bkt_count_keys: the bucket's start / size (sum of the totals before it) and the
// exclusive offsets of its keys in cnt[] (relative to the bucket start); returns the longest segment.
struct BktHead { uint32_t start, nb, k0, nk, b; };
__device__ __forceinline__ uint32_t bkt_count_body(const uint32_t* kin, uint32_t* cnt, uint32_t* part,
                                                   const BktHead& h);

__device__ __forceinline__ uint32_t bkt_count_keys(const uint32_t* kin, BktDiv bd, uint32_t K, const uint32_t* tot,
                                                   uint32_t* cnt, uint32_t* part, BktHead& h) {
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  h.b = b;
  h.k0 = b * bd.w;
  h.nk = min(K - h.k0, bd.w);
  uint32_t s = 0;
  for (uint32_t d = tid; d < b; d += kBlock) s += tot[d];
  part[tid] = s;
  for (uint32_t i = tid; i < h.nk; i += kBlock) cnt[i] = 0;
  __syncthreads();
  for (uint32_t o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  h.start = part[0];
  h.nb = tot[b];
  __syncthreads();
  return bkt_count_body(kin, cnt, part, h);
}

// Counting part of bkt_count_keys (h known, cnt[0, h.nk) zeroed and visible): key counts of the
// bucket's items kin[h.start, +h.nb), exclusive offsets in cnt[], and the longest segment.
__device__ __forceinline__ uint32_t bkt_scan_counts(uint32_t* cnt, uint32_t* part, const BktHead& h);
template <int U = kGlobUnroll, class KeyAt>
__device__ __forceinline__ uint32_t bkt_count_f(const KeyAt& key_at, uint32_t* cnt, uint32_t* part, const BktHead& h) {
  const uint32_t tid = threadIdx.x;
  // U keys in flight per thread: one workgroup walks an oversized bucket alone (a probed target's
  // 10k-request inbox), and a load per iteration made that a chain of ~40 latencies
  for (uint32_t j0 = tid; j0 < h.nb; j0 += kBlock * U) {
    uint32_t k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t j = j0 + u * kBlock;
      k[u] = j < h.nb ? key_at(j) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k[u] != 0xFFFFFFFFu) atomicAdd(&cnt[k[u] - h.k0], 1u);
  }
  __syncthreads();
  return bkt_scan_counts(cnt, part, h);
}
// key counts cnt[0, h.nk) -> exclusive offsets; returns the longest segment
__device__ __forceinline__ uint32_t bkt_scan_counts(uint32_t* cnt, uint32_t* part, const BktHead& h) {
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (h.nk + kBlock - 1) / kBlock, i0 = tid * per;
  uint32_t sum = 0, mx = 0;
  for (uint32_t i = 0; i < per && i0 + i < h.nk; ++i) {
    sum += cnt[i0 + i];
    mx = max(mx, cnt[i0 + i]);
  }
  uint32_t total;
  uint32_t run = block_excl_scan(sum, part, total);
  for (uint32_t i = 0; i < per && i0 + i < h.nk; ++i) {
    const uint32_t len = cnt[i0 + i];
    cnt[i0 + i] = run;
    run += len;
  }
  __syncthreads();
  // block max of the segment lengths (part[] is free again)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o));
  if (lane_id() == 0) part[tid >> 6] = mx;
  __syncthreads();
  uint32_t m = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) m = max(m, part[w]);
  __syncthreads();
  return m;
}
__device__ __forceinline__ uint32_t bkt_count_body(const uint32_t* kin, uint32_t* cnt, uint32_t* part,
                                                   const BktHead& h) {
  return bkt_count_f([&](uint32_t j) { return kin[h.start + j]; }, cnt, part, h);
}

// Global form of pass 3 (after bkt_count_keys): (kout, vout) grouped by key, off[k] (+ off2),
// medium (medium_above < len <= kTile) / large (len > kTile) segment lists.
constexpr uint32_t kNoMedium = 0xFFFFFFFFu;
// medium_above = kMediumSpans: the bucket's keys go to k_rest in groups of G consecutive keys, G the
// power of two that puts about kTile / 2 items in a group at the bucket's mean run length: a group of
// at most kTile items is one medium entry, g | (G' - 1) << kSpanKeyShift, sorted by one block in LDS
// (span_sort handles several segments); a fuller group lists its keys one by one (its long keys are
// large segments as always). An overflowing fused bucket listed every key alone: a flood of two
// publications per wave put ~10^6 keys of 2-30 items through k_rest one block each, 8 ms a window.
// (A first form grew each span key by key up to a kTile stretch: that serial walk cost config 3's
// probed-target bucket 1.5 us.)
constexpr uint32_t kMediumSpans = 0xFFFFFFFEu;
constexpr uint32_t kSpanKeyShift = 21;  // keys < 2^21 (nloc <= 2^20); <= 2^11 keys per span
constexpr uint32_t kSpanKeyMask = (1u << kSpanKeyShift) - 1u;
__device__ __forceinline__ void bkt_global_offsets(const uint32_t* cnt, const BktHead& h, uint32_t* off, uint32_t* off2,
                                                   uint32_t medium_above, uint32_t* medium, LargeSeg* large,
                                                   DevScalars* sc);
template <int U = kGlobUnroll, class ItemAt>
__device__ __forceinline__ void bkt_emit_global_f(const ItemAt& item_at, uint32_t* kout, uint32_t* vout, uint32_t B,
                                                  uint32_t K, uint32_t* cnt, const BktHead& h, uint32_t* off,
                                                  uint32_t* off2, uint32_t medium_above, uint32_t* medium,
                                                  LargeSeg* large, DevScalars* sc, uint32_t* vout2 = nullptr) {
  const uint32_t tid = threadIdx.x;
  bkt_global_offsets(cnt, h, off, off2, medium_above, medium, large, sc);
  for (uint32_t j0 = tid; j0 < h.nb; j0 += kBlock * U) {
    uint2 e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t j = j0 + u * kBlock;
      e[u] = j < h.nb ? item_at(j) : make_uint2(0xFFFFFFFFu, 0u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e[u].x == 0xFFFFFFFFu) continue;
      const uint32_t pos = h.start + atomicAdd(&cnt[e[u].x - h.k0], 1u);
      kout[pos] = e[u].x;
      vout[pos] = e[u].y;
      if (vout2) vout2[pos] = e[u].y;
    }
  }
}
// the global form's key offsets off[k] (+ off2) and its medium / large segment lists
__device__ __forceinline__ void bkt_global_offsets(const uint32_t* cnt, const BktHead& h, uint32_t* off, uint32_t* off2,
                                                   uint32_t medium_above, uint32_t* medium, LargeSeg* large,
                                                   DevScalars* sc) {
  const uint32_t tid = threadIdx.x;
  const auto len_of = [&](uint32_t i) { return (i + 1 < h.nk ? cnt[i + 1] : h.nb) - cnt[i]; };
  uint32_t G = 1;  // keys per span group (kMediumSpans)
  if (medium_above == kMediumSpans && h.nk) {
    const uint32_t mean = max(h.nb / h.nk, 1u);
    while (G < 512u && 2u * G * mean <= (uint32_t)kTile / 2u) G <<= 1;
  }
  for (uint32_t i = tid; i < h.nk; i += kBlock) {
    const uint32_t a = cnt[i];
    const uint32_t len = len_of(i);
    const uint32_t k = h.k0 + i, run = h.start + a;
    off[k] = run;
    if (off2) off2[k] = run;
    if (len > (uint32_t)kTile) {
      const uint32_t li = atomicAdd(&sc->n_large, 1u);
      LargeSeg L;
      L.seg = k; L.start = run; L.len = len; L.pad = 0;
      large[li] = L;
      atomicMax(&sc->max_large, len);
    } else if (medium_above != kMediumSpans && len > medium_above) {  // kNoMedium: never
      medium[atomicAdd(&sc->n_medium, 1u)] = k;
    }
    if (medium_above == kMediumSpans && (i & (G - 1u)) == 0) {  // the group's head lists it
      const uint32_t e = min(i + G, h.nk), items = (e < h.nk ? cnt[e] : h.nb) - a;
      if (G > 1 && items <= (uint32_t)kTile) {
        if (items) medium[atomicAdd(&sc->n_medium, 1u)] = k | ((e - i - 1) << kSpanKeyShift);
      } else {
        for (uint32_t j = i; j < e; ++j) {
          const uint32_t l = len_of(j);
          if (l && l <= (uint32_t)kTile) medium[atomicAdd(&sc->n_medium, 1u)] = h.k0 + j;
        }
      }
    }
  }
  // the end of this bucket's last segment: a neighbouring bucket on the fused path writes offsets
  // only for its own long keys, so the boundary must not be left to it (same value if it does)
  if (tid == 0) {
    off[h.k0 + h.nk] = h.start + h.nb;
    if (off2) off2[h.k0 + h.nk] = h.start + h.nb;
  }
  __syncthreads();
}
__device__ __forceinline__ void bkt_emit_global(const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
                                                uint32_t* vout, uint32_t B, uint32_t K, uint32_t* cnt,
                                                const BktHead& h, uint32_t* off, uint32_t* off2,
                                                uint32_t medium_above, uint32_t* medium, LargeSeg* large,
                                                DevScalars* sc, uint32_t* vout2) {
  bkt_emit_global_f([&](uint32_t j) { return make_uint2(kin[h.start + j], vin[h.start + j]); }, kout, vout, B, K, cnt,
                    h, off, off2, medium_above, medium, large, sc, vout2);
}

// pass 3: one workgroup per bucket, global form only (signals, and > 2^bs-key fallbacks); vout2, if
// given, receives a second copy of the values.
__global__ __launch_bounds__(kBlock) void k_bkt_sort(const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
                                                     uint32_t* vout, BktDiv bd, uint32_t B, uint32_t K,
                                                     const uint32_t* tot, uint32_t* off, uint32_t* off2,
                                                     uint32_t medium_above, uint32_t* medium, LargeSeg* large,
                                                     DevScalars* sc, uint32_t* vout2) {
  __shared__ uint32_t cnt[1u << kBktMaxKeyBits];
  __shared__ uint32_t part[kBlock];
  BktHead h;
  bkt_count_keys(kin, bd, K, tot, cnt, part, h);
  bkt_emit_global(kin, vin, kout, vout, B, K, cnt, h, off, off2, medium_above, medium, large, sc, vout2);
}

// Wheel insert with buckets = slots (slots <= kMaxBins): records are copied straight from the L
// batch into this window's arena region in slot order, and the slot directory is the scan. The
// first block also closes the window's counters (the former k_finish).
#ifndef TG_WHEEL_UNROLL
#define TG_WHEEL_UNROLL 8
#endif
constexpr int kWheelUnroll = TG_WHEEL_UNROLL;

// Queue occupancy: a record entering the wheel for the first time (no
// TGSIM_F_WHEEL) is counted in its sender's pend and marked; runs of one sender among a wave's 64
// consecutive records share one atomic (the token bucket stages its output grouped by sender). The
// atomics return nothing, so no wave waits on them.
__device__ __forceinline__ void pend_count_wave(PendRef pend, uint32_t lo, uint32_t nloc, uint32_t src, bool add) {
  const uint32_t lane = lane_id();
  const uint32_t key = add && src - lo < nloc ? src - lo : 0xFFFFFFFFu;
  const uint32_t prev = __shfl_up(key, 1);
  const bool head = key != 0xFFFFFFFFu && (lane == 0 || prev != key);
  const uint64_t heads = __ballot(head);
  const uint64_t valid = __ballot(key != 0xFFFFFFFFu);
  if (head) {
    // the run: this lane and the following lanes with the same key (heads end it)
    const uint64_t after = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
    const uint32_t end = after ? (uint32_t)__ffsll((unsigned long long)after) - 1u : 64u;
    const uint64_t span = (end >= 64 ? ~0ull : ((1ull << end) - 1)) & ~((1ull << lane) - 1);
    __hip_atomic_fetch_add(&pend[key], (uint32_t)__popcll(valid & span), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The host's exact refresh of its occupancy bound: max over local senders of pend, per block into
// part[blockIdx.x] (the host folds the kRadixBlocks partials; one atomicMax per block on one address
// serialised ~1000 blocks: 14.7 us plus a memset per refresh, config 5). TCP mode: mult * (pend + pending retransmissions), which
// bounds mult * the sender's unsettled segments (tgsim_tcp.hip). TCP acks mode (refreshed every
// window): pend + mult * (retransmissions released into the window + the deliveries the sender got
// last window, each answered by at most one ACK).
__global__ __launch_bounds__(kBlock) void k_pend_max(PendRef pend, const uint32_t* retx, const uint32_t* inbox,
                                                     uint32_t inbox_mult, uint32_t mult, uint32_t nloc, uint32_t* part) {
  __shared__ uint32_t red[kBlock / 64];
  uint32_t mx = 0;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < nloc; i += gridDim.x * kBlock) {
    uint64_t v = pend[i];
    if (inbox) v += (uint64_t)mult * ((uint64_t)retx[i] + (uint64_t)inbox_mult * (inbox[i + 1] - inbox[i]));
    else if (retx) v = (uint64_t)mult * (v + retx[i]);
    mx = max(mx, (uint32_t)min<uint64_t>(v, 0xFFFFFFFFull));
  }
  mx = wave_max(mx);
  if (lane_id() == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// The window's counters close once the window end's passes have run: the deliveries, the staged
// count the next netem pass reads, the statistics (first block of the insert launch, or of the
// long-inbox launch when the insert runs on the side stream).
__device__ __forceinline__ void close_window_counters(DevScalars* sc) {
  const uint32_t n = sc->qn[Q_D];
  sc->n_out = n;
  sc->n_msgs_last = sc->n_msgs_dev;  // the shape pass of this window has read it
  sc->n_msgs_dev = 0;
  sc->st[ST_DELIVERED] += n;
  sc->st[ST_TB_ITEMS] += sc->qn[Q_A];
  sc->st[ST_EXTRACTED] += sc->n_extract;
  sc->st[ST_INSERTED] += sc->qn[Q_L];
}

__device__ __forceinline__ void wheel_scatter_body(const BktSrc& src, DevScalars* sc, const tgsim_record* L,
                                                   tgsim_record* arena, uint32_t* dirs, uint32_t slots,
                                                   const uint32_t* histx, const uint32_t* tot, PendRef pend,
                                                   uint32_t lo, uint32_t nloc, bool close = true) {
  __shared__ uint32_t base[kMaxBins];
  __shared__ uint32_t part[kBlock];
  const uint64_t off = sc->ins_off;
  if (blockIdx.x == 0) {
    if (close && threadIdx.x == 0) close_window_counters(sc);
    if (off != ~0ull) {
      bkt_bases(slots, nullptr, tot, base, part);
      const uint32_t dir = (sc->reg_head - 1) % kMaxRegions;
      for (uint32_t s = threadIdx.x; s < slots; s += kBlock) dirs[(size_t)dir * (slots + 1) + s] = base[s];
      if (threadIdx.x == 0) dirs[(size_t)dir * (slots + 1) + slots] = sc->qn[Q_L];
      __syncthreads();
    }
  }
  if (off == ~0ull) return;  // region allocation failed (error bit set)
  uint32_t start, end;
  bkt_block_range(src, start, end);
  if (start == end) return;  // block-uniform: nothing to insert
  bkt_bases(slots, histx, tot, base, part);
  // kWheelUnroll records in flight per thread; out-of-range lanes load a clamped (valid) record so
  // the arrays stay in registers (a conditional load, or HIP's uint4 wrapper, left them in scratch)
  for (uint32_t j0 = start + threadIdx.x; j0 < end; j0 += kBlock * kWheelUnroll) {
    uint32_t k[kWheelUnroll];
    v4u32 ra[kWheelUnroll], rb[kWheelUnroll];
#pragma unroll
    for (int u = 0; u < kWheelUnroll; ++u) {
      const uint32_t j = j0 + u * kBlock;
      const bool in = j < end;
      k[u] = in ? src.keys[j] : 0xFFFFFFFFu;
      const v4u32* p = reinterpret_cast<const v4u32*>(L + (in ? j : j0));
      ra[u] = p[0];
      rb[u] = p[1];
    }
#pragma unroll
    for (int u = 0; u < kWheelUnroll; ++u) {
      const bool fresh = k[u] != 0xFFFFFFFFu && !(rb[u].z & TGSIM_F_WHEEL);
#ifndef TG_EXP_NO_SCATTER_INC
      pend_count_wave(pend, lo, nloc, ra[u].z, fresh);
#endif
      if (k[u] != 0xFFFFFFFFu) {
        const uint32_t pos = atomicAdd(&base[k[u]], 1u);
        v4u32* q = reinterpret_cast<v4u32*>(arena + off + pos);
        v4u32 b = rb[u];
        b.z |= TGSIM_F_WHEEL;
        st4(q, ra[u].x, ra[u].y, ra[u].z, ra[u].w);
        st4(q + 1, b.x, b.y, b.z, b.w);
      }
    }
  }
}

// ============================================================================================
// segmented sorts: LDS rank sort (short segments) / bitonic (up to kTile) per span, and a
// chunk sort + merge path for segments longer than kTile
// ============================================================================================

struct SortSmem {
  uint64_t k1[kSpan];
  uint64_t k2[kSpan];
  uint32_t sg[kSpan];
  uint32_t k3[kSpan];
  uint32_t perm[kSpan];  // sorted position -> element
  int64_t scA[kBlock];
  int64_t scB[kBlock];
  int64_t carry;
  uint32_t maxlen;
  uint32_t pad;
};

__device__ __forceinline__ bool el_less(const SortSmem& s, uint32_t a, uint32_t b) {
  return key_less(s.sg[a], s.k1[a], s.k2[a], s.k3[a], s.sg[b], s.k1[b], s.k2[b], s.k3[b]);
}

__device__ __forceinline__ void bitonic_lds(SortSmem& s, uint32_t npad) {
  for (uint32_t k = 2; k <= npad; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < (npad >> 1); p += kBlock) {
        const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const uint32_t l = i + j;
        const bool up = (i & k) == 0;
        if (el_less(s, l, i) == up) {
          uint32_t ts = s.sg[i]; s.sg[i] = s.sg[l]; s.sg[l] = ts;
          uint64_t t1 = s.k1[i]; s.k1[i] = s.k1[l]; s.k1[l] = t1;
          uint64_t t2 = s.k2[i]; s.k2[i] = s.k2[l]; s.k2[l] = t2;
          uint32_t t3 = s.k3[i]; s.k3[i] = s.k3[l]; s.k3[l] = t3;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ void pad_key(SortSmem& s, uint32_t j) {
  s.sg[j] = 0xFFFFFFFFu; s.k1[j] = ~0ull; s.k2[j] = ~0ull; s.k3[j] = 0xFFFFFFFFu;
}

// Sort the m loaded elements of s (whole segments, contiguous in sg order) into perm[] (sorted
// position -> element), the arrays staying in place; npad = next_pow2(m). Returns false, touching
// nothing, when k1 spreads too far over the elements to pack.
#ifdef TGSIM_PHASE_PROF
// debug: the last chunk sort's keys-loaded and sorted clocks, then the last 1024-key packed sort's
// clocks after min/max, packing, the network and the restore, and whether it packed
__device__ uint64_t g_chunk_ph[8];
#define PB_PH(i) do { if (threadIdx.x == 0 && m == 1024) g_chunk_ph[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PB_PH(i) do {} while (0)
#endif
// Bucket sort of the packed keys nk (this thread's elements p0 .. p0 + PER - 1, < m real) when they
// spread evenly: bucket = (key - min) >> sh over 1024 buckets (counts in scA / scB), one LDS atomic
// per element for its slot, a block scan of the counts, each element's id at its bucket slot in
// perm, then every element ranks itself among its bucket mates (packed key, then (k2, k3) as the
// network's ties) and takes its place. Leaves perm = sorted order and k1 restored by element, as
// packed_bitonic does; returns false - having written only scA / scB and perm - when some bucket
// holds more than kBucketMax elements (clustered keys: the network is the better form). The network
// took ~22 us per 1024-key chunk (55 stages, a barrier each: DESIGN.md 5, splitbrain's long inbox).
constexpr uint32_t kBucketMax = 32;
constexpr uint32_t kBuckets = 2 * kBlock * sizeof(int64_t) / sizeof(uint32_t);  // scA + scB as u32
static_assert(kBuckets == 1024, "1024 buckets in scA / scB");
__device__ __forceinline__ bool packed_bucket(SortSmem& s, uint32_t m, const uint64_t (&nk)[kSpan / kBlock],
                                              uint32_t p0, uint32_t lo, uint32_t b1, uint64_t mn) {
  constexpr uint32_t PER = kSpan / kBlock, BPT = kBuckets / kBlock;
  __shared__ uint32_t s_big;
  uint64_t kmn = ~0ull, kmx = 0;
  for (uint32_t u = 0; u < PER; ++u)
    if (p0 + u < m) { kmn = nk[u] < kmn ? nk[u] : kmn; kmx = nk[u] > kmx ? nk[u] : kmx; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = __shfl_xor(kmn, o), b = __shfl_xor(kmx, o);
    kmn = a < kmn ? a : kmn;
    kmx = b > kmx ? b : kmx;
  }
  if ((threadIdx.x & 63) == 0) { s.scA[threadIdx.x >> 6] = (int64_t)kmn; s.scB[threadIdx.x >> 6] = (int64_t)kmx; }
  if (threadIdx.x == 0) s_big = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const uint64_t a = (uint64_t)s.scA[w], b = (uint64_t)s.scB[w];
    kmn = a < kmn ? a : kmn;
    kmx = b > kmx ? b : kmx;
  }
  __syncthreads();  // scA / scB become the counts
  const uint64_t d = kmx - kmn;
  const uint32_t bits = d ? 64u - (uint32_t)__builtin_clzll(d) : 0u;
  const uint32_t sh = bits > 10u ? bits - 10u : 0u;  // (d >> sh) < 1024
  uint32_t* C = reinterpret_cast<uint32_t*>(s.scA);
  for (uint32_t i = 0; i < BPT; ++i) C[threadIdx.x * BPT + i] = 0;
  __syncthreads();
  uint32_t bk[PER], sl[PER];
  for (uint32_t u = 0; u < PER; ++u) {
    bk[u] = p0 + u < m ? (uint32_t)((nk[u] - kmn) >> sh) : 0u;
    sl[u] = p0 + u < m ? atomicAdd(&C[bk[u]], 1u) : 0u;
  }
  __syncthreads();
  uint32_t c4 = 0;
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t c = C[threadIdx.x * BPT + i];
    c4 += c;
    if (c > kBucketMax) s_big = 1u;
  }
  uint32_t tot;
  uint32_t run = block_excl_scan(c4, s.perm, tot);  // its barriers publish s_big
  if (s_big) {
    __syncthreads();  // perm (the scan's scratch) is rewritten by the network's setup
    return false;     // block-uniform
  }
  __syncthreads();  // the scan's reads of perm are done
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t c = C[threadIdx.x * BPT + i];
    C[threadIdx.x * BPT + i] = run;
    run += c;
  }
  uint64_t* kw = s.k1;  // the packed keys, by element
  for (uint32_t u = 0; u < PER; ++u)
    if (p0 + u < m) kw[p0 + u] = nk[u];
  __syncthreads();
  for (uint32_t u = 0; u < PER; ++u)
    if (p0 + u < m) s.perm[C[bk[u]] + sl[u]] = p0 + u;
  __syncthreads();
  uint32_t pos[PER];
  for (uint32_t u = 0; u < PER; ++u) {
    const uint32_t j = p0 + u;
    pos[u] = 0xFFFFFFFFu;
    if (j >= m) continue;
    const uint32_t a = C[bk[u]], e = bk[u] + 1u < kBuckets ? C[bk[u] + 1u] : m;
    const uint64_t x = nk[u], x2 = s.k2[j];
    const uint32_t x3 = s.k3[j];
    uint32_t r = 0;
    for (uint32_t i = a; i < e; ++i) {
      const uint32_t q = s.perm[i];
      const uint64_t y = kw[q];
      r += (y < x || (y == x && (s.k2[q] < x2 || (s.k2[q] == x2 && s.k3[q] < x3)))) ? 1u : 0u;
    }
    pos[u] = a + r;
  }
  __syncthreads();  // every bucket read before the places are written
  const uint64_t m1 = b1 ? (~0ull >> (64u - b1)) : 0ull;
  for (uint32_t u = 0; u < PER; ++u) {
    if (pos[u] == 0xFFFFFFFFu) continue;
    s.perm[pos[u]] = p0 + u;
    kw[p0 + u] = (lo < 64u ? ((nk[u] >> lo) & m1) : 0ull) + mn;  // k1 restored by element
  }
  __syncthreads();
  return true;
}

__device__ bool packed_bitonic(SortSmem& s, uint32_t m, uint32_t npad) {
    PB_PH(2);
    // k1's spread over the span: below 2^52 the sort runs on (segment rank | k1 - min | the top
    // bits of k2, element) pairs - one u64 compare per step, two arrays swapped instead of four - the
    // rank and k1 fields as wide as the span needs, k2's leading bits in the rest (a probed target's
    // ~10k requests share their arrival times, and every tie went through the elements' k2 / k3: a
    // 1024-element chunk took ~40 us). Equal packed keys (same segment, k1 and k2 top) are ordered by
    // (k2, k3) through the elements. The packed keys live in k1's array (it has no spare LDS: every
    // kernel that reaches rest_body allocates this struct) and k1 is restored by element afterwards.
    uint64_t mn = ~0ull, mx = 0;
    for (uint32_t j = threadIdx.x; j < m; j += kBlock) {
      mn = s.k1[j] < mn ? s.k1[j] : mn;
      mx = s.k1[j] > mx ? s.k1[j] : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) { s.scA[threadIdx.x >> 6] = (int64_t)mn; s.scB[threadIdx.x >> 6] = (int64_t)mx; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const uint64_t a = (uint64_t)s.scA[w], b = (uint64_t)s.scB[w];
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    __syncthreads();  // scA / scB are free again
    PB_PH(3);
    if (!(mx - mn < (1ull << 52))) return false;
    {
      uint64_t* kw = s.k1;
      // segment rank of each position: segment starts up to it, minus one (m <= kSpan = 2^11)
      constexpr uint32_t PER = kSpan / kBlock;
      const uint32_t p0 = threadIdx.x * PER;
      uint32_t c = 0;
      for (uint32_t u = 0; u < PER; ++u) {
        const uint32_t j = p0 + u;
        c += (j < m && j > 0 && s.sg[j] != s.sg[j - 1]) ? 1u : 0u;
      }
      uint32_t tot;
      uint32_t r = block_excl_scan(c, s.perm, tot);  // perm is scratch until it is filled below
      // field widths (block-uniform): rank rb <= 11 bits (tot <= kSpan - 1), k1 b1 <= 52, k2 the rest
      const uint32_t rb = tot ? 32u - (uint32_t)__builtin_clz(tot) : 0u;
      const uint64_t spread = mx - mn;
      const uint32_t b1 = spread ? 64u - (uint32_t)__builtin_clzll(spread) : 0u;
      const uint32_t lo = 64u - rb - b1;  // >= 1
      uint64_t nk[PER];
      for (uint32_t u = 0; u < PER; ++u) {
        const uint32_t j = p0 + u;
        nk[u] = ~0ull;  // padding: sorts after every real key (ties with one go by element, below)
        if (j < m) {
          r += (j > 0 && s.sg[j] != s.sg[j - 1]) ? 1u : 0u;
          const uint64_t hi = rb ? ((uint64_t)r << (64u - rb)) : 0ull;
          const uint64_t mid = lo < 64u ? ((s.k1[j] - mn) << lo) : 0ull;
          nk[u] = hi | mid | (s.k2[j] >> (64u - lo));
        }
      }
      __syncthreads();  // every k1 read before the packed keys replace them
      if (packed_bucket(s, m, nk, p0, lo, b1, mn)) {
        PB_PH(6);
        return true;
      }
      for (uint32_t u = 0; u < PER; ++u) {
        const uint32_t j = p0 + u;
        if (j < npad) { kw[j] = nk[u]; s.perm[j] = j < m ? j : 0xFFFFFFFFu; }
      }
      __syncthreads();
      PB_PH(4);
      for (uint32_t k = 2; k <= npad; k <<= 1) {
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
          for (uint32_t q = threadIdx.x; q < (npad >> 1); q += kBlock) {
            const uint32_t i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1));
            const uint32_t l = i + jj;
            const bool up = (i & k) == 0;
            const uint64_t ki = kw[i], kl = kw[l];
            const uint32_t ei = s.perm[i], el = s.perm[l];
            bool lt;  // element at l sorts before the one at i
            if (kl != ki) lt = kl < ki;
            else if (el == 0xFFFFFFFFu || ei == 0xFFFFFFFFu) lt = el < ei;  // padding (never ties a real key)
            else lt = s.k2[el] != s.k2[ei] ? s.k2[el] < s.k2[ei] : s.k3[el] < s.k3[ei];
            if (lt == up) {
              kw[i] = kl; kw[l] = ki;
              s.perm[i] = el; s.perm[l] = ei;
            }
          }
          __syncthreads();
        }
      }
      PB_PH(5);
      // restore k1 by element: sorted position i holds element perm[i]'s key
      uint32_t ee[PER];
      const uint64_t m1 = b1 ? (~0ull >> (64u - b1)) : 0ull;
      for (uint32_t u = 0; u < PER; ++u) {
        const uint32_t i = p0 + u;
        ee[u] = 0xFFFFFFFFu;
        if (i < m) { ee[u] = s.perm[i]; nk[u] = (lo < 64u ? ((kw[i] >> lo) & m1) : 0ull) + mn; }
      }
      __syncthreads();
      for (uint32_t u = 0; u < PER; ++u)
        if (ee[u] != 0xFFFFFFFFu) s.k1[ee[u]] = nk[u];
    }
    __syncthreads();
    PB_PH(6);
    return true;
}

// Sort m loaded elements (whole segments, contiguous) and leave perm[] = sorted order.
// off/s_begin give each element's segment bounds (global positions).
__device__ __forceinline__ void span_sort(SortSmem& s, uint32_t m, const uint32_t* off, uint32_t s_begin) {
  if (threadIdx.x == 0) s.maxlen = 0;
  __syncthreads();
  uint32_t ml = 0;
  for (uint32_t j = threadIdx.x; j < m; j += kBlock) {
    const uint32_t g = s.sg[j];
    const uint32_t len = off[g + 1] - off[g];
    ml = len > ml ? len : ml;
  }
  ml = wave_max(ml);
  if ((threadIdx.x & 63) == 0) atomicMax(&s.maxlen, ml);
  __syncthreads();
  if (s.maxlen <= (uint32_t)kRankSortMax) {
    // O(len) rank per element inside its segment; keys are unique (k3 carries the index)
    for (uint32_t j = threadIdx.x; j < m; j += kBlock) {
      const uint32_t g = s.sg[j];
      const uint32_t a = off[g] - s_begin, b = off[g + 1] - s_begin;
      uint32_t r = 0;
      for (uint32_t i = a; i < b; ++i) r += el_less(s, i, j) ? 1u : 0u;
      s.perm[a + r] = j;
    }
  } else {
    const uint32_t npad = next_pow2(m);
    if (!packed_bitonic(s, m, npad)) {
      for (uint32_t j = m + threadIdx.x; j < npad; j += kBlock) pad_key(s, j);
      __syncthreads();
      bitonic_lds(s, npad);
      for (uint32_t j = threadIdx.x; j < m; j += kBlock) s.perm[j] = j;
    }
  }
  __syncthreads();
}

// The sort keys of (keys, vals)[st, st + cnt) into LDS positions [0, cnt), padding up to npad: four
// elements per thread with every level of their loads (pair, then the policy's gather) in flight
// together - a loop of one element at a time was a chain of 2 x 4 dependent round trips per chunk.
template <class P>
__device__ __forceinline__ void load_span_keys(const P& p, SortSmem& s, const uint32_t* keys, const uint32_t* vals,
                                               uint32_t st, uint32_t cnt, uint32_t npad) {
  constexpr int U = 4;
  if (cnt == 0) {
    for (uint32_t j = threadIdx.x; j < npad; j += kBlock) pad_key(s, j);
    return;
  }
  for (uint32_t j0 = threadIdx.x; j0 < npad; j0 += kBlock * U) {
    uint32_t kk[U], vv[U], sg[U], k3[U];
    uint64_t k1[U], k2[U];
    // unconditional loads (a lane past the end re-reads the last element): behind a branch per
    // element, each gather waited for every load before it (s_waitcnt vmcnt(0)) - U serial round
    // trips instead of one
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t j = min(j0 + u * kBlock, cnt - 1);
      kk[u] = keys[st + j];
      vv[u] = vals[st + j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) p.key(kk[u], vv[u], sg[u], k1[u], k2[u], k3[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t j = j0 + u * kBlock;
      if (j < cnt) { s.sg[j] = sg[u]; s.k1[j] = k1[u]; s.k2[j] = k2[u]; s.k3[j] = k3[u]; }
      else if (j < npad) pad_key(s, j);
    }
  }
}

template <class P>
__global__ __launch_bounds__(kBlock) void k_seg_small(P p, const uint32_t* keys, const uint32_t* vals,
                                                      const uint32_t* off, const uint32_t* n_ptr,
                                                      uint32_t cap) {
  __shared__ SortSmem s;
  const uint32_t n = clamp_n(n_ptr, cap);
  const uint32_t ntiles = (n + kTile - 1) / kTile;
  for (uint32_t w = blockIdx.x; w < ntiles; w += gridDim.x) {
    const uint32_t a = w * kTile, b = min(a + kTile, n);
    const uint32_t s_begin = (a == 0 || keys[a] != keys[a - 1]) ? a : off[keys[a] + 1];
    uint32_t s_next = (b >= n) ? n : ((keys[b] != keys[b - 1]) ? b : off[keys[b] + 1]);
    if (s_begin >= s_next) continue;
    const uint32_t kl = keys[s_next - 1];
    if (off[kl + 1] - off[kl] > (uint32_t)kTile) s_next = off[kl];
    if (s_next <= s_begin) continue;
    const uint32_t m = s_next - s_begin;
    load_span_keys(p, s, keys, vals, s_begin, m, m);
    __syncthreads();
    span_sort(s, m, off, s_begin);
    p.epilogue(s, m, s_begin, off, w);
    __syncthreads();
  }
}

__device__ __forceinline__ bool kless(const uint64_t* K1, const uint64_t* K2, const uint32_t* K3,
                                      uint32_t x, uint32_t y) {
  return key_less(0, K1[x], K2[x], K3[x], 0, K1[y], K2[y], K3[y]);
}

// ============================================================================================
// (2) token bucket: HTB as GCRA, X_i = min(max(X_{i-1}, e_i - tau) + c_i, 2^61), d_i = max(e_i, X_{i-1}).
// Each step is the max-plus affine map x -> max(min(x + A, K), B); maps compose associatively, so
// a block scan over the sorted span gives every d_i. A == kNegInf marks a constant map (segment head).
// ============================================================================================

struct MP { int64_t A, B; };

__device__ __forceinline__ int64_t sadd(int64_t a, int64_t b) {
  if (a == kNegInf || b == kNegInf) return kNegInf;
  const int64_t s = a + b;
  return s > kTbClamp ? kTbClamp : s;
}
__device__ __forceinline__ MP mp_then(MP e, MP l) {  // l after e
  MP r;
  r.A = sadd(e.A, l.A);
  const int64_t eb = sadd(e.B, l.A);
  r.B = eb > l.B ? eb : l.B;
  return r;
}
__device__ __forceinline__ int64_t mp_apply(MP f, int64_t x) {
  if (f.A == kNegInf || x == kNegInf) return f.B;
  int64_t v = x + f.A;
  v = v > kTbClamp ? kTbClamp : v;
  return v > f.B ? v : f.B;
}

template <class Sh>
__device__ __forceinline__ uint64_t l2t_ns(const Sh& sh, uint32_t len) {
  const uint64_t c = ((uint64_t)len * sh.mult) >> sh.shift;
  return c > kCostClamp ? kCostClamp : c;
}

struct TBPolicy {
  const tgsim_record* A;
  const TbShape* shape;
  int64_t* X;
  PendRef pend;  // queue occupancy: a wheel copy leaving now (D / X) no longer counts
  uint32_t lo;
  Geo geo;
  Queues Q;
  const DevScalars* sc;

  __device__ __forceinline__ void key(uint32_t seg, uint32_t idx, uint32_t& sg, uint64_t& k1, uint64_t& k2,
                                      uint32_t& k3) const {
    const uint4 a = reinterpret_cast<const uint4*>(A + idx)[0];
    const uint4 b = reinterpret_cast<const uint4*>(A + idx)[1];
    sg = seg;
    k1 = ((uint64_t)a.y << 32) | a.x;                               // netem time_to_send (>= 0)
    k2 = ((uint64_t)b.x << 1) | ((b.z & TGSIM_F_CLONE) ? 0u : 1u);  // seq, clone first
    k3 = idx;
  }

  // Scan m sorted items (element perm[j] at sorted position j; segments contiguous).
  // has_carry: the first item continues a segment whose X before it is `carry`.
  // final: the last item ends its segment. salt: wave-uniform append salt.
  __device__ void scan(SortSmem& s, uint32_t m, bool has_carry, int64_t carry, bool final, uint32_t salt) const {
    const int64_t t_end = sc->t_end;
    const uint32_t IT = (m + kBlock - 1) / kBlock;
    const uint32_t j0 = threadIdx.x * IT;
    // phase 1: per-thread aggregate
    MP agg = {0, kNegInf};
    for (uint32_t u = 0; u < IT; ++u) {
      const uint32_t j = j0 + u;
      if (j >= m) break;
      const uint32_t e_ = s.perm[j];
      const uint32_t sl = s.sg[j];
      const TbShape& sh = shape[sl];
      const int64_t e = (int64_t)s.k1[e_];
      const int64_t c = (int64_t)l2t_ns(sh, A[s.k3[e_]].size);
      const bool head = (j == 0) ? !has_carry : (s.sg[j - 1] != sl);
      MP f;
      if (head) {
        const int64_t xs = X[sl];
        const int64_t b = xs > e - sh.tau ? xs : e - sh.tau;
        const int64_t v = b + c;
        f.A = kNegInf; f.B = v > kTbClamp ? kTbClamp : v;
      } else {
        f.A = c;
        const int64_t v = e - sh.tau + c;
        f.B = v > kTbClamp ? kTbClamp : v;
      }
      agg = mp_then(agg, f);
    }
    s.scA[threadIdx.x] = agg.A;
    s.scB[threadIdx.x] = agg.B;
    __syncthreads();
    // phase 2: inclusive Hillis-Steele scan of the 256 aggregates
    for (uint32_t o = 1; o < kBlock; o <<= 1) {
      MP v = {0, kNegInf};
      const bool has = threadIdx.x >= o;
      if (has) { v.A = s.scA[threadIdx.x - o]; v.B = s.scB[threadIdx.x - o]; }
      MP me = {s.scA[threadIdx.x], s.scB[threadIdx.x]};
      __syncthreads();
      if (has) { me = mp_then(v, me); s.scA[threadIdx.x] = me.A; s.scB[threadIdx.x] = me.B; }
      __syncthreads();
    }
    MP P = {0, kNegInf};
    if (has_carry) { P.A = kNegInf; P.B = carry; }
    if (threadIdx.x > 0) {
      const MP prev = {s.scA[threadIdx.x - 1], s.scB[threadIdx.x - 1]};
      P = mp_then(P, prev);
    }
    // phase 3: per item d = max(e, X_prev), route the departed copy
    for (uint32_t u = 0; u < IT; ++u) {
      const uint32_t j = j0 + u;
      tgsim_record rec;
      int q = -1;
      if (j < m) {
        const uint32_t e_ = s.perm[j];
        const uint32_t sl = s.sg[j];
        const TbShape& sh = shape[sl];
        const int64_t e = (int64_t)s.k1[e_];
        load_rec(A + s.k3[e_], rec);
        const int64_t c = (int64_t)l2t_ns(sh, rec.size);
        const bool head = (j == 0) ? !has_carry : (s.sg[j - 1] != sl);
        int64_t xprev;
        MP f;
        if (head) {
          xprev = X[sl];
          const int64_t b = xprev > e - sh.tau ? xprev : e - sh.tau;
          const int64_t v = b + c;
          f.A = kNegInf; f.B = v > kTbClamp ? kTbClamp : v;
        } else {
          xprev = mp_apply(P, kNegInf);
          f.A = c;
          const int64_t v = e - sh.tau + c;
          f.B = v > kTbClamp ? kTbClamp : v;
        }
        P = mp_then(P, f);
        s.k2[e_] = (uint64_t)mp_apply(P, kNegInf);  // X after this item (written back below)
        if (j + 1 == m) s.carry = mp_apply(P, kNegInf);
        rec.t = e > xprev ? e : xprev;
        rec.meta |= TGSIM_F_STAGE_D;
        q = qid_stage_d(geo, rec.dst, rec.t, t_end);
        if ((rec.meta & TGSIM_F_WHEEL) && q != Q_L) {
          rec.meta &= ~(uint32_t)TGSIM_F_WHEEL;
          atomicSub(&pend[rec.src - lo], 1u);
        }
      }
      Q.push(q, rec, salt + u);
    }
    __syncthreads();  // every head has read X before any segment end overwrites it
    for (uint32_t u = 0; u < IT; ++u) {
      const uint32_t j = j0 + u;
      if (j >= m) break;
      const bool last = (j + 1 == m) ? final : (s.sg[j + 1] != s.sg[j]);
      if (last) X[s.sg[j]] = (int64_t)s.k2[s.perm[j]];
    }
    __syncthreads();
  }

  __device__ void epilogue(SortSmem& s, uint32_t m, uint32_t, const uint32_t*, uint32_t w) const {
    scan(s, m, false, 0, true, w * 16);
  }
};

// Exclusive block scan of two per-thread counts; totals returned to every thread. red: [2 * waves].
__device__ __forceinline__ void block_scan2(uint32_t& v0, uint32_t& v1, uint32_t* red, uint32_t& t0, uint32_t& t1) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t x0 = v0, x1 = v1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y0 = __shfl_up(x0, o), y1 = __shfl_up(x1, o);
    if ((int)lane >= o) { x0 += y0; x1 += y1; }
  }
  if (lane == 63) { red[2 * wave] = x0; red[2 * wave + 1] = x1; }
  __syncthreads();
  uint32_t p0 = 0, p1 = 0;
  t0 = 0; t1 = 0;
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    const uint32_t a0 = red[2 * w], a1 = red[2 * w + 1];
    if (w < wave) { p0 += a0; p1 += a1; }
    t0 += a0; t1 += a1;
  }
  v0 = p0 + x0 - v0;
  v1 = p1 + x1 - v1;
}

// ============================================================================================
// (3) deliveries: inbox order (dst, t, src, seq, clone-first), written as SoA
// ============================================================================================

struct EmitPolicy {
  const tgsim_record* D;
  PendRef pend;  // queue occupancy: a delivered wheel copy of a local sender no longer counts
  uint32_t lo, nloc;
  int64_t* o_t;
  uint32_t *o_src, *o_dst, *o_seq, *o_size, *o_flags, *o_coff;

  __device__ __forceinline__ void key(uint32_t seg, uint32_t idx, uint32_t& sg, uint64_t& k1, uint64_t& k2,
                                      uint32_t& k3) const {
    const uint4 a = reinterpret_cast<const uint4*>(D + idx)[0];
    const uint4 b = reinterpret_cast<const uint4*>(D + idx)[1];
    sg = seg;
    k1 = ((uint64_t)a.y << 32) | a.x;
    k2 = ((uint64_t)a.z << 32) | b.x;
    k3 = (((b.z & TGSIM_F_CLONE) ? 0u : 1u) << 31) | idx;
  }
  __device__ __forceinline__ void write(uint32_t pos, uint32_t k3) const {
    tgsim_record r;
    load_rec(D + (k3 & 0x7FFFFFFFu), r);
    put(pos, r);
  }
  __device__ __forceinline__ void put(uint32_t pos, const tgsim_record& r) const {
    if ((r.meta & TGSIM_F_WHEEL) && r.src - lo < nloc) atomicSub(&pend[r.src - lo], 1u);
    o_t[pos] = r.t; o_src[pos] = r.src; o_dst[pos] = r.dst; o_seq[pos] = r.seq; o_size[pos] = r.size;
    o_flags[pos] = r.meta & ~(uint32_t)(TGSIM_F_STAGE_D | TGSIM_F_WHEEL); o_coff[pos] = r.corrupt_off;
  }
  __device__ void epilogue(SortSmem& s, uint32_t m, uint32_t s_begin, const uint32_t*, uint32_t) const {
    for (uint32_t j = threadIdx.x; j < m; j += kBlock) write(s_begin + j, s.k3[s.perm[j]]);
  }
};


// ============================================================================================
// fused bucket consumers: one workgroup per bucket of <= 2^kBktFusedKeyBits keys finishes the
// group-by in LDS and consumes it there. The bucket's items stay in the registers of the thread
// that gathered them (kIPT per thread), so a workgroup's critical path is four memory round trips:
// bucket bounds (+ the senders' shape / token state), item list, one 32-B gather per item, the
// output reservation. In between, all in LDS: counting sort by key, rank inside each key's run
// (O(run) compares), and the policy (GCRA along each sender's run / delivery position).
// A bucket holding more than kBktCap items, and any key longer than kBktRankMax, is written out in
// key order instead and listed for k_rest (medium / large segments).
// ============================================================================================

// 1536 items per bucket keep a workgroup at 40 KB of LDS and 112-118 VGPRs, so four buckets share a
// CU (2048 items: 52.7 KB, three per CU); the fourth workgroup's memory phases overlap the others'
// LDS-bound ranking: storm step -8.7 %, flood -5.5 %. 1024 items / five per CU made
// the consumers faster still but overflowed the flood's buckets (1M senders: ~900 items each).
#ifndef TG_BKT_CAP
#define TG_BKT_CAP 1536
#endif
#ifndef TG_STAGE_N
#define TG_STAGE_N 960
#endif
#ifndef TG_BKT_WGS_PER_CU
#define TG_BKT_WGS_PER_CU 4
#endif
constexpr int kBktCap = TG_BKT_CAP;   // items of one bucket held by the workgroup
#ifndef TG_BKT_KEY_BITS
#define TG_BKT_KEY_BITS 9
#endif
constexpr int kBktFusedKeyBits = TG_BKT_KEY_BITS;   // keys per bucket on the fused path (log2)
#ifndef TGSIM_BKT_RANK_MAX
#define TGSIM_BKT_RANK_MAX 512
#endif
constexpr uint32_t kBktRankMax = TGSIM_BKT_RANK_MAX;  // longest key run ranked in LDS
constexpr int kIPT = kBktCap / kBlock;  // items per thread

constexpr uint32_t kStageN = TG_STAGE_N;  // records staged per round for the coalesced output (k1 + k2 + k3 area:
                                    // a storm bucket of ~1.1k copies leaves in one round)

struct BktFusedSmem {
  uint32_t cnt[1u << kBktFusedKeyBits];  // per key: run start, then run end (relative to the bucket)
  uint64_t k1[kBktCap];                  // TB: netem time, then departure; emit: delivery time
  uint64_t k2[kBktCap];                  // TB: seq << 32 | !clone << 31 | size; emit: src << 32 | seq
  uint32_t k3[kBktCap];                  // batch index (emit: | !clone << 31)
  uint16_t key[kBktCap];                 // key of each slot, relative to the bucket's first key
  uint16_t ord[kBktCap];                 // by_pos: sorted position -> slot; else slot -> sorted position
                                         // (TB, after the GCRA: per key, wheel copies leaving the queue)
  uint32_t part[kBlock];
  uint32_t maxlen, flag;
#ifdef TGSIM_PHASE_PROF
  uint64_t ph[10];
  uint64_t w0;
#endif
};
#ifdef TGSIM_PHASE_PROF
#define TG_PH(i) do { if (threadIdx.x == 0) { if ((i) == 0) sm.w0 = wall_clock64(); sm.ph[i] = clock64(); } } while (0)
__device__ uint64_t g_tg_ph[2][1024][12];
#define TG_PH_END(kid, nb) do { __syncthreads(); if (threadIdx.x == 0 && blockIdx.x < 1024) { sm.ph[8] = clock64(); \
  uint64_t* o = g_tg_ph[kid][blockIdx.x]; o[0] = nb; for (int i_ = 0; i_ < 8; ++i_) o[1 + i_] = sm.ph[i_ + 1] - sm.ph[i_]; \
  o[9] = sm.w0; o[10] = wall_clock64(); o[11] = gridDim.x; } } while (0)
#else
#define TG_PH(i) do {} while (0)
#define TG_PH_END(name, nb) do {} while (0)
#endif

__device__ __forceinline__ bool k3less(uint64_t a1, uint64_t a2, uint32_t a3, uint64_t b1, uint64_t b2, uint32_t b3) {
  if (a1 != b1) return a1 < b1;
  if (a2 != b2) return a2 < b2;
  return a3 < b3;
}

// The bucket's items, one gathered record per item in the registers of its thread. On return
// (true): slot[u] is item u's LDS slot, sm.cnt[k] the END of key k's run, sm.ord the sorted order
// of every key run of length <= kBktRankMax (by_pos: position -> slot, else slot -> position); longer runs are written out (kout, vout,
// off) and listed. false: the bucket was too big and went to the global form (k_rest).

// chunk of item j: the last chunk p with cexcl[p] <= j (cexcl ascending, cexcl[0] = 0)
__device__ __forceinline__ uint32_t chunk_of(const uint32_t* cexcl, uint32_t j) {
  uint32_t lo = 0, hi = kRadixBlocks;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cexcl[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

static_assert(kRadixBlocks == kBlock, "one consumer thread per partition block");

template <bool by_pos, class KeyFn>
__device__ __forceinline__ bool bkt_fused_load(const BktSrc& src, const uint32_t* poff, const uint2* kv,
                                               uint32_t* kscr, uint32_t* vscr, uint32_t* kout,
                                               uint32_t* vout, BktDiv bd, uint32_t B, uint32_t K, uint32_t* off,
                                               uint32_t* off2, uint32_t* medium, LargeSeg* large, DevScalars* sc,
                                               BktFusedSmem& sm, BktHead& h, const tgsim_record* batch,
                                               const KeyFn& keyfn, tgsim_record (&rec)[kIPT],
                                               uint32_t (&slot)[kIPT]) {
  // XCD-aware bucket order: hardware dispatch puts block i on XCD i % 8, so consecutive buckets -
  // whose chunks share cache lines in every partition block's range - go to the same XCD's L2
  const uint32_t b = xcd_major(blockIdx.x, B);
  h.b = b;
  TG_PH(0);
  h.k0 = b * bd.w;
  h.nk = min(K - h.k0, bd.w);
  // chunk table (in the k1 area, free until the sort keys are written): partition block p left
  // this bucket's items at kv[csrc[p] ...), cexcl[p] items of the bucket before them
  uint32_t* cexcl = reinterpret_cast<uint32_t*>(sm.k1);
  uint32_t* csrc = cexcl + kRadixBlocks;
  {
    const uint32_t p = threadIdx.x;
    uint32_t ps, pe;
    // the row is read beside the sub-queue counter, not after it (one global round trip, not two):
    // every partition block has a row allocated, and what an empty block's row holds is masked
    const uint32_t* row = poff + (size_t)p * (B + 1);
    const uint32_t rlo = row[b], rhi = row[b + 1];
    bkt_range_of(src, p, ps, pe);
    const bool live = ps < pe;  // an empty partition block wrote no row (bkt_local_body)
    const uint32_t lo = live ? rlo : 0u, hi = live ? rhi : 0u;
    uint32_t c = hi - lo, l = lo, tc, tl;
    block_scan2(c, l, sm.part, tc, tl);  // c: items before chunk p; tc: bucket size; tl: bucket start
    cexcl[p] = c;
    csrc[p] = ps + lo;
    h.nb = tc;
    h.start = tl;
  }
  for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock) sm.cnt[i] = 0;
  if (threadIdx.x == 0) sm.maxlen = 0;
  __syncthreads();
  TG_PH(1);
#ifdef TGSIM_BKT_COPY3
  if (h.nb > (uint32_t)kBktCap) {  // every key of the bucket goes to k_rest: contiguous copy first
    for (uint32_t j0 = threadIdx.x; j0 < h.nb; j0 += kBlock * kGlobUnroll) {
      uint2 e[kGlobUnroll];
#pragma unroll
      for (int u = 0; u < kGlobUnroll; ++u) {
        const uint32_t j = min(j0 + u * kBlock, h.nb - 1);  // clamped: the load stays valid
        const uint32_t p = chunk_of(cexcl, j);
        e[u] = kv[csrc[p] + (j - cexcl[p])];
      }
#pragma unroll
      for (int u = 0; u < kGlobUnroll; ++u) {
        const uint32_t j = j0 + u * kBlock;
        if (j < h.nb) { kscr[h.start + j] = e[u].x; vscr[h.start + j] = e[u].y; }
      }
    }
    __syncthreads();
    (void)bkt_count_body(kscr, sm.cnt, sm.part, h);
    bkt_emit_global(kscr, vscr, kout, vout, B, K, sm.cnt, h, off, off2, 0, medium, large, sc, nullptr);
    return false;
  }
#endif
  if (h.nb > (uint32_t)kBktCap) {  // every key of the bucket goes to k_rest
    // two passes straight over the partition's chunks, thread p walking chunk p's contiguous items
    // (no item -> chunk search): key counts, then the grouped scatter. A contiguous copy first (and
    // a search per item) cost a third pass over the bucket: a probed target's 10k-request inbox,
    // walked by this one workgroup
    const uint32_t p = threadIdx.x;
    const uint32_t cn = (p + 1 < (uint32_t)kRadixBlocks ? cexcl[p + 1] : h.nb) - cexcl[p];
    const uint2* run = kv + csrc[p];
    for (uint32_t i0 = 0; i0 < cn; i0 += kOverUnroll) {
      uint32_t k[kOverUnroll];
#pragma unroll
      for (int u = 0; u < kOverUnroll; ++u) k[u] = i0 + u < cn ? run[i0 + u].x : 0xFFFFFFFFu;
#pragma unroll
      for (int u = 0; u < kOverUnroll; ++u)
        if (k[u] != 0xFFFFFFFFu) atomicAdd(&sm.cnt[k[u] - h.k0], 1u);
    }
    __syncthreads();
    (void)bkt_scan_counts(sm.cnt, sm.part, h);
    bkt_global_offsets(sm.cnt, h, off, off2, kMediumSpans, medium, large, sc);
    for (uint32_t i0 = 0; i0 < cn; i0 += kOverUnroll) {
      uint2 e[kOverUnroll];
#pragma unroll
      for (int u = 0; u < kOverUnroll; ++u) e[u] = i0 + u < cn ? run[i0 + u] : make_uint2(0xFFFFFFFFu, 0u);
#pragma unroll
      for (int u = 0; u < kOverUnroll; ++u) {
        if (e[u].x == 0xFFFFFFFFu) continue;
        const uint32_t pos = h.start + atomicAdd(&sm.cnt[e[u].x - h.k0], 1u);
        kout[pos] = e[u].x;
        vout[pos] = e[u].y;
      }
    }
    (void)kscr; (void)vscr;
    return false;
  }
  // this thread's items (strided: consecutive positions used to leave half the threads idle)
  uint32_t kk[kIPT], ix[kIPT];
  // item u of this thread is bucket position threadIdx.x + u * kBlock: every thread of the block
  // issues loads (a bucket of ~1k items fills 4 rounds of 256 threads, not 131 threads x 8)
#pragma unroll
  for (int u = 0; u < kIPT; ++u) {
    const uint32_t j = threadIdx.x + (uint32_t)u * kBlock;
    kk[u] = 0xFFFFFFFFu;
    ix[u] = 0;
    if (j < h.nb) {
      const uint32_t p = chunk_of(cexcl, j);
      const uint2 e = kv[csrc[p] + (j - cexcl[p])];
      kk[u] = e.x - h.k0;
      ix[u] = e.y;
    }
  }

#pragma unroll
  for (int u = 0; u < kIPT; ++u)
    if (kk[u] != 0xFFFFFFFFu) load_rec(batch + ix[u], rec[u]);  // issued before the LDS work below
  __syncthreads();  // the chunk table (k1 area) is dead from here
  TG_PH(2);
#pragma unroll
  for (int u = 0; u < kIPT; ++u)
    if (kk[u] != 0xFFFFFFFFu) atomicAdd(&sm.cnt[kk[u]], 1u);
  __syncthreads();
  TG_PH(3);
  // exclusive scan of the key counts (each thread a contiguous run of keys) + longest run
  const uint32_t per = (h.nk + kBlock - 1) / kBlock, i0 = threadIdx.x * per;
  uint32_t sum = 0, mx = 0;
  for (uint32_t i = 0; i < per && i0 + i < h.nk; ++i) { sum += sm.cnt[i0 + i]; mx = max(mx, sm.cnt[i0 + i]); }
  mx = wave_max(mx);  // one LDS atomic per wave, not one per key
  if (mx && (threadIdx.x & 63) == 0) atomicMax(&sm.maxlen, mx);
  uint32_t total;
  uint32_t run = block_excl_scan(sum, sm.part, total);
  for (uint32_t i = 0; i < per && i0 + i < h.nk; ++i) {
    const uint32_t len = sm.cnt[i0 + i];
    sm.cnt[i0 + i] = run;
    run += len;
  }
  __syncthreads();
  TG_PH(4);
  // slots + sort keys (from the registers: no second gather)
#pragma unroll
  for (int u = 0; u < kIPT; ++u) {
    slot[u] = 0xFFFFFFFFu;
    if (kk[u] == 0xFFFFFFFFu) continue;
    const uint32_t s = atomicAdd(&sm.cnt[kk[u]], 1u);
    slot[u] = s;
    keyfn(rec[u], ix[u], sm.k1[s], sm.k2[s], sm.k3[s]);
    sm.key[s] = (uint16_t)kk[u];
  }
  __syncthreads();  // cnt[k] is now the END of key k's run
  TG_PH(5);
  // rank inside the run. With four workgroups per CU the LDS latency is covered by the other waves;
  // what the phase costs is instructions issued (measured: two slots per trip with eight loads in
  // flight was 20 % slower). So the loop over the run only counts, per comparand one
  // compare-and-add each for "earlier" and "equal" on k1; a tie is then a slot that counted an
  // equal entry besides itself, and only such slots walk their run again for the full-key order.
  for (uint32_t s = threadIdx.x; s < h.nb; s += kBlock) {
    const uint32_t k = sm.key[s];
    const uint32_t a = k ? sm.cnt[k - 1] : 0u, e = sm.cnt[k];
    if (e - a > kBktRankMax) continue;
    const uint64_t x1 = sm.k1[s];
    uint32_t r = 0, eq = 0, i = a;
    for (; i + 4 <= e; i += 4) {
      uint64_t y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = sm.k1[i + j];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r += y[j] < x1 ? 1u : 0u;
        eq += y[j] == x1 ? 1u : 0u;
      }
    }
    if (i < e) {  // the last one to three: one masked group (loads clamped to the run), not a loop
      const uint32_t n = e - i;
      const uint64_t y0 = sm.k1[i], y1 = sm.k1[n > 1 ? i + 1 : i], y2 = sm.k1[n > 2 ? i + 2 : i];
      r += y0 < x1 ? 1u : 0u;
      eq += y0 == x1 ? 1u : 0u;
      r += n > 1 && y1 < x1 ? 1u : 0u;
      eq += n > 1 && y1 == x1 ? 1u : 0u;
      r += n > 2 && y2 < x1 ? 1u : 0u;
      eq += n > 2 && y2 == x1 ? 1u : 0u;
    }
    if (eq > 1) {  // ties on k1 (the slot itself is one equal entry): the rest of the key decides
      const uint64_t x2 = sm.k2[s];
      const uint32_t x3 = sm.k3[s];
      for (i = a; i < e; ++i)
        if (i != s && sm.k1[i] == x1) r += k3less(x1, sm.k2[i], sm.k3[i], x1, x2, x3) ? 1u : 0u;
    }
    if (by_pos) sm.ord[a + r] = (uint16_t)s;
    else sm.ord[s] = (uint16_t)(a + r);
  }
  if (sm.maxlen > kBktRankMax) {  // block-uniform: write the long keys out for k_rest
    for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock) {
      const uint32_t a = i ? sm.cnt[i - 1] : 0u, len = sm.cnt[i] - a;
      if (len <= kBktRankMax) continue;
      const uint32_t k = h.k0 + i, g = h.start + a;
      for (uint32_t u = 0; u < len; ++u) { kout[g + u] = k; vout[g + u] = sm.k3[a + u] & 0x7FFFFFFFu; }
      off[k] = g;
      off[k + 1] = g + len;
      if (len > (uint32_t)kTile) {
        const uint32_t li = atomicAdd(&sc->n_large, 1u);
        LargeSeg L;
        L.seg = k; L.start = g; L.len = len; L.pad = 0;
        large[li] = L;
        atomicMax(&sc->max_large, len);
      } else {
        medium[atomicAdd(&sc->n_medium, 1u)] = k;
      }
    }
  }
  __syncthreads();
  TG_PH(6);
  return true;
}

static_assert(offsetof(BktFusedSmem, k2) == offsetof(BktFusedSmem, k1) + 8 * kBktCap &&
                  offsetof(BktFusedSmem, k3) == offsetof(BktFusedSmem, k2) + 8 * kBktCap &&
                  32 * kStageN <= 20 * kBktCap, "output staging uses the k1 + k2 + k3 area");

// length of the run of the key owning LDS slot s
__device__ __forceinline__ uint32_t run_len(const BktFusedSmem& sm, uint32_t s) {
  const uint32_t k = sm.key[s];
  return sm.cnt[k] - (k ? sm.cnt[k - 1] : 0u);
}

struct TBKey {
  __device__ __forceinline__ void operator()(const tgsim_record& r, uint32_t idx, uint64_t& k1, uint64_t& k2,
                                             uint32_t& k3) const {
    k1 = (uint64_t)r.t;                                                                  // netem time_to_send
    k2 = ((uint64_t)r.seq << 32) | ((r.meta & TGSIM_F_CLONE) ? 0u : 0x80000000u) | r.size;  // seq, clone first, size
    k3 = idx;
  }
};

__global__ __launch_bounds__(kBlock) void k_tb_bucket(TBPolicy p, BktSrc src, const uint32_t* poff,
                                                      const uint2* kv, uint32_t* kscr,
                                                      uint32_t* vscr, uint32_t* kout, uint32_t* vout, BktDiv bd,
                                                      uint32_t B, uint32_t K, uint32_t* off, uint32_t* medium,
                                                      LargeSeg* large, DevScalars* sc) {
  __shared__ BktFusedSmem sm;
  BktHead h;
  tgsim_record rec[kIPT];
  uint32_t slot[kIPT];
  if (!bkt_fused_load<true>(src, poff, kv, kscr, vscr, kout, vout, bd, B, K, off, nullptr, medium, large, sc,
                            sm, h, p.A, TBKey{}, rec, slot)) {
    if (threadIdx.x == 0) sc->rest_tb = 1u;  // the bucket's keys are listed for k_rest<TB>
    return;
  }
  if (sm.maxlen > kBktRankMax && threadIdx.x == 0) sc->rest_tb = 1u;  // so are its long keys
  // the GCRA along each sender's run (one thread per sender); departures replace k1
  for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock) {
    const uint32_t a = i ? sm.cnt[i - 1] : 0u, e = sm.cnt[i];
    if (e == a || e - a > kBktRankMax) continue;
    const uint32_t sl = h.k0 + i;
    const TbShape sh = p.shape[sl];
    int64_t x = p.X[sl];
    for (uint32_t r = a; r < e; ++r) {
      const uint32_t s = sm.ord[r];
      const int64_t t = (int64_t)sm.k1[s];
      uint64_t c = ((uint64_t)(sm.k2[s] & 0x7FFFFFFFu) * sh.mult) >> sh.shift;
      c = c > kCostClamp ? kCostClamp : c;
      const int64_t d = t > x ? t : x;
      const int64_t b0 = x > t - sh.tau ? x : t - sh.tau;
      const int64_t v = b0 + (int64_t)c;
      x = v > kTbClamp ? kTbClamp : v;
      sm.k1[s] = (uint64_t)d;
    }
    p.X[sl] = x;
  }
  __syncthreads();
  // the run order is consumed: its LDS counts, per key, the wheel copies that leave the queue now
  static_assert(sizeof(BktFusedSmem::ord) >= 4u << kBktFusedKeyBits, "dec fits the ord area");
  uint32_t* dec = reinterpret_cast<uint32_t*>(sm.ord);
  for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock) dec[i] = 0;
  __syncthreads();
  TG_PH(7);
  // route each departed copy from the registers (D now, L later, X another shard); one
  // reservation per queue for the whole block
  const int64_t t_end = sc->t_end;
  int code[kIPT];
  uint32_t nX = 0;
#pragma unroll
  for (int u = 0; u < kIPT; ++u) {
    code[u] = -1;
    if (slot[u] == 0xFFFFFFFFu || run_len(sm, slot[u]) > kBktRankMax) continue;
    rec[u].t = (int64_t)sm.k1[slot[u]];
    rec[u].meta |= TGSIM_F_STAGE_D;
    code[u] = qid_stage_d(p.geo, rec[u].dst, rec[u].t, t_end);
    nX += code[u] >= Q_X0;
    if ((rec[u].meta & TGSIM_F_WHEEL) && code[u] != Q_L) {  // leaves its sender's queue now
      rec[u].meta &= ~(uint32_t)TGSIM_F_WHEEL;
      atomicAdd(&dec[sm.key[slot[u]]], 1u);
    }
  }
  // staging slots, so that the lanes of a staging store hold neighbouring records (slots contiguous
  // per thread put neighbouring lanes' 32-B records ~128 B apart: 8-way LDS bank conflicts). D by
  // consumer group (an LDS counting sort: lanes of one group get consecutive slots) - each output
  // line then holds records that one XCD's emit workgroups read (Queues::group_of) -, L in
  // (wave, item, lane) order from ballots.
  const Queues& Q = p.Q;
  // the staged output's two record bases, two key bases and the window's base_slot (k_window_start
  // wrote it; this launch comes later), in scalar registers before the loops: see pin_scalar
  tgsim_record *const outD = pin_scalar(Q.D), *const outL = pin_scalar(Q.L);
  uint32_t *const keyD = pin_scalar(Q.KD), *const keyL = pin_scalar(Q.KL);
  const int64_t base_slot = uniform_i64(Q.sc->base_slot);
  uint32_t* gcnt = sm.part + 2 * (kBlock / 64);  // [8] D records per consumer group, then offsets
  uint32_t rkD[kIPT];
  uint64_t mL[kIPT];
  uint32_t wL = 0;
#pragma unroll
  for (int u = 0; u < kIPT; ++u) {
    mL[u] = __ballot(code[u] == Q_L);
    wL += (uint32_t)__popcll(mL[u]);
  }
  const uint32_t wave = threadIdx.x >> 6;
  // cross-shard copies (S > 1): per peer an LDS count (each copy's rank in it), its offset in the
  // block's X run and one reservation per workgroup on the peer's cursor, sm.part[64 / 128 / 192 + p]
  uint32_t* xcnt = sm.part + 64;
  uint32_t* xbase = sm.part + 128;
  uint32_t* xoff = sm.part + 192;
  static_assert(kBlock >= 192 + kMaxShards, "exchange counts fit sm.part");
  if (threadIdx.x == 0) sm.flag = 0;
  if (threadIdx.x < 8) gcnt[threadIdx.x] = 0;
  if (threadIdx.x < kMaxShards) xcnt[threadIdx.x] = 0;
  if ((threadIdx.x & 63) == 0) sm.part[kBlock / 64 + wave] = wL;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kIPT; ++u) {
    rkD[u] = 0;
    if (code[u] == Q_D) {
      const uint32_t g = Q.group_of(rec[u].dst - p.lo);
      rkD[u] = (g << 24) | atomicAdd(&gcnt[g], 1u);
    } else if (code[u] >= Q_X0) {
      rkD[u] = atomicAdd(&xcnt[code[u] - Q_X0], 1u);
    }
  }
  // this workgroup owns its senders' counters for the launch (long runs: k_rest, later)
  for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock)
    if (dec[i]) p.pend[h.k0 + i] -= dec[i];
  if (nX) sm.flag = 1;
  __syncthreads();  // group counts complete
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int g = 0; g < 8; ++g) { const uint32_t v = gcnt[g]; gcnt[8 + g] = run; run += v; }
    gcnt[16] = run;
    run = 0;
    if (sm.flag)
      for (uint32_t k = 0; k < p.geo.S; ++k) { xoff[k] = run; run += xcnt[k]; }
    gcnt[17] = run;
  }
  __syncthreads();
  uint32_t tD = gcnt[16], tL = 0, bL = 0;
  const uint32_t tX = gcnt[17];
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    const uint32_t c = sm.part[kBlock / 64 + w];
    bL += w < wave ? c : 0u;
    tL += c;
  }
  const uint32_t sub = ((blockIdx.x & 7u) << 3) | ((blockIdx.x >> 3) & 7u);
  __syncthreads();  // every thread has read the scan partials in sm.part (and k1 for the last time)
  if (threadIdx.x == 0) {
    sm.part[0] = tD ? atomicAdd(Q.qc + (((uint32_t)Q_D * kNSub + sub) << 5), tD) : 0u;
    sm.part[1] = tL ? atomicAdd(Q.qc + (((uint32_t)Q_L * kNSub + sub) << 5), tL) : 0u;
  }
  // a peer's run goes into this workgroup's slice; what does not fit there goes on into the next
  // slice (xb1: its base there), so a slice that fills up early (few producers, uneven traffic)
  // costs no capacity the block still has
  __shared__ uint32_t xb1[kMaxShards];
  const uint32_t xg = Q.xslice(), xg1 = (xg + 1u) & (Q.xg - 1u);
  if (sm.flag && threadIdx.x >= 64 && threadIdx.x < 64 + p.geo.S) {  // another wave: in parallel
    const uint32_t pr = threadIdx.x - 64, c = xcnt[pr];
    uint32_t b0 = 0, fit = 0, b1 = 0;
    if (c) {
      b0 = atomicAdd(Q.xctr(pr, xg), c);
      fit = b0 < Q.xcs ? min(c, Q.xcs - b0) : 0u;
      if (fit < c) b1 = Q.xg > 1u ? atomicAdd(Q.xctr(pr, xg1), c - fit) : Q.xcs;  // one slice: no room
    }
    xbase[pr] = b0;
    xcnt[pr] = fit;
    xb1[pr] = b1;
  }
  // the routed copies pass through LDS in append order (the D run, the L run, then the X runs peer
  // by peer), kStageN per round, so that every wave store covers consecutive records: whole lines,
  // no reliance on L2 merging partial writes
  uint4* st = reinterpret_cast<uint4*>(sm.k1);
  const uint32_t tDL = tD + tL, nst = tDL + tX;
  for (uint32_t r0 = 0; r0 < nst; r0 += kStageN) {
    uint32_t cL = tD + bL;
#pragma unroll
    for (int u = 0; u < kIPT; ++u) {
      const uint32_t qD = gcnt[8 + (rkD[u] >> 24)] + (rkD[u] & 0xFFFFFFu);
      const uint32_t qL = cL + mask_rank(mL[u]);
      cL += (uint32_t)__popcll(mL[u]);
      if (code[u] < 0) continue;
      const uint32_t q = code[u] == Q_D ? qD : (code[u] == Q_L ? qL : tDL + xoff[code[u] - Q_X0] + rkD[u]);
      if (q < r0 || q >= r0 + kStageN) continue;
      const uint32_t i = q - r0;
      st[2 * i] = make_uint4((uint32_t)rec[u].t, (uint32_t)((uint64_t)rec[u].t >> 32), rec[u].src, rec[u].dst);
      st[2 * i + 1] = make_uint4(rec[u].seq, rec[u].size, rec[u].meta, rec[u].corrupt_off);
    }
    __syncthreads();
    const uint32_t n = min(kStageN, nst - r0);
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      const uint32_t q = r0 + i;
      const uint4 a = st[2 * i], b = st[2 * i + 1];
      if (q >= tDL) {  // a cross-shard copy: its peer's run (S is small: a linear search)
        const uint32_t x = q - tDL;
        uint32_t pr = 0;
        while (pr + 1 < p.geo.S && xoff[pr + 1] <= x) ++pr;
        const uint32_t xi = x - xoff[pr], fit = xcnt[pr];
        uint32_t pos = xi < fit ? xbase[pr] + xi : xb1[pr] + (xi - fit);
        uint32_t g = xi < fit ? xg : xg1;
        // both slices full (a skewed window): each remaining copy takes one slot in the peer's
        // other slices by an atomic of its own (rare), so the per-peer bound is the whole block
        for (uint32_t k = 2; pos >= Q.xcs && k < Q.xg; ++k) {
          g = (xg + k) & (Q.xg - 1u);
          pos = atomicAdd(Q.xctr(pr, g), 1u);
        }
        if (pos < Q.xcs) {
          uint4* dst = reinterpret_cast<uint4*>(Q.xslot(pr, g) + pos);
          st4(dst, a.x, a.y, a.z, a.w);
          st4(dst + 1, b.x, b.y, b.z, b.w);
        } else {
          atomicOr(&Q.sc->err, ERR_CAP_X);
        }
        continue;
      }
      const bool isD = q < tD;
      const uint32_t pos = isD ? sm.part[0] + q : sm.part[1] + (q - tD);
      if (pos < Q.subcap) {
        // the key from the staged words, the two bases by value select from the pinned pointers:
        // three stores with no load (and no wait) among them. (Q.K[isD ? ...] and isD ? Q.D : Q.L
        // compiled to vector loads from the kernel arguments at a lane-varying offset, key_of to a
        // load of base_slot and a 64-bit division: two full waits of the wave's stores per record)
        const size_t at = (size_t)sub * Q.subcap + pos;
        const uint32_t key = isD ? a.w - Q.lo
                                 : slot_key(Q.sdiv, (int64_t)(((uint64_t)a.y << 32) | a.x), base_slot, Q.slots);
        uint4* dst = reinterpret_cast<uint4*>((isD ? outD : outL) + at);
        st4(dst, a.x, a.y, a.z, a.w);
        st4(dst + 1, b.x, b.y, b.z, b.w);
        stn((isD ? keyD : keyL) + at, key);
      } else {
        atomicOr(&Q.sc->err, isD ? ERR_CAP_D : ERR_CAP_L);
      }
    }
    __syncthreads();
  }
  TG_PH_END(0, h.nb);
}

struct EmitKey {
  __device__ __forceinline__ void operator()(const tgsim_record& r, uint32_t idx, uint64_t& k1, uint64_t& k2,
                                             uint32_t& k3) const {
    k1 = (uint64_t)r.t;                                          // delivery time
    k2 = ((uint64_t)r.src << 32) | r.seq;                        // src, seq
    k3 = (((r.meta & TGSIM_F_CLONE) ? 0u : 1u) << 31) | idx;     // clone first
  }
};

__global__ __launch_bounds__(kBlock) void k_emit_bucket(EmitPolicy p, BktSrc src, const uint32_t* poff,
                                                        const uint2* kv, uint32_t* kscr,
                                                        uint32_t* vscr, uint32_t* kout, uint32_t* vout, BktDiv bd,
                                                        uint32_t B, uint32_t K, uint32_t* off, uint32_t* off2,
                                                        uint32_t* medium, LargeSeg* large, DevScalars* sc,
                                                        BktSrc srcL, const uint32_t* hist, uint32_t* histx,
                                                        uint32_t* tot, uint32_t slots) {
  // blocks [B, B + slots): the wheel insert's per-slot scans of the L histogram (k_local_hist made it;
  // nothing here reads it), one slot each - they share this launch instead of a dependent one
  if (blockIdx.x >= B) {
    radix_rows_body(srcL, hist, histx, tot, slots, blockIdx.x - B, slots);
    return;
  }
  __shared__ BktFusedSmem sm;
  BktHead h;
  tgsim_record rec[kIPT];
  uint32_t slot[kIPT];
  if (!bkt_fused_load<false>(src, poff, kv, kscr, vscr, kout, vout, bd, B, K, off, off2, medium, large, sc,
                             sm, h, p.D, EmitKey{}, rec, slot))
    return;
  for (uint32_t i = threadIdx.x; i < h.nk; i += kBlock) {  // inbox offsets of the bucket's receivers
    const uint32_t o = h.start + (i ? sm.cnt[i - 1] : 0u);
    off[h.k0 + i] = o;
    off2[h.k0 + i] = o;
  }
  if (h.b == B - 1 && threadIdx.x == 0) { off[K] = h.start + h.nb; off2[K] = h.start + h.nb; }
  TG_PH(7);
  // the deliveries pass through LDS in inbox order (SoA, kStageN per round) and leave with
  // coalesced stores: every wave store covers 64 consecutive entries of one output array. Entries
  // of long keys hold stale LDS here; k_rest rewrites them after this kernel.
  int64_t* st_t = reinterpret_cast<int64_t*>(sm.k1);
  uint32_t* st_u = reinterpret_cast<uint32_t*>(sm.k1) + 2 * kStageN;
  for (uint32_t r0 = 0; r0 < h.nb; r0 += kStageN) {
#pragma unroll
    for (int u = 0; u < kIPT; ++u) {
      if (slot[u] == 0xFFFFFFFFu || run_len(sm, slot[u]) > kBktRankMax) continue;
      const uint32_t o = sm.ord[slot[u]];
      if (o < r0 || o >= r0 + kStageN) continue;
      const uint32_t i = o - r0;
      const tgsim_record& r = rec[u];
#ifndef TG_EXP_NO_EMIT_DEC
      if ((r.meta & TGSIM_F_WHEEL) && r.src - p.lo < p.nloc) atomicSub(&p.pend[r.src - p.lo], 1u);
#endif
      st_t[i] = r.t;
      st_u[i] = r.src; st_u[kStageN + i] = r.dst; st_u[2 * kStageN + i] = r.seq; st_u[3 * kStageN + i] = r.size;
      st_u[4 * kStageN + i] = r.meta & ~(uint32_t)(TGSIM_F_STAGE_D | TGSIM_F_WHEEL); st_u[5 * kStageN + i] = r.corrupt_off;
    }
    __syncthreads();
    const uint32_t n = min(kStageN, h.nb - r0);
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      const uint32_t o = h.start + r0 + i;
      stn(p.o_t + o, st_t[i]); stn(p.o_src + o, st_u[i]); stn(p.o_dst + o, st_u[kStageN + i]);
      stn(p.o_seq + o, st_u[2 * kStageN + i]); stn(p.o_size + o, st_u[3 * kStageN + i]);
      stn(p.o_flags + o, st_u[4 * kStageN + i]); stn(p.o_coff + o, st_u[5 * kStageN + i]);
    }
    __syncthreads();
  }
  TG_PH_END(1, h.nb);
}

// ============================================================================================
// (4) sync service
// ============================================================================================

struct SigPolicy {
  const uint32_t* inst;
  const int64_t* t;
  const uint32_t* count;
  uint32_t* seq_out;
  int64_t* log;
  uint64_t log_base;
  uint32_t kmin;

  __device__ __forceinline__ void key(uint32_t seg, uint32_t idx, uint32_t& sg, uint64_t& k1, uint64_t& k2,
                                      uint32_t& k3) const {
    sg = seg;
    k1 = (uint64_t)t[idx];
    k2 = inst[idx];
    k3 = idx;
  }
  __device__ __forceinline__ void write(uint32_t seg, uint32_t gpos, uint32_t seg_start, uint64_t k1,
                                        uint32_t idx) const {
    seq_out[idx] = count[kmin + seg] + (gpos - seg_start) + 1u;
    log[log_base + gpos] = (int64_t)k1;
  }
  __device__ void epilogue(SortSmem& s, uint32_t m, uint32_t s_begin, const uint32_t* off, uint32_t) const {
    for (uint32_t j = threadIdx.x; j < m; j += kBlock) {
      const uint32_t e = s.perm[j];
      write(s.sg[j], s_begin + j, off[s.sg[j]], s.k1[e], s.k3[e]);
    }
  }
};

// The deferred messages' sub-lists joined into one (key = local sender, value = message index);
// their total goes to *n_out (the group-by's count). sharded 0: one list, *n_out already its count.
__global__ __launch_bounds__(kBlock) void k_keys_corr(const uint32_t* idx, uint32_t sharded, const uint32_t* qc,
                                                      const uint32_t* n_dev, uint32_t n_cap, const uint32_t* src,
                                                      uint32_t* n_out,
                                                      uint32_t lo, uint32_t* keys, uint32_t* vals,
                                                      unsigned long long* kc_deferred, uint32_t* seq_left,
                                                      uint32_t seq_left0) {
  __shared__ uint32_t pre[kDeferSub + 1];
  const uint32_t seg = defer_seg_cap(n_dev ? min(*n_dev, n_cap) : n_cap);  // as the shape pass sized it
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int s = 0; s < kDeferSub; ++s) {
      pre[s] = run;
      run += sharded ? min(qc[(uint32_t)(kQcDefer + s) << 5], seg) : (s == 0 ? *n_out : 0u);
    }
    pre[kDeferSub] = run;
  }
  __syncthreads();
  const uint32_t n = pre[kDeferSub];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (sharded) *n_out = n;
    atomicAdd(kc_deferred, (unsigned long long)n);
    *seq_left = seq_left0;  // k_shape_seq_wide counts up from here (a memset would be a launch of its own)
  }
  // sharded: block b walks sub-list b % kDeferSub (gridDim a multiple of it), contiguous reads
  const uint32_t S = sharded ? (uint32_t)kDeferSub : 1u, s = blockIdx.x % S, nb = gridDim.x / S;
  const uint32_t cnt = pre[s + 1] - pre[s], out = pre[s];
  const uint32_t* in = idx + (size_t)s * seg;
  for (uint32_t j = blockIdx.x / S * blockDim.x + threadIdx.x; j < cnt; j += nb * blockDim.x) {
    const uint32_t i = in[j];
    keys[out + j] = src[i] - lo;
    vals[out + j] = i;
  }
}

struct CorrPolicy {
  const int64_t* t;
  const uint32_t* seq;
  uint32_t* sorted;

  __device__ __forceinline__ void key(uint32_t seg, uint32_t idx, uint32_t& sg, uint64_t& k1, uint64_t& k2,
                                      uint32_t& k3) const {
    sg = seg;
    k1 = (uint64_t)t[idx] ^ 0x8000000000000000ull;  // signed order (t_send >= 0 anyway)
    k2 = seq[idx];
    k3 = idx;
  }
  __device__ __forceinline__ void write(uint32_t, uint32_t gpos, uint32_t, uint64_t, uint32_t idx) const {
    sorted[gpos] = idx;
  }
  __device__ void epilogue(SortSmem& s, uint32_t m, uint32_t s_begin, const uint32_t* off, uint32_t) const {
    for (uint32_t j = threadIdx.x; j < m; j += kBlock) {
      const uint32_t e = s.perm[j];
      write(s.sg[j], s_begin + j, off[s.sg[j]], s.k1[e], s.k3[e]);
    }
  }
};

// ---- sequential netem per sender: correlated draws and the queue limit ------------------------
// A sender whose shape uses a correlated draw (get_crandom [EXT]), or whose queue may reach netem's
// limit this window (Heavy), is decided in the order its messages reach its qdisc,
// (t_send, seq). k_shape defers those messages; they are grouped by sender and ordered (k_seg_small
// / k_rest with CorrPolicy); the extraction copied the heavy senders' due wheel records to H (grouped
// by the bucketed group-by). One wave per sender (k_shape_seq): the lanes load a chunk of 64
// messages and their Philox words in parallel, lane 0 walks the chunk in order - correlated state,
// then the limit - and the lanes write the statuses and append the queued copies. The queue is
// tracked as in the oracle: copies whose departure is known in this window (min-heap K), queued
// copies still waiting for the token bucket (min-heap U on (netem time, seq, clone first), run
// through the HTB GCRA as enqueue times pass them - the recurrence and order of k_tb_bucket), and
// a count of copies that stay queued past the window. Senders that are not heavy skip the tracking:
// their queue cannot reach the limit.

constexpr int kSeqCap = 1024;   // copies tracked per heavy sender: >= TGSIM_NETEM_LIMIT (queue never exceeds it)
constexpr int kSeqChunk = 64;   // messages per chunk, one per lane
static_assert(kSeqCap >= (int)TGSIM_NETEM_LIMIT, "a heavy sender's queue fits the LDS heaps");

struct SeqSmem {
  int64_t ue[kSeqCap];      // U: netem time
  uint64_t uk[kSeqCap];     // U: seq << 1 | !clone (clone first)
  uint32_t us[kSeqCap];     // U: size
  int64_t kd[kSeqCap];      // K: departure time
  int64_t mt[kSeqChunk];
  uint32_t midx[kSeqChunk], mdst[kSeqChunk], mseq[kSeqChunk], msize[kSeqChunk];
  uint32_t w0[2][kSeqChunk][4];  // block-0 Philox words: [0] original, [1] clone
  uint32_t w1[2][kSeqChunk][3];  // block-1 (corrupt) words
  int64_t ct[2][kSeqChunk];      // queued copy: netem time
  uint32_t cm[2][kSeqChunk];     // queued copy: meta (flags, corrupt bit)
  uint32_t co[2][kSeqChunk];     // queued copy: corrupt offset
  uint8_t st[kSeqChunk], adm[kSeqChunk];  // status, queued copies (bit c = copy c)
  uint32_t nu, nk;
  // parallel form: the chunk's admitted copies that outlive it, sorted; K lives in ue / kd (two
  // ascending buffers)
  int64_t cb[2 * kSeqChunk];
};

__device__ __forceinline__ bool u_less(const SeqSmem& m, uint32_t a, uint32_t b) {
  return m.ue[a] != m.ue[b] ? m.ue[a] < m.ue[b] : m.uk[a] < m.uk[b];
}
__device__ __forceinline__ void u_swap(SeqSmem& m, uint32_t a, uint32_t b) {
  const int64_t e = m.ue[a]; m.ue[a] = m.ue[b]; m.ue[b] = e;
  const uint64_t k = m.uk[a]; m.uk[a] = m.uk[b]; m.uk[b] = k;
  const uint32_t s = m.us[a]; m.us[a] = m.us[b]; m.us[b] = s;
}
__device__ void u_down(SeqSmem& m, uint32_t i, uint32_t n) {
  for (;;) {
    const uint32_t l = 2 * i + 1, r = l + 1;
    uint32_t s = i;
    if (l < n && u_less(m, l, s)) s = l;
    if (r < n && u_less(m, r, s)) s = r;
    if (s == i) return;
    u_swap(m, i, s);
    i = s;
  }
}
__device__ void u_push(SeqSmem& m, int64_t e, uint64_t k, uint32_t size, DevScalars* sc) {
  if (m.nu >= (uint32_t)kSeqCap) { atomicOr(&sc->err, ERR_QUEUE_CAP); return; }
  uint32_t i = m.nu++;
  m.ue[i] = e; m.uk[i] = k; m.us[i] = size;
  while (i) {
    const uint32_t p = (i - 1) / 2;
    if (!u_less(m, i, p)) break;
    u_swap(m, i, p);
    i = p;
  }
}
__device__ void k_down(SeqSmem& m, uint32_t i, uint32_t n) {
  for (;;) {
    const uint32_t l = 2 * i + 1, r = l + 1;
    uint32_t s = i;
    if (l < n && m.kd[l] < m.kd[s]) s = l;
    if (r < n && m.kd[r] < m.kd[s]) s = r;
    if (s == i) return;
    const int64_t t = m.kd[i]; m.kd[i] = m.kd[s]; m.kd[s] = t;
    i = s;
  }
}
__device__ void k_push(SeqSmem& m, int64_t d, DevScalars* sc) {
  if (m.nk >= (uint32_t)kSeqCap) { atomicOr(&sc->err, ERR_QUEUE_CAP); return; }
  uint32_t i = m.nk++;
  m.kd[i] = d;
  while (i) {
    const uint32_t p = (i - 1) / 2;
    if (m.kd[p] <= m.kd[i]) break;
    const int64_t t = m.kd[p]; m.kd[p] = m.kd[i]; m.kd[i] = t;
    i = p;
  }
}

// ---- the parallel form for queue-heavy senders without HTB or correlation ----------------------
// Without a token bucket a copy departs at its netem time, and without correlation every draw is a
// pure function of the message: only the limit couples a sender's copies. Copy q enqueued at t_q is
// admitted iff far + #{queued departures > t_q} < limit, the queued departures being the sorted
// array K (due wheel records, earlier chunks' copies) plus this chunk's admitted copies before q.
// Per chunk (64 messages, up to 128 copies, clone first) every lane computes its copies and their
// base = far + |K > t| by bisection; if the count with every earlier copy admitted stays below the
// limit nothing is dropped; otherwise one wave-uniform pass decides the copies in order, counting
// the earlier admitted ones with ballots. The chunk's admitted copies that outlive its last enqueue
// are then merged into K (bitonic sort + merge path). Same decisions as the heaps below, in
// parallel (the all-to-all and splitbrain senders took lane 0's serial walk).

// first index in [lo, hi) of the ascending k whose value is > t
__device__ __forceinline__ uint32_t upper_idx(const int64_t* k, uint32_t lo, uint32_t hi, int64_t t) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] <= t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ascending bitonic sort of v[0..n) (n a power of two) by the block's one wave
__device__ void wave_bitonic(int64_t* v, uint32_t n) {
  for (uint32_t k = 2; k <= n; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < n; i += kSeqChunk) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const int64_t x = v[i], y = v[p];
          if ((x > y) == ((i & k) == 0)) { v[i] = y; v[p] = x; }
        }
      }
      __syncthreads();
    }
}

// out[0..a+b) = merge of the ascending A[0..a) and B[0..b), merge path split per lane
__device__ void wave_merge(const int64_t* A, uint32_t a, const int64_t* B, uint32_t b, int64_t* out) {
  const uint32_t T = a + b, per = (T + kSeqChunk - 1) / kSeqChunk;
  const uint32_t d = min(T, threadIdx.x * per), e = min(T, d + per);
  uint32_t lo = d > b ? d - b : 0u, hi = min(d, a);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - mid - 1]) lo = mid + 1; else hi = mid;
  }
  uint32_t i = lo, j = d - lo;
  for (uint32_t o = d; o < e; ++o) out[o] = (j >= b || (i < a && A[i] <= B[j])) ? A[i++] : B[j++];
  __syncthreads();
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o);
  return v;
}

#ifdef TGSIM_PHASE_PROF
// debug builds: per sender (first 1024 blocks' last sender) the cycles of k_shape_seq's phases:
// [0] K setup, [1] chunk loads + Philox, [2] decisions, [3] queue after the chunk, [4] appends, [5] chunks
__device__ uint64_t g_seq_ph[1024][8];
#define SQ_T0() uint64_t sq_t = clock64(); uint64_t sq_acc[6] = {0, 0, 0, 0, 0, 0}
#define SQ_PH(k) do { const uint64_t n_ = clock64(); sq_acc[k] += n_ - sq_t; sq_t = n_; } while (0)
#define SQ_END() do { if (lane == 0 && blockIdx.x < 1024) for (int k_ = 0; k_ < 6; ++k_) g_seq_ph[blockIdx.x][k_] = sq_acc[k_]; } while (0)
#else
#define SQ_T0() do {} while (0)
#define SQ_PH(k) do {} while (0)
#define SQ_END() do {} while (0)
#endif

__global__ __launch_bounds__(kSeqChunk) void k_shape_seq(ShapeArgs a, const uint32_t* sorted, const uint32_t* moff,
                                                         const uint32_t* hoff, const uint32_t* hidx,
                                                         const tgsim_record* H, const uint32_t* rho4,
                                                         uint32_t* last4, const int64_t* Xs, const uint8_t* done) {
  __shared__ SeqSmem m;
  DevScalars* sc = a.Q.sc;
  if (sc->seq_left == 0) return;  // k_shape_seq_wide decided every sender (block-uniform)
  const int64_t t_end = sc->t_end;
  const uint32_t lane = threadIdx.x;
  for (uint32_t l = blockIdx.x; l < a.nloc; l += gridDim.x) {  // block-uniform
    const uint32_t j0 = moff[l], j1 = moff[l + 1];
    if (j0 == j1 || done[l]) continue;  // k_shape_seq_wide decided the sender's window
    const ShapeDev sh = a.shape[l];
    const bool corr = (sh.flags & kShCorr) != 0;
    const bool heavy = a.heavy.of(l);
    const bool limited = (sh.flags & kShLimited) != 0;
    const uint32_t src = a.lo + l;
    uint32_t rho[3] = {0, 0, 0}, cl[3] = {0, 0, 0};
    if (corr) {
      rho[0] = rho4[4 * l]; rho[1] = rho4[4 * l + 1]; rho[2] = rho4[4 * l + 2];
      cl[0] = last4[4 * l]; cl[1] = last4[4 * l + 1]; cl[2] = last4[4 * l + 2];
    }
    int64_t X = Xs[l];
    uint64_t far = 0;  // queued copies not leaving in this window
    SQ_T0();
    if (lane == 0) { m.nu = 0; m.nk = 0; }
    __syncthreads();
    // the parallel form: heavy, no HTB, no correlation, and every due record's departure known
    bool fast = heavy && !corr && !limited;
    uint32_t kcur = 0, kh = 0, ksz = 0;  // K: ascending in m.ue (kcur 0) or m.kd (kcur 1), [kh, ksz) live
    if (fast) {
      // one pass over the due records: their departures into K (padded to a power of two) and whether
      // any is a stage-A record (queued under an earlier, limited shape: heaps). Four records per lane
      // in flight: a dependent index -> record chain per 64 records took ~2 us each.
      const uint32_t h0 = hoff[l], h1 = hoff[l + 1];
      uint32_t n0 = h1 - h0;
      if (n0 > (uint32_t)kSeqCap) {
        if (lane == 0) atomicOr(&sc->err, ERR_QUEUE_CAP);
        n0 = kSeqCap;
      }
      const uint32_t np2 = n0 > 1 ? next_pow2(n0) : 1u;
      bool anyA = false;
      for (uint32_t j0 = 0; j0 < np2; j0 += 4 * kSeqChunk) {
        uint32_t ix[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t j = j0 + u * kSeqChunk + lane;
          ix[u] = j < n0 ? hidx[h0 + j] : 0u;
        }
        uint4 ra[4], rb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t j = j0 + u * kSeqChunk + lane;
          if (j < n0) {
            ra[u] = reinterpret_cast<const uint4*>(H + ix[u])[0];
            rb[u] = reinterpret_cast<const uint4*>(H + ix[u])[1];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t j = j0 + u * kSeqChunk + lane;
          if (j < n0) {
            m.ue[j] = (int64_t)(((uint64_t)ra[u].y << 32) | ra[u].x);
            anyA |= !(rb[u].z & TGSIM_F_STAGE_D);
          } else if (j < np2) {
            m.ue[j] = INT64_MAX;
          }
        }
      }
      fast = __ballot(anyA) == 0;
      __syncthreads();
      if (fast) {
        if (np2 > 1) wave_bitonic(m.ue, np2);
        ksz = n0;
        const uint32_t p = a.heavy.pend[l];
        far = p > h1 - h0 ? p - (h1 - h0) : 0;
      }
    }
    if (heavy && !fast) {  // the sender's due wheel records: U (token bucket pending) or K (departing now)
      const uint32_t h0 = hoff[l], h1 = hoff[l + 1];
      for (uint32_t b = h0; b < h1; b += kSeqChunk) {
        const uint32_t j = b + lane;
        tgsim_record r;
        const bool in = j < h1;
        if (in) load_rec(H + hidx[j], r);
        const bool isA = in && !(r.meta & TGSIM_F_STAGE_D), isD = in && !isA;
        const uint64_t ma = __ballot(isA), md = __ballot(isD);
        const uint32_t pa = m.nu + mask_rank(ma), pd = m.nk + mask_rank(md);
        if (isA && pa < (uint32_t)kSeqCap) {
          m.ue[pa] = r.t; m.uk[pa] = ((uint64_t)r.seq << 1) | ((r.meta & TGSIM_F_CLONE) ? 0u : 1u); m.us[pa] = r.size;
        }
        if (isD && pd < (uint32_t)kSeqCap) m.kd[pd] = r.t;
        __syncthreads();
        if (lane == 0) {
          m.nu += (uint32_t)__popcll(ma); m.nk += (uint32_t)__popcll(md);
          if (m.nu > (uint32_t)kSeqCap || m.nk > (uint32_t)kSeqCap) {
            atomicOr(&sc->err, ERR_QUEUE_CAP);
            m.nu = min(m.nu, (uint32_t)kSeqCap); m.nk = min(m.nk, (uint32_t)kSeqCap);
          }
        }
        __syncthreads();
      }
      if (lane == 0) {  // Floyd heap construction
        for (uint32_t i = m.nu / 2; i-- > 0;) u_down(m, i, m.nu);
        for (uint32_t i = m.nk / 2; i-- > 0;) k_down(m, i, m.nk);
      }
      const uint32_t p = a.heavy.pend[l];
      far = p > h1 - h0 ? p - (h1 - h0) : 0;
    }
    const bool need_w0 = sh.dup_t || sh.loss_t || sh.reorder_t || sh.sigma;
    uint32_t n_lost = 0, n_copies = 0, n_over = 0;
    SQ_PH(0);
    for (uint32_t c0 = j0; c0 < j1; c0 += kSeqChunk) {
      const uint32_t cn = min((uint32_t)kSeqChunk, j1 - c0);
      // parallel: the chunk's messages and their Philox words
      if (lane < cn) {
        const uint32_t i = sorted[c0 + lane];
        const uint32_t seq = a.seq[i];
        m.midx[lane] = i; m.mdst[lane] = a.dst[i]; m.mseq[lane] = seq; m.msize[lane] = a.size[i]; m.mt[lane] = a.t[i];
        for (uint32_t c = 0; c < 2; ++c) {
          if (c == 1 && !sh.dup_t) break;
          uint32_t o[4] = {0, 0, 0, 0};
          if (need_w0) philox4x32_10(seq, src, c, kNetemSalt, a.key0, a.key1, o);
          m.w0[c][lane][0] = o[0]; m.w0[c][lane][1] = o[1]; m.w0[c][lane][2] = o[2]; m.w0[c][lane][3] = o[3];
          if (sh.corrupt_t) {
            philox4x32_10(seq, src, c | 2u, kNetemSalt, a.key0, a.key1, o);
            m.w1[c][lane][0] = o[0]; m.w1[c][lane][1] = o[1]; m.w1[c][lane][2] = o[2];
          }
        }
      }
      __syncthreads();
      SQ_PH(1);
      if (fast) {
        // every lane: its message's copies (clone first) with their netem times, as k_shape_seq's walk
        uint8_t st = 0, adm = 0, valid = 0;
        int64_t e2[2] = {INT64_MIN, INT64_MIN};
        uint32_t meta2[2] = {0, 0}, coff2[2] = {0, 0};
        int64_t ts = INT64_MAX, base = 0;
        if (lane < cn) {
          ts = m.mt[lane];
          const uint32_t size = m.msize[lane];
          const uint32_t* r0 = m.w0[0][lane];
          const bool dup = sh.dup_t && sh.dup_t >= r0[0];
          const bool lst = sh.loss_t && sh.loss_t >= r0[1];
          const int count = 1 + (dup ? 1 : 0) - (lst ? 1 : 0);
          if (count == 0) {
            st = TGSIM_ST_LOST;
          } else {
            st = TGSIM_ST_QUEUED;
            if (dup && lst) st |= TGSIM_ST_FLAG_DUP_CANCEL;
            if (count == 2) st |= TGSIM_ST_FLAG_DUP;
            for (int c = count == 2 ? 1 : 0; c >= 0; --c) {
              const uint32_t* w = m.w0[c][lane];
              if (c == 1 && sh.loss_t && sh.loss_t >= w[1]) { st |= TGSIM_ST_FLAG_CLONE_LOST; continue; }
              uint32_t meta = c ? TGSIM_F_CLONE : 0u, coff = 0;
              if (sh.corrupt_t) {
                const uint32_t* w1 = m.w1[c][lane];
                if (sh.corrupt_t >= w1[0] && size > 0) {
                  meta |= TGSIM_F_CORRUPT | ((w1[2] % 8u) << TGSIM_F_BIT_SHIFT);
                  coff = w1[1] % size;
                }
              }
              int64_t e;
              if (sh.reorder_t && !(sh.reorder_t < w[3])) {
                meta |= TGSIM_F_REORDERED;
                e = ts;
              } else {
                const int64_t delay = tabledist(sh.mu, sh.sigma, w[2]);
                e = ts + (delay > 0 ? delay : 0);
              }
              meta |= TGSIM_F_STAGE_D;  // unlimited: the netem time is the departure
              e2[c] = e; meta2[c] = meta; coff2[c] = coff;
              valid |= (uint8_t)(1u << c);
            }
          }
          base = (int64_t)far + (int64_t)(ksz - upper_idx(kcur ? m.kd : m.ue, kh, ksz, ts));
        }
        // every earlier copy admitted and still queued: at most q of them before copy q (enqueue order:
        // message by message, clone first), so base + q below the limit admits every copy of the chunk
        bool over = false;
        for (int c = 1; c >= 0; --c)
          if (valid & (1u << c)) over |= base + (int64_t)(2 * lane + (c ? 0u : 1u)) >= (int64_t)TGSIM_NETEM_LIMIT;
        // Closed form when every copy of the chunk outlives the chunk's last enqueue (an all-to-all
        // round: 50 ms of latency against a 1 ms send spread): then every earlier admitted copy is
        // still queued at each enqueue, so copy k (k-th valid copy in enqueue order) is admitted iff
        // A_k < lim_k = limit - base_k, A_k = copies admitted before it. base_k never grows along the
        // chunk (its enqueue times do not decrease), so with L_k = max(lim_k, 0) the recurrence is
        // A_{k+1} = min(A_k + 1, L_k), i.e. A_{k+1} = (k + 1) + min(0, min_{i <= k} (L_i - i - 1)):
        // a prefix minimum over the wave instead of a step per copy.
        int64_t emin = INT64_MAX, tmax = INT64_MIN;
        if (valid & 2u) emin = e2[1] < emin ? e2[1] : emin;
        if (valid & 1u) emin = e2[0] < emin ? e2[0] : emin;
        if (valid) tmax = ts;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const int64_t a = __shfl_xor(emin, o), b = __shfl_xor(tmax, o);
          emin = a < emin ? a : emin;
          tmax = b > tmax ? b : tmax;
        }
        const bool closed = emin > tmax;  // wave-uniform
        if (__ballot(over) == 0) {
          adm = valid;
        } else if (closed) {
          const uint32_t nv = (uint32_t)__popc((uint32_t)valid);
          uint32_t k0 = nv;  // exclusive prefix of valid copies over the lanes
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(k0, o);
            if ((int)lane >= o) k0 += y;
          }
          k0 -= nv;
          const int64_t lim = (int64_t)TGSIM_NETEM_LIMIT - base;
          const int64_t Lp = lim > 0 ? lim : 0;
          // this lane's copies in enqueue order: clone (if valid), then the original
          const int64_t x0 = Lp - (int64_t)k0 - 1, x1 = Lp - (int64_t)k0 - 2;
          int64_t lmin = nv == 0 ? INT64_MAX : (nv == 1 ? x0 : (x0 < x1 ? x0 : x1));
          int64_t incl = lmin;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(incl, o);
            if ((int)lane >= o) incl = y < incl ? y : incl;
          }
          int64_t prev = __shfl_up(incl, 1);  // prefix minimum before this lane's first copy
          if (lane == 0) prev = INT64_MAX;
          adm = 0;
          uint32_t k = k0;
          for (int c = 1; c >= 0; --c) {  // clone first
            if (!(valid & (1u << c))) continue;
            const int64_t x = Lp - (int64_t)k - 1;
            const int64_t cur = prev < x ? prev : x;
            const int64_t before = (int64_t)k + (prev < 0 ? prev : 0);
            const int64_t after = (int64_t)k + 1 + (cur < 0 ? cur : 0);
            if (after == before + 1) adm |= (uint8_t)(1u << c);
            prev = cur;
            ++k;
          }
        } else {  // decide copy by copy, in enqueue order, counting the earlier admitted ones
          // Copy q (= 2 * message + (original ? 1 : 0): clone first) is admitted iff it is valid and
          // base_q + #{admitted p < q with e_p > t_q} < limit. Every lane first builds, for its
          // message's enqueue time, the 128-bit set G of the chunk's copies with e > t (one pass over
          // the candidates in LDS); the walk is then scalar: the admitted set A in two 64-bit words,
          // per copy one AND + popcount against the owner's G (readlane) and its limit. Ballots over
          // the admitted bits cost ~230 cycles per copy (VALU -> SALU -> VALU per step).
          int64_t* ce = m.cb;  // candidates in enqueue order (the kept copies reuse it afterwards)
          ce[2 * lane] = (valid & 2u) ? e2[1] : INT64_MIN;
          ce[2 * lane + 1] = (valid & 1u) ? e2[0] : INT64_MIN;
          __syncthreads();
          uint64_t g0 = 0, g1 = 0;
#pragma unroll 8
          for (uint32_t p = 0; p < 64; ++p) {
            g0 |= (uint64_t)(ce[p] > ts ? 1u : 0u) << p;
            g1 |= (uint64_t)(ce[64 + p] > ts ? 1u : 0u) << p;
          }
          __syncthreads();  // ce is rewritten by the kept copies below
          // admission limit of the lane's copies: count < limit - base (invalid: never)
          const int64_t lim = (int64_t)TGSIM_NETEM_LIMIT - base;
          const int32_t lim32 = lim < INT32_MIN ? INT32_MIN : (lim > INT32_MAX ? INT32_MAX : (int32_t)lim);
          const int32_t lim1 = (valid & 2u) ? lim32 : INT32_MIN, lim0 = (valid & 1u) ? lim32 : INT32_MIN;
          const uint32_t g0l = (uint32_t)g0, g0h = (uint32_t)(g0 >> 32), g1l = (uint32_t)g1, g1h = (uint32_t)(g1 >> 32);
          uint64_t A0 = 0, A1 = 0;
          // only lanes with a copy the limit can still admit take a step (an all-to-all sender's queue
          // is full: ~20 % of its copies get in), in lane order, clone before original
          uint64_t cand = __ballot(lim1 > 0 || lim0 > 0);
          while (cand) {
            const int owner = __ffsll((unsigned long long)cand) - 1;
            cand &= cand - 1ull;
            const uint64_t G0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g0h, owner) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)g0l, owner);
            const uint64_t G1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g1h, owner) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)g1l, owner);
            const int32_t l1 = __builtin_amdgcn_readlane(lim1, owner), l0 = __builtin_amdgcn_readlane(lim0, owner);
#pragma unroll
            for (uint32_t o = 0; o < 2; ++o) {
              const uint32_t q = 2u * (uint32_t)owner + o;
              const int32_t lq = o ? l0 : l1;
              const uint64_t m0 = q < 64 ? ((1ull << q) - 1ull) : ~0ull;
              const uint64_t m1 = q < 64 ? 0ull : ((1ull << (q - 64)) - 1ull);
              const int32_t cnt = __popcll(A0 & G0 & m0) + __popcll(A1 & G1 & m1);
              if (cnt < lq) {
                if (q < 64) A0 |= 1ull << q; else A1 |= 1ull << (q - 64);
              }
            }
          }
          const uint32_t qc = 2 * lane, qo = 2 * lane + 1;  // this lane's clone / original
          const uint64_t Ac = qc < 64 ? A0 >> qc : A1 >> (qc - 64);
          const uint64_t Ao = qo < 64 ? A0 >> qo : A1 >> (qo - 64);
          adm = (uint8_t)(((Ac & 1u) << 1) | (Ao & 1u));
        }
        SQ_PH(2);
        if (lane < cn) {
          if (st != TGSIM_ST_LOST) {
            const uint8_t dropped = valid & ~adm;
            if (dropped & 2u) st |= TGSIM_ST_FLAG_CLONE_LOST;
            if (dropped & 1u) st |= TGSIM_ST_FLAG_OVERLIMIT;
            if (!adm) st = (uint8_t)((st & 0xF0u) | TGSIM_ST_OVERLIMIT);
            n_over += (uint32_t)__popc(dropped);
            n_copies += (uint32_t)__popc(adm);
          } else {
            ++n_lost;
          }
          m.st[lane] = st;
          m.adm[lane] = adm;
          for (int c = 0; c < 2; ++c) { m.ct[c][lane] = e2[c]; m.cm[c][lane] = meta2[c]; m.co[c][lane] = coff2[c]; }
        }
        // the queue after the chunk: departures up to its last enqueue have left; copies going past
        // the window stay counted in far; the rest join K
        const int64_t t_last = __shfl(ts, (int)cn - 1);
        uint32_t nfar = 0, nk = 0;
        for (int c = 0; c < 2; ++c) {
          const bool in = (adm >> c) & 1u;
          nfar += in && e2[c] >= t_end ? 1u : 0u;
          const bool keep = in && e2[c] < t_end && e2[c] > t_last;
          const uint64_t bk = __ballot(keep);
          if (keep) m.cb[nk + mask_rank(bk)] = e2[c];  // slots per round, filled below
          nk += (uint32_t)__popcll(bk);
        }
        far += wave_sum(nfar);
        kh = upper_idx(kcur ? m.kd : m.ue, kh, ksz, t_last);
        if (nk) {
          const uint32_t np2 = nk > 1 ? next_pow2(nk) : 1u;
          for (uint32_t j = nk + lane; j < np2; j += kSeqChunk) m.cb[j] = INT64_MAX;
          __syncthreads();
          if (np2 > 1) wave_bitonic(m.cb, np2);
          uint32_t na = ksz - kh;
          if (na + nk > (uint32_t)kSeqCap) {  // cannot happen: the queue never holds more than the limit
            if (lane == 0) atomicOr(&sc->err, ERR_QUEUE_CAP);
            na = (uint32_t)kSeqCap - nk;
          }
          wave_merge((kcur ? m.kd : m.ue) + kh, na, m.cb, nk, kcur ? m.ue : m.kd);
          kcur ^= 1u;
          kh = 0;
          ksz = na + nk;
        }
        __syncthreads();
        SQ_PH(3);
      }
      // sequential: netem_enqueue per message in qdisc order
      if (!fast && lane == 0) {
        for (uint32_t k = 0; k < cn; ++k) {
          const int64_t ts = m.mt[k];
          const uint32_t size = m.msize[k];
          if (heavy) {
            while (m.nu && m.ue[0] < ts) {  // departures up to ts: HTB GCRA in k_tb_bucket's order
              const int64_t e = m.ue[0];
              const uint32_t usz = m.us[0];
              --m.nu;
              if (m.nu) { m.ue[0] = m.ue[m.nu]; m.uk[0] = m.uk[m.nu]; m.us[0] = m.us[m.nu]; u_down(m, 0, m.nu); }
              const int64_t dd = e > X ? e : X;
              const int64_t b0 = X > e - sh.tau ? X : e - sh.tau;
              const int64_t v = b0 + (int64_t)l2t_ns(sh, usz);
              X = v > kTbClamp ? kTbClamp : v;
              k_push(m, dd, sc);
            }
            while (m.nk && m.kd[0] <= ts) {  // a copy leaving at ts has left (occupancy [enqueue, d))
              --m.nk;
              if (m.nk) { m.kd[0] = m.kd[m.nk]; k_down(m, 0, m.nk); }
            }
          }
          const uint32_t* r0 = m.w0[0][k];
          const bool dup = sh.dup_t && sh.dup_t >= crandom(cl[0], rho[0], r0[0]);
          const bool lst = sh.loss_t && sh.loss_t >= r0[1];
          const int count = 1 + (dup ? 1 : 0) - (lst ? 1 : 0);
          uint8_t st;
          uint8_t adm = 0;
          if (count == 0) {
            st = TGSIM_ST_LOST;
            ++n_lost;
          } else {
            st = TGSIM_ST_QUEUED;
            if (dup && lst) st |= TGSIM_ST_FLAG_DUP_CANCEL;
            for (int c = count == 2 ? 1 : 0; c >= 0; --c) {  // the clone is enqueued first
              const uint32_t* w = m.w0[c][k];
              if (c == 1 && sh.loss_t && sh.loss_t >= w[1]) { st |= TGSIM_ST_FLAG_CLONE_LOST; continue; }
              uint32_t meta = c ? TGSIM_F_CLONE : 0u, coff = 0;
              if (sh.corrupt_t) {
                const uint32_t* w1 = m.w1[c][k];
                if (sh.corrupt_t >= crandom(cl[1], rho[1], w1[0]) && size > 0) {
                  meta |= TGSIM_F_CORRUPT | ((w1[2] % 8u) << TGSIM_F_BIT_SHIFT);
                  coff = w1[1] % size;
                }
              }
              if (heavy && far + m.nu + m.nk >= TGSIM_NETEM_LIMIT) {  // sch->q.qlen >= sch->limit
                ++n_over;
                st |= c ? TGSIM_ST_FLAG_CLONE_LOST : TGSIM_ST_FLAG_OVERLIMIT;
                continue;
              }
              int64_t e;
              if (sh.reorder_t && !(sh.reorder_t < crandom(cl[2], rho[2], w[3]))) {
                meta |= TGSIM_F_REORDERED;
                e = ts;
              } else {
                const int64_t delay = tabledist(sh.mu, sh.sigma, w[2]);
                e = ts + (delay > 0 ? delay : 0);
              }
              if (!limited) meta |= TGSIM_F_STAGE_D;
              m.ct[c][k] = e; m.cm[c][k] = meta; m.co[c][k] = coff;
              adm |= (uint8_t)(1u << c);
              ++n_copies;
              if (heavy) {
                if (e >= t_end) ++far;
                else if (limited) u_push(m, e, ((uint64_t)m.mseq[k] << 1) | (c ? 0u : 1u), size, sc);
                else k_push(m, e, sc);
              }
            }
            if (count == 2) st |= TGSIM_ST_FLAG_DUP;
            if (!adm) st = (uint8_t)((st & 0xF0u) | TGSIM_ST_OVERLIMIT);
          }
          m.st[k] = st;
          m.adm[k] = adm;
        }
      }
      __syncthreads();
      // parallel: statuses and the queued copies
      tgsim_record r1, r2;
      int q1 = -1, q2 = -1;
      if (lane < cn) {
        a.status[m.midx[lane]] = m.st[lane];
        const uint8_t adm = m.adm[lane];
        for (int c = 1; c >= 0; --c) {
          if (!(adm & (1u << c))) continue;
          tgsim_record& r = c ? r1 : r2;
          r.t = m.ct[c][lane]; r.src = src; r.dst = m.mdst[lane]; r.seq = m.mseq[lane]; r.size = m.msize[lane];
          r.meta = m.cm[c][lane]; r.corrupt_off = m.co[c][lane];
          (c ? q1 : q2) = qid_copy(a.geo, r, t_end);
        }
      }
      const int qs[2] = {q1, q2};
      const tgsim_record rs[2] = {r1, r2};
      // chunk k of sender l: sub-queue (l + k) % 64, so one sender's appends spread over all of them
      a.Q.push_batch<2>(qs, rs, l + (c0 - j0) / kSeqChunk, true);
      __syncthreads();
      SQ_PH(4);
#ifdef TGSIM_PHASE_PROF
      sq_acc[5]++;
#endif
    }
    SQ_END();
    n_lost = wave_sum(n_lost);  // the walk counts in lane 0, the parallel form in every lane
    n_copies = wave_sum(n_copies);
    n_over = wave_sum(n_over);
    if (lane == 0) {
      if (corr) { last4[4 * l] = cl[0]; last4[4 * l + 1] = cl[1]; last4[4 * l + 2] = cl[2]; }
      unsigned long long* row = a.stats + (size_t)(l & (kNSub - 1)) * 16;
      if (n_lost) atomicAdd(&row[ST_LOST], (unsigned long long)n_lost);
      if (n_copies) atomicAdd(&row[ST_COPIES], (unsigned long long)n_copies);
      if (n_over) atomicAdd(&row[ST_OVERLIMIT], (unsigned long long)n_over);
    }
    __syncthreads();
  }
}

// ---- the whole-sender closed form -----------------------------------------
// The parallel form above walks a sender's window chunk by chunk in one wave: the admission test of
// chunk c needs the queue the earlier chunks left. When every copy the sender enqueues in the window
// outlives its last enqueue (min netem time > max send time: an all-to-all round's 50 ms of latency
// against a 1 ms send spread), every earlier admitted copy is still queued at each enqueue, so copy
// k is admitted iff A_k < L_k with A_k the copies admitted before it and L_k = limit - far -
// |K > t_k| (K: the due wheel records' departures), and A_{k+1} = min(A_k + 1, max(L_k, 0)) has the
// closed form A_k = k + min(0, min_{i<k} (L_i - i - 1)) (L never decreases along the window). One
// 1024-thread workgroup per sender evaluates it for the whole window at once: one message per
// thread, two block scans. A sender it cannot take (correlated, shaped, a due stage-A record, more
// than 1024 messages or due records, or the condition fails) is left to k_shape_seq (done[l] = 0).
constexpr int kWide = 1024;
constexpr int kWideWaves = kWide / 64;

__device__ __forceinline__ uint32_t wide_excl_scan(uint32_t v, uint32_t* red, uint32_t& total) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if ((int)lane >= o) x += y;
  }
  if (lane == 63) red[wave] = x;
  __syncthreads();
  uint32_t pre = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWideWaves; ++w) {
    const uint32_t a = red[w];
    pre += w < (int)wave ? a : 0u;
    total += a;
  }
  __syncthreads();
  return pre + x - v;
}
// exclusive prefix minimum over the block's threads (INT64_MAX for thread 0)
__device__ __forceinline__ int64_t wide_excl_min(int64_t v, int64_t* red) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  int64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o);
    if ((int)lane >= o) x = y < x ? y : x;
  }
  if (lane == 63) red[wave] = x;
  __syncthreads();
  int64_t pre = INT64_MAX;
#pragma unroll
  for (int w = 0; w < kWideWaves; ++w) {
    const int64_t a = red[w];
    if (w < (int)wave) pre = a < pre ? a : pre;
  }
  __syncthreads();
  int64_t ex = __shfl_up(x, 1);
  if (lane == 0) ex = INT64_MAX;
  return ex < pre ? ex : pre;
}

// Ascending sort of one 64-bit key per thread of the kWide-thread block into LDS: each wave ranks
// its 64 keys against each other (64 scalar broadcasts, no barrier), then four merge rounds of run
// pairs (64 -> 1024), each element placing itself by a binary search of the other run (A side:
// keys below; B side: keys at or below, so equal keys - the padding - keep their order). Returns
// the buffer that holds the sorted keys (a or b). A register bitonic took ~11 us per sender: its 45
// cross-lane stages are dependent ds_bpermute round trips.
static_assert(kWide == 1024, "wide_sort: four merge rounds from 64-key runs");
__device__ __forceinline__ uint64_t* wide_sort(uint64_t x, uint64_t* a, uint64_t* b) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint32_t xh = (uint32_t)(x >> 32), xl = (uint32_t)x;
  uint32_t r = 0;
#pragma unroll 8
  for (int j = 0; j < 64; ++j) {
    const uint32_t yh = (uint32_t)__builtin_amdgcn_readlane((int)xh, j), yl = (uint32_t)__builtin_amdgcn_readlane((int)xl, j);
    const uint64_t y = ((uint64_t)yh << 32) | yl;
    r += (y < x || (y == x && (uint32_t)j < lane)) ? 1u : 0u;
  }
  uint32_t pos = wave * 64u + r;
  a[pos] = x;
  uint64_t *src = a, *dst = b;
  for (uint32_t L = 64; L < (uint32_t)kWide; L <<= 1) {
    __syncthreads();
    const uint32_t base = pos & ~(2 * L - 1);
    const bool in_a = (pos & L) == 0;
    const uint64_t* other = src + base + (in_a ? L : 0u);
    uint32_t lo = 0, hi = L;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint64_t y = other[mid];
      if (in_a ? y < x : y <= x) lo = mid + 1; else hi = mid;
    }
    pos = base + (pos - base - (in_a ? 0u : L)) + lo;
    dst[pos] = x;
    uint64_t* t = src; src = dst; dst = t;
  }
  __syncthreads();
  return src;
}

// Bucket sort of one packed key per thread (key >> 42 = t_send - min, below it seq and the position,
// so keys are distinct) for send times spread over < 2^22 ns: bucket = (t_send - min) >> sh, with
// sh the least shift that leaves < 1024 buckets. One LDS atomic per key claims a slot in its bucket,
// a block scan of the bucket counts places the buckets, and each key ranks itself among its bucket
// mates (a few for send times spread evenly). Writes inv[rank] = this thread's position and raises
// *tie when two keys share (t_send, seq). Returns false (nothing written) when some bucket holds more
// than kWideBucketMax keys - clustered send times - where the merge sort above is the better form.
constexpr uint32_t kWideBucketMax = 32;
__device__ __forceinline__ bool wide_bucket_sort(uint64_t key, bool live, uint32_t sh, uint32_t* cnt, uint64_t* tmp,
                                                 uint32_t* inv, uint32_t* red, uint32_t* big, uint32_t* tie) {
  const uint32_t tid = threadIdx.x;
  const uint32_t b = live ? (uint32_t)(key >> (42 + sh)) : 0u;
  cnt[tid] = 0u;
  __syncthreads();
  const uint32_t slot = live ? atomicAdd(&cnt[b], 1u) : 0u;
  __syncthreads();
  const uint32_t c = cnt[tid];
  if (c > kWideBucketMax) *big = 1u;
  uint32_t tot;
  const uint32_t start = wide_excl_scan(c, red, tot);  // its barriers publish *big
  if (*big) return false;                             // block-uniform
  cnt[tid] = start;
  __syncthreads();
  const uint32_t s = live ? cnt[b] : 0u;
  const uint32_t e = live ? (b + 1u < (uint32_t)kWide ? cnt[b + 1] : tot) : 0u;
  if (live) tmp[s + slot] = key;
  __syncthreads();
  if (live) {
    uint32_t r = 0, t = 0;  // t: a count, not a bool (see the fast-retransmit walk, tgsim_tcp.hip)
    for (uint32_t j = s; j < e; ++j) {
      const uint64_t y = tmp[j];
      r += y < key ? 1u : 0u;
      t += (y != key && (y >> 10) == (key >> 10)) ? 1u : 0u;
    }
    __asm__ volatile("" : "+v"(t));
    inv[s + r] = tid;
    if (t) *tie = 1u;
  }
  __syncthreads();
  return true;
}

#ifdef TGSIM_PHASE_PROF
// debug builds: per block (its last sender) of the last k_shape_seq_wide launch, s_memrealtime at:
// start, sorted, K ready, copies drawn, decided, appended, end
__device__ uint64_t g_wide_ph[4096][12];
#define WIDE_PH(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_wide_ph[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WIDE_PH(k) do {} while (0)
#endif
#ifdef TG_WIDE_WPE
#define TG_WIDE_ATTR __attribute__((amdgpu_waves_per_eu(TG_WIDE_WPE)))
#else
#define TG_WIDE_ATTR
#endif
__global__ __launch_bounds__(kWide) TG_WIDE_ATTR void k_shape_seq_wide(ShapeArgs a, const uint32_t* gvals, uint32_t* sorted,  // may alias
                                                          const uint32_t* moff, const uint32_t* hoff,
                                                          const uint32_t* hidx, const tgsim_record* H,
                                                          uint8_t* done) {
  __shared__ int64_t K[kWide];                 // the due records' departures, ascending
  __shared__ uint64_t S1[kWide];               // sort keys
  __shared__ uint32_t S2[kWide], S3[kWide];    // exact sort: seq, position; then S3 = sorted -> position
  __shared__ int64_t Mt[kWide];                // the messages by position in the group-by's order
  __shared__ uint32_t Ms[kWide], Md[kWide], Mz[kWide], Mi[kWide];
  __shared__ uint32_t red[kWideWaves];
  __shared__ int64_t red64[kWideWaves], rmin[kWideWaves], rmax[kWideWaves];
  __shared__ int64_t rnmin[kWideWaves], rnmax[kWideWaves];  // the next sender's send-time range, per wave
  __shared__ uint32_t s_flag, s_stage_a, s_big, s_wtot[kWideWaves][3];
  DevScalars* sc = a.Q.sc;
  const int64_t t_end = sc->t_end;
  const uint32_t tid = threadIdx.x;
  // A block walks its senders one ahead: the next sender's loads - two dependent levels, (message
  // index, due record index), then (the message's fields, the due record) - are in flight while
  // this sender sorts and decides (the first level from the top of the iteration, the second from
  // the end of the due-record count; 3.6 us of a ~19-us sender were these loads, waited for).
  struct Meta { uint32_t j0, n, h0, n0; bool elig; };
  struct Pf { int64_t ts; uint64_t kx; uint32_t i, sq, dst, size; bool stage_a; };
  auto meta_of = [&](uint32_t l) {
    Meta m{0u, 0u, 0u, 0u, false};
    if (l >= a.nloc) return m;
    m.j0 = moff[l];
    m.n = moff[l + 1] - m.j0;
    if (m.n == 0 || m.n > (uint32_t)kWide) return m;
    const ShapeDev sh = a.shape[l];
    m.h0 = hoff ? hoff[l] : 0u;
    m.n0 = (hoff ? hoff[l + 1] : 0u) - m.h0;
    // block-uniform: the closed form needs queue tracking without HTB or correlation
    m.elig = hoff && a.heavy.of(l) && !(sh.flags & (kShCorr | kShLimited)) && m.n0 <= (uint32_t)kWide;
    return m;
  };
  auto load1 = [&](const Meta& m, uint32_t& qi, uint32_t& qhx) {
    qi = 0;
    qhx = 0;
    if (m.n > (uint32_t)kWide) return;
    if (tid < m.n) qi = gvals[m.j0 + tid];
    if (m.elig && tid < m.n0) qhx = hidx[m.h0 + tid];
  };
  auto load2 = [&](const Meta& m, uint32_t qi, uint32_t qhx, Pf& p) {
    p.ts = 0; p.kx = ~0ull; p.i = qi; p.sq = 0; p.dst = 0; p.size = 0; p.stage_a = false;
    if (m.n > (uint32_t)kWide) return;
    if (tid < m.n) { p.ts = a.t[qi]; p.sq = a.seq[qi]; p.dst = a.dst[qi]; p.size = a.size[qi]; }
    if (m.elig && tid < m.n0) {
      tgsim_record r;
      load_rec(H + qhx, r);
      p.kx = (uint64_t)r.t ^ 0x8000000000000000ull;
      p.stage_a = !(r.meta & TGSIM_F_STAGE_D);  // queued under an earlier, shaped Shape: k_shape_seq's heaps
    }
  };
  Meta nm = meta_of(blockIdx.x);
  Pf pf;
  {
    uint32_t qi, qhx;
    load1(nm, qi, qhx);
    load2(nm, qi, qhx, pf);
  }
  // true: the last sender's tail published this sender's send-time range (rnmin / rnmax) and reset
  // the flags, so the sort starts without a barrier of its own (block-uniform)
  bool mm_ready = false;
  for (uint32_t l = blockIdx.x; l < a.nloc; l += gridDim.x) {  // block-uniform
    const bool mm = mm_ready;
    mm_ready = false;
    const Meta cm = nm;
    const uint32_t j0 = cm.j0, n = cm.n, n0 = cm.n0;
    const bool elig = cm.elig;
    const uint32_t i = pf.i;
    int64_t ts = pf.ts;
    uint32_t sq = pf.sq;
    const uint32_t mdst = pf.dst, msize = pf.size;
    uint64_t kx = pf.kx;
    const bool stage_a = pf.stage_a;
    nm = meta_of(l + gridDim.x);
    uint32_t qi, qhx;
    load1(nm, qi, qhx);
    if (n == 0) { load2(nm, qi, qhx, pf); continue; }
    if (n > (uint32_t)kWide) {  // k_rest ordered it; k_shape_seq walks it
      if (tid == 0) { done[l] = 0; atomicAdd(&sc->seq_left, 1u); }
      load2(nm, qi, qhx, pf);
      continue;
    }
    WIDE_PH(0);
    const ShapeDev sh = a.shape[l];
    if (!mm && tid == 0) { s_flag = 0; s_stage_a = 0; s_big = 0; }
    if (tid < n) { Mt[tid] = ts; Ms[tid] = sq; Md[tid] = mdst; Mz[tid] = msize; Mi[tid] = i; }
#ifdef TGSIM_PHASE_PROF
    if (tid < n) Mi[tid] += (uint32_t)(kx & 0);  // the loads complete before the clock below
#endif
    WIDE_PH(7);
    // the sender's messages in (t_send, seq, index) order (k_seg_small<CorrPolicy>'s order, which
    // this kernel replaces for every sender of at most kWide = kTile of them). Packed: one 64-bit
    // key (t_send - min << 42 | seq << 10 | position) sorted mostly in registers, when the send times
    // span less than 2^22 ns and no two messages share (t_send, seq); else the exact sort over
    // (t_send, seq, index) in LDS.
    const uint32_t np2m = n > 1 ? next_pow2(n) : 1u;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    if (mm) {
#pragma unroll
      for (int w = 0; w < kWideWaves; ++w) {
        mn = rnmin[w] < mn ? rnmin[w] : mn;
        mx = rnmax[w] > mx ? rnmax[w] : mx;
      }
    } else {
      mn = tid < n ? ts : INT64_MAX;
      mx = tid < n ? ts : INT64_MIN;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int64_t x = __shfl_xor(mn, o), y = __shfl_xor(mx, o);
        mn = x < mn ? x : mn;
        mx = y > mx ? y : mx;
      }
      if (lane_id() == 0) { rmin[tid >> 6] = mn; rmax[tid >> 6] = mx; }
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kWideWaves; ++w) {
        mn = rmin[w] < mn ? rmin[w] : mn;
        mx = rmax[w] > mx ? rmax[w] : mx;
      }
    }
    if (stage_a) s_stage_a = 1u;  // read after the sort's barriers
    const bool packed = (uint64_t)(mx - mn) < (1ull << 22);  // block-uniform
    WIDE_PH(8);
    if (packed) {
      const uint64_t key = tid < n ? ((uint64_t)(ts - mn) << 42) | ((uint64_t)sq << 10) | tid : ~0ull;
      const uint32_t span = (uint32_t)(mx - mn), bits = span ? 32u - (uint32_t)__builtin_clz(span) : 0u;
      const uint32_t sh = bits > 10u ? bits - 10u : 0u;  // (span >> sh) < 1024
      if (!wide_bucket_sort(key, tid < n, sh, S2, S1, S3, red, &s_big, &s_flag)) {  // block-uniform
        const uint64_t* srt = wide_sort(key, S1, reinterpret_cast<uint64_t*>(K));
        S3[tid] = (uint32_t)(srt[tid] & 1023u);
        if (tid > 0 && tid < n && (srt[tid] >> 10) == (srt[tid - 1] >> 10)) s_flag = 1u;  // a (t_send, seq) tie
        __syncthreads();
      }
      WIDE_PH(9);
    }
    if (!packed || s_flag) {  // block-uniform
      if (tid < n) {
        S1[tid] = (uint64_t)Mt[tid] ^ 0x8000000000000000ull;
        S2[tid] = Ms[tid];
        S3[tid] = tid;
      } else if (tid < np2m) {
        S1[tid] = ~0ull; S2[tid] = ~0u; S3[tid] = ~0u;
      }
      __syncthreads();
      for (uint32_t k = 2; k <= np2m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
          if (tid < np2m) {
            const uint32_t p = tid ^ j;
            if (p > tid) {
              const uint64_t x1 = S1[tid], y1 = S1[p];
              const uint32_t x2 = S2[tid], y2 = S2[p], x3 = S3[tid], y3 = S3[p];
              const uint32_t xi = x3 < n ? Mi[x3] : ~0u, yi = y3 < n ? Mi[y3] : ~0u;
              const bool gt = x1 != y1 ? x1 > y1 : (x2 != y2 ? x2 > y2 : xi > yi);
              if (gt == ((tid & k) == 0)) {
                S1[tid] = y1; S1[p] = x1; S2[tid] = y2; S2[p] = x2; S3[tid] = y3; S3[p] = x3;
              }
            }
          }
          __syncthreads();
        }
    }
    if (tid < n) sorted[j0 + tid] = Mi[S3[tid]];
    WIDE_PH(1);
    if (!elig || s_stage_a) {  // block-uniform: k_shape_seq walks it
      if (tid == 0) { done[l] = 0; atomicAdd(&sc->seq_left, 1u); }
      load2(nm, qi, qhx, pf);
      __syncthreads();  // every thread's reads of this sender's LDS are done
      continue;
    }
    // |K > t_k| for every message k without sorting K: the messages' send times in (t_send, seq)
    // order (K's array), each due departure v counted at the first message it has not left by,
    // lb(v) = first k with t_k >= v (a copy leaving at t has left: occupancy [enqueue, departure)),
    // then #{K <= t_k} = the inclusive prefix of those counts (S2 as the histogram)
    if (tid < n) K[tid] = Mt[S3[tid]];
    S2[tid] = 0;
    __syncthreads();
    if (tid < n0) {
      const int64_t v = (int64_t)(kx ^ 0x8000000000000000ull);
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (K[mid] < v) lo = mid + 1; else hi = mid;
      }
      if (lo < n) atomicAdd(&S2[lo], 1u);
    }
    __syncthreads();
    uint32_t gone;  // #{K <= t_k} for this thread's message
    {
      uint32_t tk;
      const uint32_t h = S2[tid];
      gone = wide_excl_scan(h, red, tk) + h;
    }
    WIDE_PH(2);
    load2(nm, qi, qhx, pf);  // the next sender's second level, in flight through the decisions
    const uint32_t pnd = a.heavy.pend[l];
    const int64_t far = pnd > n0 ? (int64_t)(pnd - n0) : 0;
    // this thread's message: its copies (clone first) and netem times, as k_shape_seq's parallel form
    const uint32_t src = a.lo + l;
    uint8_t st = 0, valid = 0;
    int64_t e2[2] = {INT64_MIN, INT64_MIN};
    uint32_t meta2[2] = {0, 0}, coff2[2] = {0, 0};
    int64_t base = 0;
    ts = INT64_MIN;
    uint32_t idx = 0, dst = 0, seq = 0, size = 0;
    if (tid < n) {
      const uint32_t p = S3[tid];  // this thread's message: the tid-th in (t_send, seq) order
      idx = Mi[p]; seq = Ms[p]; dst = Md[p]; size = Mz[p]; ts = Mt[p];
      uint32_t w0[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, w1[2][3] = {{0, 0, 0}, {0, 0, 0}};
      const bool need_w0 = sh.dup_t || sh.loss_t || sh.reorder_t || sh.sigma;
#pragma unroll
      for (uint32_t c = 0; c < 2; ++c) {
        if (c == 1 && !sh.dup_t) break;
        if (need_w0) philox4x32_10(seq, src, c, kNetemSalt, a.key0, a.key1, w0[c]);
        if (sh.corrupt_t) {
          uint32_t o[4];
          philox4x32_10(seq, src, c | 2u, kNetemSalt, a.key0, a.key1, o);
          w1[c][0] = o[0]; w1[c][1] = o[1]; w1[c][2] = o[2];
        }
      }
      const bool dup = sh.dup_t && sh.dup_t >= w0[0][0];
      const bool lst = sh.loss_t && sh.loss_t >= w0[0][1];
      const int count = 1 + (dup ? 1 : 0) - (lst ? 1 : 0);
      if (count == 0) {
        st = TGSIM_ST_LOST;
      } else {
        st = TGSIM_ST_QUEUED;
        if (dup && lst) st |= TGSIM_ST_FLAG_DUP_CANCEL;
        if (count == 2) st |= TGSIM_ST_FLAG_DUP;
#pragma unroll
        for (int c = 1; c >= 0; --c) {
          if (c == 1 && count != 2) continue;
          const uint32_t* w = w0[c];
          if (c == 1 && sh.loss_t && sh.loss_t >= w[1]) { st |= TGSIM_ST_FLAG_CLONE_LOST; continue; }
          uint32_t meta = c ? TGSIM_F_CLONE : 0u, coff = 0;
          if (sh.corrupt_t && sh.corrupt_t >= w1[c][0] && size > 0) {
            meta |= TGSIM_F_CORRUPT | ((w1[c][2] % 8u) << TGSIM_F_BIT_SHIFT);
            coff = w1[c][1] % size;
          }
          int64_t e;
          if (sh.reorder_t && !(sh.reorder_t < w[3])) {
            meta |= TGSIM_F_REORDERED;
            e = ts;
          } else {
            const int64_t delay = tabledist(sh.mu, sh.sigma, w[2]);
            e = ts + (delay > 0 ? delay : 0);
          }
          meta |= TGSIM_F_STAGE_D;  // unlimited: the netem time is the departure
          e2[c] = e; meta2[c] = meta; coff2[c] = coff;
          valid |= (uint8_t)(1u << c);
        }
      }
      base = far + (int64_t)(n0 - gone);
    }
    WIDE_PH(3);
    // the closed form holds when every copy outlives the window's last enqueue
    int64_t emin = INT64_MAX, tmax = INT64_MIN;
    if (valid & 2u) emin = e2[1] < emin ? e2[1] : emin;
    if (valid & 1u) emin = e2[0] < emin ? e2[0] : emin;
    if (valid) tmax = ts;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t x = __shfl_xor(emin, o), y = __shfl_xor(tmax, o);
      emin = x < emin ? x : emin;
      tmax = y > tmax ? y : tmax;
    }
    if (lane_id() == 0) { rmin[tid >> 6] = emin; rmax[tid >> 6] = tmax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWideWaves; ++w) {
      emin = rmin[w] < emin ? rmin[w] : emin;
      tmax = rmax[w] > tmax ? rmax[w] : tmax;
    }
    if (!(emin > tmax)) {  // block-uniform: k_shape_seq walks it
      if (tid == 0) { done[l] = 0; atomicAdd(&sc->seq_left, 1u); }
      __syncthreads();
      continue;
    }
    // copy k (enqueue order: message, clone first) admitted iff A_{k+1} = A_k + 1
    // k0 = copies before this thread's (exclusive sum of nv) and prev = min over earlier copies of
    // (L - index - 1), in one barrier: with e the wave-local exclusive sum and K0 the waves before,
    // an earlier thread's term is (Lp - nv - e) - K0, so each wave publishes its sum and its minimum
    // of (Lp - nv - e), and every thread folds the earlier waves' entries
    const uint32_t nv = (uint32_t)__popc((uint32_t)valid);
    const int64_t lim = (int64_t)TGSIM_NETEM_LIMIT - base;
    const int64_t Lp = lim > 0 ? lim : 0;
    uint32_t k0;
    int64_t prev;
    {
      const uint32_t lane = lane_id(), wave = tid >> 6;
      uint32_t inc = nv;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if ((int)lane >= o) inc += y;
      }
      const uint32_t e = inc - nv;
      const int64_t g = nv ? Lp - (int64_t)nv - (int64_t)e : INT64_MAX;
      int64_t pm = g;  // inclusive prefix minimum of g in the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(pm, o);
        if ((int)lane >= o) pm = y < pm ? y : pm;
      }
      if (lane == 63) { red[wave] = inc; red64[wave] = pm; }
      int64_t ex = __shfl_up(pm, 1);
      if (lane == 0) ex = INT64_MAX;
      __syncthreads();
      uint32_t K0 = 0;
      int64_t P = INT64_MAX;
#pragma unroll
      for (int w = 0; w < kWideWaves; ++w) {
        if (w < (int)wave) {
          const int64_t G = red64[w];
          if (G != INT64_MAX && G - (int64_t)K0 < P) P = G - (int64_t)K0;
          K0 += red[w];
        }
      }
      k0 = K0 + e;
      const int64_t own = ex == INT64_MAX ? INT64_MAX : ex - (int64_t)K0;
      prev = own < P ? own : P;
    }
    uint8_t adm = 0;
    uint32_t k = k0;
#pragma unroll
    for (int c = 1; c >= 0; --c) {
      if (!(valid & (1u << c))) continue;
      const int64_t x = Lp - (int64_t)k - 1;
      const int64_t cur = prev < x ? prev : x;
      const int64_t before = (int64_t)k + (prev < 0 ? prev : 0);
      const int64_t after = (int64_t)k + 1 + (cur < 0 ? cur : 0);
      if (after == before + 1) adm |= (uint8_t)(1u << c);
      prev = cur;
      ++k;
    }
    WIDE_PH(4);
    uint32_t n_lost = 0, n_copies = 0, n_over = 0;
    tgsim_record r1, r2;
    int q1 = -1, q2 = -1;
    if (tid < n) {
      if (st != TGSIM_ST_LOST) {
        const uint8_t dropped = valid & ~adm;
        if (dropped & 2u) st |= TGSIM_ST_FLAG_CLONE_LOST;
        if (dropped & 1u) st |= TGSIM_ST_FLAG_OVERLIMIT;
        if (!adm) st = (uint8_t)((st & 0xF0u) | TGSIM_ST_OVERLIMIT);
        n_over = (uint32_t)__popc(dropped);
        n_copies = (uint32_t)__popc(adm);
      } else {
        n_lost = 1;
      }
      a.status[idx] = st;
      r1.t = e2[1]; r1.src = src; r1.dst = dst; r1.seq = seq; r1.size = size; r1.meta = meta2[1]; r1.corrupt_off = coff2[1];
      r2.t = e2[0]; r2.src = src; r2.dst = dst; r2.seq = seq; r2.size = size; r2.meta = meta2[0]; r2.corrupt_off = coff2[0];
      if (adm & 2u) q1 = qid_copy(a.geo, r1, t_end);
      if (adm & 1u) q2 = qid_copy(a.geo, r2, t_end);
    }
    const int qs[2] = {q1, q2};
    const tgsim_record rs[2] = {r1, r2};
    a.Q.push_batch<2, kWideWaves>(qs, rs, l + (tid >> 6), true);
    WIDE_PH(5);
    // the sender's counters: per wave sums into the wave's LDS slots, one barrier, thread 0 folds
    // them. No barrier after: the slots are next written at the next sender's tail, and every other
    // LDS array of this sender was last read before the barrier above.
    {
      const uint32_t wl = wave_sum(n_lost), wc = wave_sum(n_copies), wo = wave_sum(n_over);
      if (lane_id() == 0) { s_wtot[tid >> 6][0] = wl; s_wtot[tid >> 6][1] = wc; s_wtot[tid >> 6][2] = wo; }
    }
    {  // the next sender's send-time range (its loads have landed by now) and flags, for its sort
      const bool nv = tid < nm.n && nm.n <= (uint32_t)kWide;
      int64_t nmn = nv ? pf.ts : INT64_MAX, nmx = nv ? pf.ts : INT64_MIN;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int64_t x = __shfl_xor(nmn, o), y = __shfl_xor(nmx, o);
        nmn = x < nmn ? x : nmn;
        nmx = y > nmx ? y : nmx;
      }
      if (lane_id() == 0) { rnmin[tid >> 6] = nmn; rnmax[tid >> 6] = nmx; }
      if (tid == 0) { s_flag = 0; s_stage_a = 0; s_big = 0; }
    }
    mm_ready = true;
    __syncthreads();
    if (tid == 0) {
      uint32_t tl = 0, tc = 0, to = 0;
#pragma unroll
      for (int w = 0; w < kWideWaves; ++w) { tl += s_wtot[w][0]; tc += s_wtot[w][1]; to += s_wtot[w][2]; }
      unsigned long long* row = a.stats + (size_t)(l & (kNSub - 1)) * 16;
      if (tl) atomicAdd(&row[ST_LOST], (unsigned long long)tl);
      if (tc) atomicAdd(&row[ST_COPIES], (unsigned long long)tc);
      if (to) atomicAdd(&row[ST_OVERLIMIT], (unsigned long long)to);
      atomicAdd(&sc->kc[KC_WIDE], (unsigned long long)n);
      done[l] = 1;
    }
    WIDE_PH(6);
  }
}

// init_crandom at a Shape call: Philox(g, epoch, 0, "CORR") words 0..2 (the kernel uses prandom).
__global__ void k_reset_corr(const uint32_t* pairs, uint32_t n, uint32_t lo, uint32_t k0, uint32_t k1,
                             uint32_t* last4) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = pairs[2 * i], ep = pairs[2 * i + 1];
  uint32_t o[4];
  philox4x32_10(lo + l, ep, 0u, 0x434F5252u /* "CORR" */, k0, k1, o);
  last4[4 * l] = o[0]; last4[4 * l + 1] = o[1]; last4[4 * l + 2] = o[2]; last4[4 * l + 3] = 0;
}

// Commit a sorted batch: per present state, check time order, append a log chunk, bump the count.
__global__ __launch_bounds__(kBlock) void k_sig_commit(const uint32_t* off, uint32_t K, uint32_t kmin,
                                                       uint64_t log_base, const int64_t* log, uint32_t* count,
                                                       int64_t* last, uint32_t* nchunks, SigChunk* chunks,
                                                       DevScalars* sc) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
    const uint32_t a = off[k], b = off[k + 1];
    if (a == b) continue;
    const uint32_t st = kmin + k;
    const int64_t first = log[log_base + a];
    if (count[st] > 0 && first < last[st]) atomicOr(&sc->err, ERR_SIG_ORDER);
    const uint32_t c = nchunks[st];
    if (c >= (uint32_t)kMaxChunksPerState) {
      atomicOr(&sc->err, ERR_STATE_CHUNKS);
    } else {
      SigChunk ch;
      ch.seq_start = count[st] + 1u; ch.len = b - a; ch.log_pos = log_base + a;
      ch.tmin = first; ch.tmax = log[log_base + b - 1]; ch.sorted = 1; ch.pad = 0;
      chunks[(size_t)st * kMaxChunksPerState + c] = ch;
      nchunks[st] = c + 1;
    }
    count[st] += b - a;
    last[st] = log[log_base + b - 1];
  }
}

// Sync-service state a kernel needs to commit a count-only signal batch and resolve waiters.
struct SigState {
  uint32_t* count;
  int64_t* last;
  uint32_t* nchunks;
  SigChunk* chunks;
  const int64_t* log;
  const uint32_t* w_state;
  const uint32_t* w_target;
  const int64_t* w_twait;
  int64_t* w_release;
  int64_t* red;   // [4]: the last batch's tmin at [0], tmax at [3]
  int64_t* part;  // [2 * kSigParts]: per-block (min, max) of a batch
  DevScalars* sc;
};

constexpr uint32_t kSigParts = 4096;  // blocks of a batch reduction (grid-stride beyond)
constexpr uint32_t kSpecGenBlocks = 512;  // generator blocks inside the wheel-insert launch (k_wheel_scatter_gen)

// Commit a count-only batch of n signals of state st with times in [tmin, tmax] (one thread).
__device__ __forceinline__ void sig_commit_count(const SigState& g, uint32_t n, uint32_t st, int64_t tmin,
                                                 int64_t tmax) {
  if (n == 0) return;
  if (g.count[st] > 0 && tmin < g.last[st]) atomicOr(&g.sc->err, ERR_SIG_ORDER);
  const uint32_t c = g.nchunks[st];
  if (c >= (uint32_t)kMaxChunksPerState) {
    atomicOr(&g.sc->err, ERR_STATE_CHUNKS);
  } else {
    SigChunk ch;
    ch.seq_start = g.count[st] + 1u; ch.len = n; ch.log_pos = 0;
    ch.tmin = tmin; ch.tmax = tmax; ch.sorted = 0; ch.pad = 0;
    g.chunks[(size_t)st * kMaxChunksPerState + c] = ch;
    g.nchunks[st] = c + 1;
  }
  g.count[st] += n;
  g.last[st] = tmax;
}

// A waiter's release time: the time of the target-th signal of its state. For a count-only chunk
// only its first and last member are known (min / max time); other targets set ERR_UNSORTED_TARGET.
__device__ __forceinline__ void resolve_waiter(const SigState& g, uint32_t w) {
  if (g.w_release[w] >= 0) return;
  const uint32_t st = g.w_state[w], tg = g.w_target[w];
  const int64_t tw = g.w_twait[w];
  if (tg == 0) { g.w_release[w] = tw; return; }
  if (g.count[st] < tg) return;
  const uint32_t nc = g.nchunks[st];
  for (uint32_t c = 0; c < nc; ++c) {
    const SigChunk ch = g.chunks[(size_t)st * kMaxChunksPerState + c];
    if (tg >= ch.seq_start && tg < ch.seq_start + ch.len) {
      int64_t t;
      if (ch.sorted) t = g.log[ch.log_pos + (tg - ch.seq_start)];
      else if (tg == ch.seq_start + ch.len - 1) t = ch.tmax;
      else if (tg == ch.seq_start) t = ch.tmin;
      else { atomicOr(&g.sc->err, ERR_UNSORTED_TARGET); return; }
      g.w_release[w] = t > tw ? t : tw;
      return;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_waiters(SigState g, uint32_t nw) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += stride) resolve_waiter(g, w);
}

struct WaiterAdd {
  uint32_t* w_state;
  uint32_t* w_target;
  int64_t* w_twait;
  uint32_t state, target;
  int64_t t_wait;
  uint32_t on;
};

__global__ void k_add_waiter(SigState g, uint32_t* w_state, uint32_t* w_target, int64_t* w_twait, uint32_t i,
                             uint32_t state, uint32_t target, int64_t t_wait) {
  w_state[i] = state; w_target[i] = target;
  w_twait[i] = t_wait == INT64_MIN ? g.sc->t_end : t_wait;
  g.w_release[i] = -1;
  resolve_waiter(g, i);  // the other waiters can only move when signals arrive
}

// Block-reduce (min, max) of a signal batch into this block's partial (no atomics: a batch has
// thousands of blocks, and same-address device atomics serialise at the memory side).
__device__ __forceinline__ void sig_block_partial(const SigState& g, int64_t mn, int64_t mx,
                                                  uint32_t bid = 0xFFFFFFFFu) {
  if (bid == 0xFFFFFFFFu) bid = blockIdx.x;
  __shared__ int64_t smin[kBlock / 64], smax[kBlock / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smin[w] = mn; smax[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / 64; ++k) { mn = smin[k] < mn ? smin[k] : mn; mx = smax[k] > mx ? smax[k] : mx; }
    g.part[2 * bid] = mn;
    g.part[2 * bid + 1] = mx;
  }
}

// One block: the batch's (min, max) from the partials -> red[0], red[3]; with commit, the batch is
// committed count-only to state st and waiters [0, nw) are resolved. wa.on: a barrier registered
// right after the batch (waiter nw) is added and resolved in the same launch.
__device__ __forceinline__ void sig_commit_block(const SigState& g, uint32_t nparts, uint32_t commit, uint32_t n,
                                                 uint32_t st, uint32_t nw, const WaiterAdd& wa) {
  if (wa.on && threadIdx.x == 0) {
    wa.w_state[nw] = wa.state; wa.w_target[nw] = wa.target;
    wa.w_twait[nw] = wa.t_wait == INT64_MIN ? g.sc->t_end : wa.t_wait;
    g.w_release[nw] = -1;
  }
  if (wa.on) ++nw;
  __shared__ int64_t smin[kBlock / 64], smax[kBlock / 64];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (uint32_t i = threadIdx.x; i < nparts; i += kBlock) {
    const int64_t a = g.part[2 * i], b = g.part[2 * i + 1];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smin[w] = mn; smax[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / 64; ++k) { mn = smin[k] < mn ? smin[k] : mn; mx = smax[k] > mx ? smax[k] : mx; }
    g.red[0] = mn;
    g.red[3] = mx;
    if (commit) sig_commit_count(g, n, st, mn, mx);
  }
  if (nw && (commit || wa.on)) {
    __syncthreads();
    for (uint32_t i = commit ? threadIdx.x : nw - 1 + threadIdx.x; i < nw; i += kBlock) resolve_waiter(g, i);
  }
}

__global__ __launch_bounds__(kBlock) void k_sig_commit(SigState g, uint32_t nparts, uint32_t commit, uint32_t n,
                                                       uint32_t st, uint32_t nw, WaiterAdd wa) {
  sig_commit_block(g, nparts, commit, n, st, nw, wa);
}

// The storm step's deferred commit + barrier registration and the window start that waits on that
// barrier, in one single-block launch (the window end is the waiter's release, resolved here).
// The same work as sig_commit_block + window_start_block, with the chain of dependent global round
// trips cut from ~16 to ~4: every load that nothing in this launch writes first is issued at entry
// (batch partials, the state's count / last / chunk count, the old waiters' releases, the window
// and region-ring scalars), each live region's fields one round trip later (overlapping the
// commit), the registered waiter's release is computed from the new chunk in registers, and the
// retired prefix of the region ring is found in parallel (thread 0 walked it). More than kBlock
// live regions or waiters take the general chain.
__global__ __launch_bounds__(kBlock) void k_window_start_commit(SigState g, uint32_t nparts, uint32_t n, uint32_t st,
                                                                uint32_t nw, WaiterAdd wa, WindowArgs w) {
  DevScalars* sc = w.sc;
  const uint32_t tid = threadIdx.x;
  const uint32_t tail = sc->reg_tail, head = sc->reg_head, nlive = head - tail;
  const int64_t H0 = sc->T, T0 = sc->t_end;
  const uint64_t arena_head0 = sc->arena_head, arena_used0 = sc->arena_used;
  const uint32_t nw_old = nw;
  if (nlive > (uint32_t)kBlock || nw_old >= (uint32_t)kBlock) {  // block-uniform: the general chain
    sig_commit_block(g, nparts, 1u, n, st, nw, wa);
    __syncthreads();  // the waiter's release (written by some thread of this block) is visible
    window_start_block(w);
    return;
  }
  uint32_t cnt0 = 0, nch0 = 0;
  int64_t last0 = 0;
  if (tid == 0) { cnt0 = g.count[st]; last0 = g.last[st]; nch0 = g.nchunks[st]; }
  const int64_t rel_old = tid < nw_old ? g.w_release[tid] : 0;
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (uint32_t i = tid; i < nparts; i += kBlock) {
    const int64_t a = g.part[2 * i], b = g.part[2 * i + 1];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  RegionDev* rp = nullptr;
  uint32_t r_cons = 0, r_n = 0, r_dir = 0;
  int64_t r_base = 0;
  uint64_t r_aoff = 0;
  if (tid < nlive) {
    rp = &w.regions[(tail + tid) % kMaxRegions];
    r_cons = rp->consumed; r_n = rp->n; r_base = rp->base_slot; r_dir = rp->dir; r_aoff = rp->arena_off;
  }
  // the per-window counters (nothing below reads them before the barriers)
  for (uint32_t i = tid; i < kQcLines; i += kBlock) w.qc[i << 5] = 0;
  {
    uint32_t* wb = sc->q;
    const uint32_t nwb = (uint32_t)((offsetof(DevScalars, err) - offsetof(DevScalars, q)) / sizeof(uint32_t));
    for (uint32_t i = tid; i < nwb; i += kBlock) wb[i] = 0;
  }
  __shared__ int64_t smin[kBlock / 64], smax[kBlock / 64];
  __shared__ int64_t s_tend;
  __shared__ uint32_t s_open;
  __shared__ uint32_t s_part[kBlock / 64];
  __shared__ unsigned long long s_freed[kBlock / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((tid & 63) == 0) { smin[tid >> 6] = mn; smax[tid >> 6] = mx; }
  __syncthreads();
  bool fast_rel = false;  // thread 0: the window's waiter is the one registered here, resolved in registers
  int64_t rel_new = -1;
  if (tid == 0) {
    for (int k = 1; k < kBlock / 64; ++k) { mn = smin[k] < mn ? smin[k] : mn; mx = smax[k] > mx ? smax[k] : mx; }
    g.red[0] = mn;
    g.red[3] = mx;
    bool chunk_ok = false;
    if (n) {  // sig_commit_count on the preloaded state
      if (cnt0 > 0 && mn < last0) atomicOr(&sc->err, ERR_SIG_ORDER);
      if (nch0 >= (uint32_t)kMaxChunksPerState) {
        atomicOr(&sc->err, ERR_STATE_CHUNKS);
      } else {
        SigChunk ch;
        ch.seq_start = cnt0 + 1u; ch.len = n; ch.log_pos = 0;
        ch.tmin = mn; ch.tmax = mx; ch.sorted = 0; ch.pad = 0;
        g.chunks[(size_t)st * kMaxChunksPerState + nch0] = ch;
        g.nchunks[st] = nch0 + 1;
        chunk_ok = true;
      }
      g.count[st] = cnt0 + n;
      g.last[st] = mx;
    }
    if (wa.on) {
      const int64_t tw = wa.t_wait == INT64_MIN ? T0 : wa.t_wait;
      wa.w_state[nw_old] = wa.state; wa.w_target[nw_old] = wa.target; wa.w_twait[nw_old] = tw;
      // resolve_waiter's answer where it follows from this commit alone; otherwise the general path
      const uint32_t tg = wa.target, cnt1 = cnt0 + n;
      bool known = false;
      if (tg == 0) {
        rel_new = tw; known = true;
      } else if (wa.state == st && n) {
        if (cnt1 < tg) {
          known = true;
        } else if (tg > cnt0) {  // inside the new chunk
          known = true;
          if (chunk_ok) {
            if (tg == cnt1) rel_new = mx > tw ? mx : tw;
            else if (tg == cnt0 + 1u) rel_new = mn > tw ? mn : tw;
            else atomicOr(&sc->err, ERR_UNSORTED_TARGET);
          }
        }
      }
      g.w_release[nw_old] = known ? rel_new : -1;
      if (!known) resolve_waiter(g, nw_old);
      fast_rel = known && w.mode == WIN_BARRIER && w.src == g.w_release + nw_old;
    }
  }
  __syncthreads();  // the commit is visible to the old waiters' resolution
  if (tid < nw_old && rel_old < 0) resolve_waiter(g, tid);
  __syncthreads();  // every release is written
  if (tid == 0) {
    int64_t e = w.t_end_arg;
    if (w.mode == WIN_BARRIER) {
      const int64_t rel = fast_rel ? rel_new : *w.src;
      if (rel < 0) {
        atomicOr(&sc->err, ERR_UNRELEASED);
        e = T0;
      } else {
        e = rel + w.offset;
      }
    } else if (w.mode == WIN_DEVICE) {
      e = *w.src + w.offset;
    }
    e = e < T0 ? T0 : e;
    sc->H = H0;
    sc->T = T0;
    sc->t_end = e;
    sc->base_slot = e / w.slot_ns;
    s_tend = e;
    s_open = nlive;
  }
  __syncthreads();
  // the extraction plan (plan_regions with the region fields already in registers)
  const int64_t t_end = s_tend;
  const int64_t kabs = t_end > 0 ? (t_end - 1) / w.slot_ns : -1;
  uint32_t len = 0;
  if (tid < nlive) {
    const uint32_t start = r_cons;
    uint32_t hi = start;
    if (kabs >= 0) {
      const int64_t krel = kabs - r_base;
      if (krel >= (int64_t)w.slots - 1) hi = r_n;
      else if (krel >= 0) hi = w.dirs[(size_t)r_dir * (w.slots + 1) + (uint32_t)krel + 1];
    }
    if (hi < start) hi = start;
    len = hi - start;
    rp->consumed = hi;
    w.plan_start[tid] = start;
    if (hi != r_n) atomicMin(&s_open, tid);
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan(len, s_part, total);  // its barriers also publish s_open
  if (tid < nlive) w.plan_off[tid] = ex;
  const uint32_t open = s_open;  // regions [0, open) of the ring are fully consumed: retired
  unsigned long long fr = (tid < open) ? (unsigned long long)r_n : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fr += __shfl_xor(fr, o);
  if ((tid & 63) == 0) s_freed[tid >> 6] = fr;
  __syncthreads();
  if (tid == open && open < nlive) sc->arena_tail = r_aoff;
  if (tid == 0) {
    unsigned long long freed = 0;
    for (int k = 0; k < kBlock / 64; ++k) freed += s_freed[k];
    w.plan_off[nlive] = total;
    sc->n_extract = total;
    sc->plan_tail = tail;
    sc->plan_n = nlive;
    sc->reg_tail = tail + open;
    sc->arena_used = arena_used0 - freed;
    if (open == nlive) sc->arena_tail = arena_head0;
  }
}

// A sharded storm batch over a transport: the shard's (first, last) time from the generator's
// partials as {last, -first} for one MAX all-reduce (k_storm_red), and the reduced pair back as the
// batch's single partial (k_storm_unpack), which the fused commit then takes for the whole batch.
__global__ __launch_bounds__(kBlock) void k_storm_red(const int64_t* part, uint32_t nparts, int64_t* red2) {
  __shared__ int64_t smin[kBlock / 64], smax[kBlock / 64];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (uint32_t i = threadIdx.x; i < nparts; i += kBlock) {
    mn = part[2 * i] < mn ? part[2 * i] : mn;
    mx = part[2 * i + 1] > mx ? part[2 * i + 1] : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = mn; smax[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / 64; ++k) { mn = smin[k] < mn ? smin[k] : mn; mx = smax[k] > mx ? smax[k] : mx; }
    red2[0] = mx;
    red2[1] = mn == INT64_MAX ? INT64_MIN : -mn;  // an empty shard contributes nothing
  }
}
__global__ void k_storm_unpack(const int64_t* red2, int64_t* part) {
  part[0] = -red2[1];
  part[1] = red2[0];
}

// Count-only batch (one state, no sequence numbers): min and max time, then the commit.
__global__ __launch_bounds__(kBlock) void k_sig_count(SigState g, const int64_t* t, uint32_t n) {
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t v = t[i];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  sig_block_partial(g, mn, mx);
}

// ============================================================================================
// the rest of a group-by's segments, in one launch and without a host round trip: medium segments
// (kThreadSeg < len <= kTile) get one block each (LDS sort + the policy's epilogue); a large segment
// (len > kTile) is owned by one block from start to end - its kChunk chunks are sorted in LDS, merged
// pairwise through the (K1, K2, K3) scratch inside the block, and handed to the policy's large
// consumer. Nothing to do costs one launch of early-exiting blocks.
// ============================================================================================

__device__ void large_consume(const TBPolicy& p, SortSmem& s, const LargeSeg& L, const uint64_t* K1,
                              const uint32_t* K3, uint32_t salt) {
  bool has_carry = false;
  int64_t carry = 0;
  for (uint32_t t0 = 0; t0 < L.len; t0 += kChunk, salt += 16) {
    const uint32_t cnt = min((uint32_t)kChunk, L.len - t0);
    for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) {
      s.sg[j] = L.seg; s.k1[j] = K1[L.start + t0 + j]; s.k3[j] = K3[L.start + t0 + j]; s.perm[j] = j;
    }
    __syncthreads();
    p.scan(s, cnt, has_carry, carry, t0 + cnt == L.len, salt);
    carry = s.carry;
    has_carry = true;
    __syncthreads();
  }
}

__device__ void large_consume(const EmitPolicy& p, SortSmem&, const LargeSeg& L, const uint64_t*, const uint32_t* K3,
                              uint32_t) {
  for (uint32_t j = threadIdx.x; j < L.len; j += kBlock) p.write(L.start + j, K3[L.start + j]);
}

__device__ void large_consume(const SigPolicy& p, SortSmem&, const LargeSeg& L, const uint64_t* K1, const uint32_t* K3,
                              uint32_t) {
  for (uint32_t j = threadIdx.x; j < L.len; j += kBlock)
    p.write(L.seg, L.start + j, L.start, K1[L.start + j], K3[L.start + j]);
}

__device__ void large_consume(const CorrPolicy& p, SortSmem&, const LargeSeg& L, const uint64_t*, const uint32_t* K3,
                              uint32_t) {
  for (uint32_t j = threadIdx.x; j < L.len; j += kBlock) p.sorted[L.start + j] = K3[L.start + j];
}

// Sort chunk [c0, c0 + kChunk) of a large segment in LDS into (K1a, K2a, K3a) at the same positions.
template <class P>
__device__ void large_chunk_sort(const P& p, SortSmem& s, const LargeSeg& L, uint32_t c0, const uint32_t* keys,
                                 const uint32_t* vals, uint64_t* K1a, uint64_t* K2a, uint32_t* K3a,
                                 uint32_t chunk = kChunk) {
  const uint32_t st = L.start + c0;
  const uint32_t cnt = min(chunk, L.len - c0);
  const uint32_t npad = next_pow2(cnt);
  load_span_keys(p, s, keys, vals, st, cnt, npad);
  __syncthreads();
#ifdef TGSIM_PHASE_PROF
  if (threadIdx.x == 0) g_chunk_ph[0] = __builtin_amdgcn_s_memrealtime();
#endif
  if (packed_bitonic(s, cnt, npad)) {  // sorted through perm, the arrays in place
    for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) {
      const uint32_t e = s.perm[j];
      K1a[st + j] = s.k1[e]; K2a[st + j] = s.k2[e]; K3a[st + j] = s.k3[e];
    }
  } else {
    bitonic_lds(s, npad);
    for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) { K1a[st + j] = s.k1[j]; K2a[st + j] = s.k2[j]; K3a[st + j] = s.k3[j]; }
  }
#ifdef TGSIM_PHASE_PROF
  if (threadIdx.x == 0) g_chunk_ph[1] = __builtin_amdgcn_s_memrealtime();
#endif
  __syncthreads();
}

// Sort one large segment inside the calling block; returns the buffer set that holds the result.
template <class P>
__device__ bool large_sort_block(const P& p, SortSmem& s, const LargeSeg& L, const uint32_t* keys,
                                 const uint32_t* vals, uint64_t* K1a, uint64_t* K2a, uint32_t* K3a, uint64_t* K1b,
                                 uint64_t* K2b, uint32_t* K3b) {
  for (uint32_t c0 = 0; c0 < L.len; c0 += kChunk) large_chunk_sort(p, s, L, c0, keys, vals, K1a, K2a, K3a);
  bool in_a = true;
  constexpr uint32_t IT = kChunk / kBlock;
  for (uint32_t W = kChunk; W < L.len; W *= 2) {
    const uint64_t* sK1 = in_a ? K1a : K1b;
    const uint64_t* sK2 = in_a ? K2a : K2b;
    const uint32_t* sK3 = in_a ? K3a : K3b;
    uint64_t* dK1 = in_a ? K1b : K1a;
    uint64_t* dK2 = in_a ? K2b : K2a;
    uint32_t* dK3 = in_a ? K3b : K3a;
    const uint32_t base = L.start;
    // Output tile [o0, o1) of the pair [As, Be): its A and B slices come from two merge-path
    // splits, are staged in LDS with coalesced loads, and merged there - each thread its IT outputs
    // after a merge-path search in LDS (the per-thread searches and merges over global memory were
    // chains of dependent loads). The splits of every tile boundary of the pass are searched at
    // once, one thread each (tile t starts at t * kChunk; a tile never spans two pairs), so a pass
    // pays one search latency, not one per tile: a 10k-delivery inbox took ~300 us in one block.
    // Boundaries beyond sg's capacity are searched per tile.
    __shared__ uint32_t spl[2];
    const uint32_t ntiles = (L.len + kChunk - 1) / kChunk;
    const bool pre = ntiles < (uint32_t)kSpan;  // block-uniform
    if (pre) {
      for (uint32_t t = threadIdx.x; t <= ntiles; t += kBlock) {
        // boundary o = t * kChunk (the segment end for t = ntiles), as the end of tile t - 1 (the
        // pair of tile t - 1) -> sg[t]; as the start of tile t -> perm[t]
        const uint32_t o = min(t * (uint32_t)kChunk, L.len);
        for (int side = 0; side < 2; ++side) {
          if (side == 0 && t == 0) continue;
          if (side == 1 && t == ntiles) continue;
          const uint32_t ot = side ? o : o - 1;  // an output inside the tile whose pair is wanted
          const uint32_t As = (ot / (2 * W)) * 2 * W;
          const uint32_t Ae = min(As + W, L.len), Be = min(As + 2 * W, L.len);
          const uint32_t nA = Ae - As, nB = Be - Ae;
          const uint32_t a0 = base + As, b0 = base + Ae;
          const uint32_t d = o - As;
          uint32_t lo = d > nB ? d - nB : 0u, hi = min(d, nA);
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (!kless(sK1, sK2, sK3, b0 + (d - 1 - mid), a0 + mid)) lo = mid + 1; else hi = mid;
          }
          (side ? s.perm : s.sg)[t] = lo;
        }
      }
      __syncthreads();
    }
    for (uint32_t o0 = 0; o0 < L.len; o0 += kChunk) {
      const uint32_t o1 = min(o0 + (uint32_t)kChunk, L.len);
      const uint32_t As = (o0 / (2 * W)) * 2 * W;
      const uint32_t Ae = min(As + W, L.len), Be = min(As + 2 * W, L.len);
      const uint32_t nA = Ae - As, nB = Be - Ae;
      const uint32_t a0 = base + As, b0 = base + Ae;
      if (pre) {
        if (threadIdx.x == 0) {
          const uint32_t t = o0 / kChunk;
          spl[0] = s.perm[t];
          spl[1] = s.sg[t + 1];
        }
      } else if (threadIdx.x < 2) {
        const uint32_t d = (threadIdx.x ? o1 : o0) - As;
        uint32_t lo = d > nB ? d - nB : 0u, hi = min(d, nA);
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (!kless(sK1, sK2, sK3, b0 + (d - 1 - mid), a0 + mid)) lo = mid + 1; else hi = mid;
        }
        spl[threadIdx.x] = lo;
      }
      __syncthreads();
      const uint32_t ia0 = spl[0], ib0 = (o0 - As) - ia0;
      const uint32_t na = spl[1] - ia0, nt = o1 - o0, nb = nt - na;
      for (uint32_t j = threadIdx.x; j < nt; j += kBlock) {
        const uint32_t src = j < na ? a0 + ia0 + j : b0 + ib0 + (j - na);
        s.k1[j] = sK1[src]; s.k2[j] = sK2[src]; s.k3[j] = sK3[src];
      }
      __syncthreads();
      const uint32_t d0 = threadIdx.x * IT;
      if (d0 < nt) {
        uint32_t lo = d0 > nb ? d0 - nb : 0u, hi = min(d0, na);
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (!kless(s.k1, s.k2, s.k3, na + (d0 - 1 - mid), mid)) lo = mid + 1; else hi = mid;
        }
        uint32_t ia = lo, ib = d0 - lo;
        for (uint32_t k = 0; k < IT && d0 + k < nt; ++k) {
          bool takeA;
          if (ib >= nb) takeA = true;
          else if (ia >= na) takeA = false;
          else takeA = !kless(s.k1, s.k2, s.k3, na + ib, ia);
          const uint32_t src = takeA ? ia++ : na + ib++;
          const uint32_t dst = base + o0 + d0 + k;
          dK1[dst] = s.k1[src]; dK2[dst] = s.k2[src]; dK3[dst] = s.k3[src];
        }
      }
      __syncthreads();  // the staged slices and spl are rewritten by the next tile
    }
    __syncthreads();
    in_a = !in_a;
  }
  return in_a;
}

// Where a ranked element of a large segment goes (the tasks of rest_body): the deliveries, signal
// sequence numbers and deferred-message order are written at their sorted position at once; the
// token bucket's GCRA runs along the whole segment in order, so its elements are placed in
// (K1b, K2b, K3b) and the segment's last rank task scans them (large_consume).
__device__ __forceinline__ void large_place(const EmitPolicy& p, const LargeSeg& L, uint32_t r, uint64_t, uint64_t,
                                            uint32_t k3, uint64_t*, uint64_t*, uint32_t*) {
  p.write(L.start + r, k3);
}
__device__ __forceinline__ void large_place(const SigPolicy& p, const LargeSeg& L, uint32_t r, uint64_t k1, uint64_t,
                                            uint32_t k3, uint64_t*, uint64_t*, uint32_t*) {
  p.write(L.seg, L.start + r, L.start, k1, k3);
}
__device__ __forceinline__ void large_place(const CorrPolicy& p, const LargeSeg& L, uint32_t r, uint64_t, uint64_t,
                                            uint32_t k3, uint64_t*, uint64_t*, uint32_t*) {
  p.sorted[L.start + r] = k3;
}
__device__ __forceinline__ void large_place(const TBPolicy&, const LargeSeg& L, uint32_t r, uint64_t k1, uint64_t k2,
                                            uint32_t k3, uint64_t* K1b, uint64_t* K2b, uint32_t* K3b) {
  K1b[L.start + r] = k1; K2b[L.start + r] = k2; K3b[L.start + r] = k3;
}
template <class P> struct LargeScan { static constexpr bool v = false; };
template <> struct LargeScan<TBPolicy> { static constexpr bool v = true; };

// elements of the sorted chunk (K1, K2, K3)[b, b + n) below the key (k1, k2, k3): kRankPar chunks'
// binary searches advance together, so their loads are in flight at once
#ifndef TGSIM_RANK_PAR
#define TGSIM_RANK_PAR 8
#endif
constexpr int kRankPar = TGSIM_RANK_PAR;  // chunks whose binary searches a rank thread runs together
__device__ __forceinline__ void below_n(const uint64_t* K1, const uint64_t* K2, const uint32_t* K3, const uint32_t (&b)[kRankPar],
                                       const uint32_t (&n)[kRankPar], uint64_t k1, uint64_t k2, uint32_t k3, uint32_t (&lo)[kRankPar]) {
  uint32_t hi[kRankPar];
#pragma unroll
  for (int q = 0; q < kRankPar; ++q) { lo[q] = 0; hi[q] = n[q]; }
  for (;;) {
    bool any = false;
#pragma unroll
    for (int q = 0; q < kRankPar; ++q) {
      if (lo[q] >= hi[q]) continue;
      any = true;
      const uint32_t mid = (lo[q] + hi[q]) >> 1, x = b[q] + mid;
#ifdef TGSIM_RANK_LAZY
      const uint64_t y1 = K1[x];
      const bool lt = y1 != k1 ? y1 < k1 : key_less(0, y1, K2[x], K3[x], 0, k1, k2, k3);
#else
      // all three words in one round trip: a probed target's requests share their arrival time, and
      // loading (k2, k3) only after k1 tied made every search step two dependent loads
      const uint64_t y1 = K1[x], y2 = K2[x];
      const uint32_t y3 = K3[x];
      const bool lt = key_less(0, y1, y2, y3, 0, k1, k2, k3);
#endif
      if (lt) lo[q] = mid + 1; else hi[q] = mid;
    }
    if (!any) break;
  }
}

constexpr uint32_t kRankTile = kBlock;   // elements of a large segment ranked per task (one per thread)
#ifndef TGSIM_PAR_CHUNK
#define TGSIM_PAR_CHUNK 1024
#endif
constexpr uint32_t kParChunk = TGSIM_PAR_CHUNK;  // chunk of the task-parallel path
constexpr uint32_t kLargeTab = 256;      // large segments whose task table fits LDS (else one block each)
#ifndef TGSIM_RANK_ST0
#define TGSIM_RANK_ST0 4
#endif
#ifndef TGSIM_SPIN_SLEEP
#define TGSIM_SPIN_SLEEP 2               // a waiting rank task's poll period, in units of 64 clocks
#endif

// The rest of a group-by's segments. Medium segments: one block each. Large segments (len > kTile)
// are sorted by many blocks at once through a task counter: first every kChunk chunk
// of every large segment is sorted in LDS by its own task, then every element is ranked by its own
// task thread - its place in its chunk plus, in every other sorted chunk, the number of elements below
// it (binary searches) - and placed. A rank task waits until its segment's chunks are sorted
// (LargeSeg::pad counts them); tasks are claimed in that order, so a waiting block only waits on
// tasks that running blocks hold. One block sorting a 10k-delivery inbox through merge passes took
// ~280 us; the tasks take the time of one chunk sort and one rank search.
// which implementation counter (DevScalars::kc) counts a policy's long-segment items
template <class P> struct KcLong { static constexpr int v = -1; };
template <> struct KcLong<TBPolicy> { static constexpr int v = KC_LONG_TB; };
template <> struct KcLong<EmitPolicy> { static constexpr int v = KC_LONG_EMIT; };
template <class P>
__device__ __forceinline__ void count_long(const DevScalars* sc, uint32_t len) {
  if (KcLong<P>::v >= 0 && threadIdx.x == 0)
    atomicAdd(const_cast<unsigned long long*>(&sc->kc[KcLong<P>::v]), (unsigned long long)len);
}

// EXPERIMENT BUILD ONLY (-DTGSIM_WHOLE_SORT; the product sorts every long inbox with the tasks).
// One workgroup sorts a whole long inbox of up to kWholeMax deliveries in LDS (VERDICT r5 item 5:
// config 3's ~10k requests at one probed node take chunk tasks plus rank searches through global
// memory, 34 us of its 83 busy us per window):
//   A  the records are gathered for the block's minimum and maximum of t, src and seq. The key packs
//      into 32 bits when the three offsets from their minimums and the clone bit fit: t | src | seq |
//      !clone, most significant first - the order key_less gives (k1, k2, k3 >> 31);
//   B  the records again (from this XCD's L2 now): each thread keeps its 40 packed keys in registers
//      and counts them into kWholeBkt LDS buckets by their top bits, then the counts are scanned;
//   C  every packed key is slotted into its bucket (LDS);
//   D  a delivery's sorted place is its bucket's start plus its bucket mates below it; it is written
//      there from its record.
// Measured on config 3 (a 9,993-request inbox, tools/gpu.sh ab): the insert launch took 67-72 us
// with it against 35 us with the tasks. One CU gathers the 10k scattered 32-B records three times
// (A, B, D) through its own L1 - ~20k line requests per pass - where the tasks spread them over 10
// chunk and 40 rank workgroups; batching 8 gathers per thread (whole_gather_idx: the first version's
// per-element branches made them ~100 dependent round trips, 85 us) did not change that bound.
// The workgroup hands the segment back to the chunk and rank tasks, before writing any delivery,
// when the key needs more than 32 bits, a bucket holds more than kWholeMate keys (D is O(mates)), or
// two packed keys are equal (two deliveries with one (src, seq, clone): the contract excludes it,
// and the tasks then order them by record index as always). Its verdict goes to LargeSeg::pad bits
// 30/31, which the segment's chunk and rank tasks wait for.
#ifndef TGSIM_WHOLE_MAX
#define TGSIM_WHOLE_MAX 10240
#endif
#ifndef TGSIM_WHOLE_BATCH
#define TGSIM_WHOLE_BATCH 8
#endif
constexpr uint32_t kWholeMax = TGSIM_WHOLE_MAX;  // longest inbox one workgroup sorts
constexpr uint32_t kWholeBits = 12, kWholeBkt = 1u << kWholeBits;
constexpr uint32_t kWholeMate = 64;    // a fuller bucket gives the segment back to the tasks
constexpr uint32_t kWholeBatch = TGSIM_WHOLE_BATCH;    // gathers a thread keeps in flight
constexpr uint32_t kWholePer = kWholeMax / kBlock;  // elements per thread
static_assert(kWholeMax % (kBlock * kWholeBatch) == 0, "whole-inbox batches tile kWholeMax");
constexpr uint32_t kWholeDone = 1u << 30, kWholeBack = 1u << 31;  // LargeSeg::pad verdict bits
static_assert(sizeof(SortSmem) >= sizeof(uint32_t) * (kWholeBkt + kWholeMax), "whole-inbox sort fits SortSmem");
static_assert(kWholeBkt % kBlock == 0, "buckets are scanned kWholeBkt / kBlock per thread");
template <class P> struct WholeSort { static constexpr bool v = false; };
#ifdef TGSIM_WHOLE_SORT  // experiment build only: measured slower than the tasks (see above)
template <> struct WholeSort<EmitPolicy> { static constexpr bool v = true; };
#endif

struct WholePack {  // key = (t - t0) << sh_t | (src - s0) << sh_s | (seq - q0) << 1 | !clone
  uint64_t t0;
  uint32_t s0, q0, sh_t, sh_s;
  __device__ __forceinline__ uint32_t key(uint64_t t, uint32_t src, uint32_t seq, uint32_t not_clone) const {
    return (uint32_t)(((t - t0) << sh_t) | ((uint64_t)(src - s0) << sh_s) | ((uint64_t)(seq - q0) << 1) | not_clone);
  }
};
__device__ __forceinline__ uint32_t bit_width64(uint64_t x) { return x ? 64u - (uint32_t)__clzll((long long)x) : 0u; }

// Returns false (nothing written) when the segment goes back to the tasks; on true
// the deliveries are written and kWholeDone is set. Every thread calls it; the verdict is uniform.
#ifdef TGSIM_PHASE_PROF
// debug builds: the last whole sort - [0] = n | bits << 32, [1..6] s_memrealtime at its start and
// after A, B (scan), C, the equal-key check and D
__device__ uint64_t g_whole_ph[8];
#define WHOLE_PH(i, v) do { if (threadIdx.x == 0) g_whole_ph[i] = (v); } while (0)
#else
#define WHOLE_PH(i, v) do {} while (0)
#endif
// The record indices of a thread's batch: unconditional loads (a lane past the end re-reads the
// last element), so the batch's loads issue back to back - with a branch per element each one waited
// for every load before it (s_waitcnt vmcnt(0)), ~80 serial round trips per pass
__device__ __forceinline__ void whole_gather_idx(const uint32_t* v, uint32_t j0, uint32_t n, uint32_t (&x)[kWholeBatch]) {
#pragma unroll
  for (uint32_t q = 0; q < kWholeBatch; ++q) x[q] = v[min(j0 + q * kBlock, n - 1)];
}
__device__ __forceinline__ bool whole_sort(const EmitPolicy& p, SortSmem& s, const LargeSeg& L, const uint32_t* vals,
                                           uint32_t* verdict) {
  __shared__ uint64_t w_t[2];         // t min, max
  __shared__ uint32_t w_u[6];         // src min, max; seq min, max; fullest bucket; equal keys seen
  __shared__ uint32_t w_red[kBlock / 64];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(&s);  // bucket counts -> starts -> ends
  uint32_t* slot = cnt + kWholeBkt;                 // packed keys: element order (B), bucket order (C)
  const uint32_t n = L.len, b0 = L.start;
  if (threadIdx.x == 0) {
    w_t[0] = ~0ull; w_t[1] = 0;
    w_u[0] = ~0u; w_u[1] = 0; w_u[2] = ~0u; w_u[3] = 0; w_u[4] = 0; w_u[5] = 0;
  }
  for (uint32_t b = threadIdx.x; b < kWholeBkt; b += kBlock) cnt[b] = 0;
  WHOLE_PH(1, __builtin_amdgcn_s_memrealtime());
  // A: the ranges of t, src and seq; each thread keeps kWholeBatch gathers in flight
  uint64_t tlo = ~0ull, thi = 0;
  uint32_t slo = ~0u, shi = 0, qlo = ~0u, qhi = 0;
#pragma unroll 1
  for (uint32_t j0 = threadIdx.x; j0 < n; j0 += kBlock * kWholeBatch) {
    uint4 a[kWholeBatch];
    uint32_t sq[kWholeBatch];
    uint32_t x[kWholeBatch];
    whole_gather_idx(vals + b0, j0, n, x);
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q) {
      a[q] = reinterpret_cast<const uint4*>(p.D + x[q])[0];
      sq[q] = p.D[x[q]].seq;
    }
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q)
      if (j0 + q * kBlock < n) {
        const uint64_t t = ((uint64_t)a[q].y << 32) | a[q].x;
        tlo = min(tlo, t); thi = max(thi, t);
        slo = min(slo, a[q].z); shi = max(shi, a[q].z);
        qlo = min(qlo, sq[q]); qhi = max(qhi, sq[q]);
      }
  }
  __syncthreads();  // the initial values above are in place
  atomicMin(&w_t[0], tlo); atomicMax(&w_t[1], thi);
  atomicMin(&w_u[0], slo); atomicMax(&w_u[1], shi);
  atomicMin(&w_u[2], qlo); atomicMax(&w_u[3], qhi);
  __syncthreads();
  const uint32_t bt = bit_width64(w_t[1] - w_t[0]), bs = bit_width64(w_u[1] - w_u[0]),
                 bq = bit_width64(w_u[3] - w_u[2]);
  const uint32_t bits = bt + bs + bq + 1;
  WHOLE_PH(0, n | (uint64_t)bits << 32);
  WHOLE_PH(2, __builtin_amdgcn_s_memrealtime());
  if (bits > 32) return false;  // block-uniform: from LDS after the barrier
  WholePack k;
  k.t0 = w_t[0]; k.s0 = w_u[0]; k.q0 = w_u[2]; k.sh_s = 1 + bq; k.sh_t = 1 + bq + bs;
  const uint32_t shift = bits > kWholeBits ? bits - kWholeBits : 0u;
  // B: the packed keys (the records again, from this XCD's L2 now) into LDS in element order, and
  // their bucket counts
#pragma unroll 1
  for (uint32_t j0 = threadIdx.x; j0 < n; j0 += kBlock * kWholeBatch) {
    uint4 a[kWholeBatch], b[kWholeBatch];
    uint32_t x[kWholeBatch];
    whole_gather_idx(vals + b0, j0, n, x);
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q) {
      a[q] = reinterpret_cast<const uint4*>(p.D + x[q])[0];
      b[q] = reinterpret_cast<const uint4*>(p.D + x[q])[1];
    }
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q)
      if (j0 + q * kBlock < n) {
        const uint64_t t = ((uint64_t)a[q].y << 32) | a[q].x;
        const uint32_t v = k.key(t, a[q].z, b[q].x, (b[q].z & TGSIM_F_CLONE) ? 0u : 1u);
        slot[j0 + q * kBlock] = v;
        atomicAdd(&cnt[v >> shift], 1u);
      }
  }
  __syncthreads();
  {
    constexpr uint32_t per = kWholeBkt / kBlock;
    uint32_t c[per], sum = 0, big = 0;
#pragma unroll
    for (uint32_t q = 0; q < per; ++q) {
      c[q] = cnt[threadIdx.x * per + q];
      sum += c[q];
      big = max(big, c[q]);
    }
    uint32_t tot;
    uint32_t pre = block_excl_scan(sum, w_red, tot);
#pragma unroll
    for (uint32_t q = 0; q < per; ++q) { cnt[threadIdx.x * per + q] = pre; pre += c[q]; }
    if (big > kWholeMate) atomicMax(&w_u[4], big);
  }
  __syncthreads();
  WHOLE_PH(3, __builtin_amdgcn_s_memrealtime());
  if (w_u[4] > kWholeMate) return false;
  // C: the keys into bucket order in place (all read before any is moved); cnt[b] ends as the end
  // of bucket b (= the start of b + 1)
  {
    uint32_t v[kWholePer];
#pragma unroll
    for (uint32_t q = 0; q < kWholePer; ++q)
      if (q * kBlock + threadIdx.x < n) v[q] = slot[q * kBlock + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kWholePer; ++q)
      if (q * kBlock + threadIdx.x < n) slot[atomicAdd(&cnt[v[q] >> shift], 1u)] = v[q];
  }
  __syncthreads();
  WHOLE_PH(4, __builtin_amdgcn_s_memrealtime());
  for (uint32_t x = threadIdx.x; x < n; x += kBlock) {  // equal packed keys: each pair seen by its first
    const uint32_t u = slot[x], e = cnt[u >> shift];
    bool eq = false;
    for (uint32_t y = x + 1; y < e; ++y) eq |= slot[y] == u;
    if (eq) w_u[5] = 1;
  }
  __syncthreads();
  WHOLE_PH(5, __builtin_amdgcn_s_memrealtime());
  if (w_u[5]) return false;
  if (threadIdx.x == 0) atomicOr(verdict, kWholeDone);  // the tasks need nothing of this block's
  // D: every delivery's place (its bucket's start + its mates below it), written from its record
#pragma unroll 1
  for (uint32_t j0 = threadIdx.x; j0 < n; j0 += kBlock * kWholeBatch) {
    uint4 a[kWholeBatch], b[kWholeBatch];
    uint32_t x[kWholeBatch];
    whole_gather_idx(vals + b0, j0, n, x);
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q) {
      a[q] = reinterpret_cast<const uint4*>(p.D + x[q])[0];
      b[q] = reinterpret_cast<const uint4*>(p.D + x[q])[1];
    }
#pragma unroll
    for (uint32_t q = 0; q < kWholeBatch; ++q) {
      if (j0 + q * kBlock >= n) continue;
      tgsim_record r;
      r.t = (int64_t)(((uint64_t)a[q].y << 32) | a[q].x);
      r.src = a[q].z; r.dst = a[q].w; r.seq = b[q].x; r.size = b[q].y; r.meta = b[q].z; r.corrupt_off = b[q].w;
      const uint32_t u = k.key((uint64_t)r.t, r.src, r.seq, (r.meta & TGSIM_F_CLONE) ? 0u : 1u);
      const uint32_t bk = u >> shift, e = cnt[bk];
      uint32_t y = bk ? cnt[bk - 1] : 0u, rank = y;
      for (; y < e; ++y) rank += slot[y] < u;
      p.put(b0 + rank, r);
    }
  }
  WHOLE_PH(6, __builtin_amdgcn_s_memrealtime());
  return true;
}

#ifdef TGSIM_PHASE_PROF
// debug builds: per task of the last task-parallel long-segment pass, {task | block << 32 | rank << 63,
// claimed, ready (chunk: sorted; rank: its chunks counted), done} in s_memrealtime ticks (100 MHz)
__device__ uint64_t g_task_ph[4096][4];
#endif

template <class P>
__device__ __forceinline__ void rest_body(const P& p, const uint32_t* keys, const uint32_t* vals, const uint32_t* off,
                                          const uint32_t* medium, const LargeSeg* large, const DevScalars* sc,
                                          uint64_t* K1a, uint64_t* K2a, uint32_t* K3a, uint64_t* K1b, uint64_t* K2b,
                                          uint32_t* K3b, uint32_t bid, uint32_t nblocks) {
  __shared__ SortSmem s;
  __shared__ uint32_t s_c1[kLargeTab + 1], s_c2[kLargeTab + 1];
  __shared__ uint32_t s_task, s_last;
  const uint32_t nm = sc->n_medium, nl = sc->n_large;
  const bool par = nl > 0 && nl <= kLargeTab && sc->max_large < (1u << 24);  // launch-uniform
  for (uint32_t w = bid; w < nm + (par ? 0u : nl); w += nblocks) {
    if (w < nm) {
      // one key, or a span of several (kMediumSpans): keys[a, a + m) are g .. g + nk - 1
      const uint32_t e = medium[w], g = e & kSpanKeyMask, nk = (e >> kSpanKeyShift) + 1u;
      const uint32_t a = off[g], m = off[g + nk] - a;
      load_span_keys(p, s, keys, vals, a, m, m);
      __syncthreads();
      span_sort(s, m, off, a);
      p.epilogue(s, m, a, off, w);
      count_long<P>(sc, m);
    } else {
      const LargeSeg L = large[w - nm];
      count_long<P>(sc, L.len);
      const bool in_a = large_sort_block(p, s, L, keys, vals, K1a, K2a, K3a, K1b, K2b, K3b);
      large_consume(p, s, L, in_a ? K1a : K1b, in_a ? K3a : K3b, (w - nm) * 131u);
    }
    __syncthreads();
  }
  if (!par) return;
  // task table: chunk tasks of segment i at [c1[i], c1[i + 1]), its rank tasks at T1 + [c2[i], c2[i + 1])
  // (measured: pinning a segment's tasks to the blocks of one XCD, so its chunks stay in that L2,
  // made the 10k inbox slower - 57 -> 70 us for the launch: a quarter of the chip's CUs per segment)
  {
    const uint32_t i = threadIdx.x;  // nl <= kLargeTab = kBlock
    uint32_t a = 0, b = 0, ta, tb;
    if (i < nl) {
      const uint32_t len = large[i].len;
      a = (len + kParChunk - 1) / kParChunk;
      b = (len + kRankTile - 1) / kRankTile;
    }
    block_scan2(a, b, s.perm, ta, tb);
    if (i < nl) { s_c1[i] = a; s_c2[i] = b; }
    if (i == 0) { s_c1[nl] = ta; s_c2[nl] = tb; }
    __syncthreads();
  }
  // whole tasks (WholeSort policies) first: task i < T0 is segment i's one-workgroup sort when it is
  // short enough, so the chunk tasks that wait for its verdict wait only on claimed tasks
  const uint32_t T0 = WholeSort<P>::v ? nl : 0u, T1 = T0 + s_c1[nl], T = T1 + s_c2[nl];
  LargeSeg* lg = const_cast<LargeSeg*>(large);
  uint32_t* ctr = const_cast<uint32_t*>(&sc->n_chunks);  // the launch's task counter (zeroed with the lists)
  for (;;) {
    __syncthreads();  // the previous task is done with LDS and s_task
    if (threadIdx.x == 0) s_task = atomicAdd(ctr, 1u);
    __syncthreads();
    // readfirstlane: the task is provably wave-uniform to the compiler, so every branch on it below
    // (and the barriers inside) stays uniform control flow
    const uint32_t task = __builtin_amdgcn_readfirstlane(s_task);
    if (task >= T) break;
    if (task < T0) {
      const LargeSeg L = large[task];
      if constexpr (WholeSort<P>::v) {
        if (L.len > kWholeMax) continue;
        if (whole_sort(p, s, L, vals, &lg[task].pad)) {
          count_long<P>(sc, L.len);
          if (threadIdx.x == 0) atomicAdd(const_cast<unsigned long long*>(&sc->kc[KC_WHOLE]), (unsigned long long)L.len);
        }
        else if (threadIdx.x == 0)  // it wrote nothing
          atomicOr(&lg[task].pad, kWholeBack);
      }
      continue;
    }
    const bool chunk = task < T1;
#ifdef TGSIM_PHASE_PROF
    const uint64_t tp_claim = __builtin_amdgcn_s_memrealtime();
#define TASK_PH(ready) do { if (threadIdx.x == 0 && task < 4096) { \
      g_task_ph[task][0] = task | ((uint64_t)blockIdx.x << 32) | (chunk ? 0ull : 1ull << 63); \
      g_task_ph[task][1] = tp_claim; g_task_ph[task][2] = (ready); \
      g_task_ph[task][3] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define TASK_PH(ready) do {} while (0)
#endif
    const uint32_t* tab = chunk ? s_c1 : s_c2;
    const uint32_t r = chunk ? task - T0 : task - T1;
    uint32_t i = 0, hi = nl;  // the segment: last i with tab[i] <= r
    while (hi - i > 1) {
      const uint32_t mid = (i + hi) >> 1;
      if (tab[mid] <= r) i = mid; else hi = mid;
    }
    const LargeSeg L = large[i];
    const uint32_t nch = s_c1[i + 1] - s_c1[i], nrk = s_c2[i + 1] - s_c2[i];
    const bool whole = WholeSort<P>::v && L.len <= kWholeMax;  // its verdict decides who sorts it
    if (chunk) {
      if (whole) {
        if (threadIdx.x == 0) {
          uint32_t spins = 0, v;
          while (!((v = __hip_atomic_fetch_add(&lg[i].pad, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) &
                   (kWholeDone | kWholeBack))) {
            __builtin_amdgcn_s_sleep(TGSIM_SPIN_SLEEP);
            if (++spins == (1u << 24)) {
              atomicOr(const_cast<uint32_t*>(&sc->err), ERR_TASKS);
              v = kWholeDone;
              break;
            }
          }
          s_last = v & kWholeDone;
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(s_last)) continue;  // sorted whole
      }
      if (r == s_c1[i]) count_long<P>(sc, L.len);  // the segment's first chunk task counts it
      large_chunk_sort(p, s, L, (r - s_c1[i]) * kParChunk, keys, vals, K1a, K2a, K3a, kParChunk);
#ifdef TGSIM_PHASE_PROF
      const uint64_t tp_sorted = __builtin_amdgcn_s_memrealtime();
#endif
      // the sorted chunk is visible device-wide before it is counted
      if (block_release_for_count()) atomicAdd(&lg[i].pad, 1u);
      TASK_PH(tp_sorted);
      continue;
    }
    if (threadIdx.x == 0) {
      // the count is read with an atomic read-modify-write: a plain (even atomic) load of coarse-
      // grained memory can keep hitting this XCD's L2 copy of the line while another XCD counts
      uint32_t spins = 0, v;
      while (((v = __hip_atomic_fetch_add(&lg[i].pad, 0u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) & 0xFFFFu) < nch &&
             !(whole && (v & kWholeDone))) {
        __builtin_amdgcn_s_sleep(TGSIM_SPIN_SLEEP);
        if (++spins == (1u << 24)) {  // a bound, never expected: report instead of hanging the device
          atomicOr(const_cast<uint32_t*>(&sc->err), ERR_TASKS);
          break;
        }
      }
      if (whole) s_last = v & kWholeDone;
    }
    block_acquire_after_poll();  // the counted chunks' keys, written by other workgroups
    if (whole && __builtin_amdgcn_readfirstlane(s_last)) continue;  // sorted whole
#ifdef TGSIM_PHASE_PROF
    const uint64_t tp_ready = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t e = (r - s_c2[i]) * kRankTile + threadIdx.x;
#ifndef TGSIM_RANK_PLAIN
    // a sampled index of the segment's sorted chunks in LDS (every st-th key of each chunk; the
    // chunks are complete, their tasks counted): a search first finds its st-key window among the
    // samples, then needs log2(st) dependent global loads instead of log2(kParChunk)
    uint32_t st = TGSIM_RANK_ST0;  // the densest sampling that fits the LDS arrays
    while (nch * (kParChunk / st) > (uint32_t)kSpan) st <<= 1;  // block-uniform
    const uint32_t S = kParChunk / st;  // samples of a full chunk
    for (uint32_t q = threadIdx.x; q < nch * S; q += kBlock) {
      const uint32_t pos = (q / S) * kParChunk + (q % S) * st;
      if (pos < L.len) { s.k1[q] = K1a[L.start + pos]; s.k2[q] = K2a[L.start + pos]; s.k3[q] = K3a[L.start + pos]; }
    }
    __syncthreads();
#endif
    if (e < L.len) {
      const uint32_t x = L.start + e, c = e / kParChunk;
      const uint64_t k1 = K1a[x], k2 = K2a[x];
      const uint32_t k3 = K3a[x];
      uint32_t rank = e - c * kParChunk;
      for (uint32_t c0 = 0; c0 < nch; c0 += kRankPar) {
        uint32_t b[kRankPar], n[kRankPar], lo[kRankPar], base[kRankPar];
#pragma unroll
        for (int q = 0; q < kRankPar; ++q) {
          const uint32_t cc = c0 + q;
          b[q] = L.start + cc * kParChunk;
          n[q] = (cc < nch && cc != c) ? min(kParChunk, L.len - cc * kParChunk) : 0u;
          base[q] = 0;
#ifndef TGSIM_RANK_PLAIN
          if (n[q]) {  // samples of chunk cc below the key: the count lies in ((m - 1) st, m st]
            const uint32_t ns = (n[q] + st - 1) / st, s0 = cc * S;
            uint32_t a = 0, z = ns;
            while (a < z) {
              const uint32_t mid = (a + z) >> 1;
              if (key_less(0, s.k1[s0 + mid], s.k2[s0 + mid], s.k3[s0 + mid], 0, k1, k2, k3)) a = mid + 1; else z = mid;
            }
            const uint32_t lo0 = a ? (a - 1) * st + 1 : 0u, hi0 = min(a * st, n[q]);
            base[q] = lo0;
            b[q] += lo0;
            n[q] = hi0 - lo0;
          }
#endif
        }
        below_n(K1a, K2a, K3a, b, n, k1, k2, k3, lo);
#pragma unroll
        for (int q = 0; q < kRankPar; ++q) rank += base[q] + lo[q];
      }
      large_place(p, L, rank, k1, k2, k3, K1b, K2b, K3b);
    }
    TASK_PH(tp_ready);
    if (LargeScan<P>::v) {  // compile-time: the segment's last rank task runs the scan
      // the placed keys are published by one release on the counting lane, and the last task
      // takes one acquire before it reads every task's placements (this was a
      // full fence in every thread on both sides)
      if (block_release_for_count()) s_last = (atomicAdd(&lg[i].pad, 1u << 16) >> 16) == nrk - 1;
      __syncthreads();
      if (__builtin_amdgcn_readfirstlane(s_last)) {
        block_acquire_after_poll();
        large_consume(p, s, L, K1b, K3b, i * 131u);
      }
      __syncthreads();
    }
  }
}

template <class P>
__global__ __launch_bounds__(kBlock) void k_rest(P p, const uint32_t* keys, const uint32_t* vals, const uint32_t* off,
                                                 const uint32_t* medium, const LargeSeg* large, const DevScalars* sc,
                                                 uint64_t* K1a, uint64_t* K2a, uint32_t* K3a, uint64_t* K1b,
                                                 uint64_t* K2b, uint32_t* K3b) {
  rest_body(p, keys, vals, off, medium, large, sc, K1a, K2a, K3a, K1b, K2b, K3b, blockIdx.x, gridDim.x);
}

// Window end, first pass of a single-shard context whose window ran the token bucket: k_rest<TB>
// (the senders with long runs) shares the launch with k_local_hist's partition of D and histogram of
// L, which read what it appends - a launch of its own cost ~4.5 us at the dependent-launch boundary
// even with nothing to do, which is nearly every window. sc->rest_tb (set by
// k_tb_bucket, constant in this launch) says whether it has work. If not, blocks [0, 2 kRadixBlocks)
// are the partition and histogram blocks, as in k_local_hist, and the kRestRoles blocks after them
// leave at once. If so, roles go by ticket: tickets [0, kRestRoles) run rest_body (the launch's two
// workgroups per CU all start as rest roles) and count themselves done after a release; a partition
// or histogram block (a later ticket) waits for all of them, so it only waits on roles that running
// workgroups hold, whatever the dispatch order. The ticket and the count have 128-B lines of their
// own, and a waiting block polls every ~8k clocks: polling every 128 clocks from every waiting block,
// on the line of the rest tasks' own counters, made the rest 2.2x slower (config 5 at two floods per
// wave).
#ifndef TG_REST_ROLES
#define TG_REST_ROLES 512
#endif
constexpr uint32_t kRestRoles = TG_REST_ROLES;
__global__ __launch_bounds__(kBlock) void k_rest_local_hist(TBPolicy p, const uint32_t* keys, const uint32_t* vals,
                                                            const uint32_t* off, const uint32_t* medium,
                                                            const LargeSeg* large, DevScalars* sc, uint64_t* K1a,
                                                            uint64_t* K2a, uint32_t* K3a, uint64_t* K1b, uint64_t* K2b,
                                                            uint32_t* K3b, BktSrc srcD, BktDiv bdD, uint32_t BD,
                                                            uint2* kv, uint32_t* poff, BktSrc srcL, BktDiv bdL,
                                                            uint32_t BL, uint32_t* hist, uint32_t* qc) {
  __shared__ uint32_t s_role;
  const bool busy = sc->rest_tb != 0u;  // launch-uniform: written by k_tb_bucket, read-only here
  if (blockIdx.x == 0 && threadIdx.x == 0) sc->rest_tb_last = busy ? 1u : 0u;
  uint32_t* ticket = qc + ((uint32_t)kQcRest << 5);
  uint32_t* done = qc + ((uint32_t)(kQcRest + 1) << 5);
  uint32_t role;  // [0, 2 kRadixBlocks): partition / histogram; above: rest
  if (busy) {
    if (threadIdx.x == 0) s_role = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t t = __builtin_amdgcn_readfirstlane(s_role);
    role = t < kRestRoles ? 2u * kRadixBlocks + t : t - kRestRoles;
  } else {
    role = blockIdx.x;
  }
  if (role >= 2u * kRadixBlocks) {
    if (!busy) return;
    rest_body(p, keys, vals, off, medium, large, sc, K1a, K2a, K3a, K1b, K2b, K3b, role - 2u * kRadixBlocks, kRestRoles);
    // its departures (D, L), token state and queue counts are visible device-wide before it counts
    if (block_release_for_count()) atomicAdd(done, 1u);
    return;
  }
  if (busy) {
    if (threadIdx.x == 0) {
      uint32_t spins = 0;
      while (__hip_atomic_fetch_add(done, 0u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < kRestRoles) {
        __builtin_amdgcn_s_sleep(127);
        if (++spins == (1u << 20)) {  // a bound, never expected: report instead of hanging the device
          atomicOr(&sc->err, ERR_TASKS);
          break;
        }
      }
    }
    block_acquire_after_poll();
  }
  if (role < (uint32_t)kRadixBlocks) bkt_local_body(srcD, sc, bdD, BD, kv, poff, role);
  else bkt_hist_body(srcL, sc, bdL, BL, hist, role - kRadixBlocks);
}

// Window end, last pass: the wheel insert (blocks [0, kRadixBlocks)) and the deliveries' long
// inboxes (k_rest<Emit>, the other blocks) are independent after k_emit_bucket, so they share one
// launch: a launch that finds nothing to do still costs ~4.5 us at a dependent-launch boundary
// (DESIGN.md 5). The scatter runs one workgroup per CU, so rest_body's LDS costs it no occupancy;
// the storm generator's blocks beside it do lose some (two workgroups per CU: a build without the
// long-inbox role measured 22.4 against 25.3 us for k_wheel_scatter_gen, less than a launch's ~4.5).
__global__ __launch_bounds__(kBlock) void k_wheel_scatter(BktSrc src, DevScalars* sc, const tgsim_record* L,
                                                          tgsim_record* arena, uint32_t* dirs, uint32_t slots,
                                                          const uint32_t* hist, const uint32_t* tot, PendRef pend,
                                                          uint32_t lo, uint32_t nloc, EmitPolicy p,
                                                          const uint32_t* keys, const uint32_t* vals,
                                                          const uint32_t* off, const uint32_t* medium,
                                                          const LargeSeg* large, uint64_t* K1a, uint64_t* K2a,
                                                          uint32_t* K3a, uint64_t* K1b, uint64_t* K2b, uint32_t* K3b) {
  static_assert(kRadixBlocks == kBlock, "slot rows are scanned by one kBlock workgroup each");
  if (blockIdx.x < (uint32_t)kRadixBlocks)
    wheel_scatter_body(src, sc, L, arena, dirs, slots, hist, tot, pend, lo, nloc);
  else
    rest_body(p, keys, vals, off, medium, large, sc, K1a, K2a, K3a, K1b, K2b, K3b, blockIdx.x - kRadixBlocks,
              gridDim.x - kRadixBlocks);
}

// The same split over two streams (Dev::side): the wheel insert alone on the side
// stream - nothing after the window reads the wheel before the next window starts - and the long
// inboxes with the counters' close on the context stream, where the reactions that read the
// deliveries follow at once.
__global__ __launch_bounds__(kBlock) void k_wheel_insert(BktSrc src, DevScalars* sc, const tgsim_record* L,
                                                         tgsim_record* arena, uint32_t* dirs, uint32_t slots,
                                                         const uint32_t* hist, const uint32_t* tot, PendRef pend,
                                                         uint32_t lo, uint32_t nloc) {
  wheel_scatter_body(src, sc, L, arena, dirs, slots, hist, tot, pend, lo, nloc, false);
}
__global__ __launch_bounds__(kBlock) void k_inbox_rest(DevScalars* sc, EmitPolicy p, const uint32_t* keys,
                                                       const uint32_t* vals, const uint32_t* off,
                                                       const uint32_t* medium, const LargeSeg* large, uint64_t* K1a,
                                                       uint64_t* K2a, uint32_t* K3a, uint64_t* K1b, uint64_t* K2b,
                                                       uint32_t* K3b) {
  if (blockIdx.x == 0 && threadIdx.x == 0) close_window_counters(sc);
  rest_body(p, keys, vals, off, medium, large, sc, K1a, K2a, K3a, K1b, K2b, K3b, blockIdx.x, gridDim.x);
}

// ============================================================================================
// exchange (sharded runs)
// ============================================================================================

// Peer p's header: the count of each slice in the record's eight 32-bit words (one slice: t = count)
__global__ void k_xheaders(tgsim_record* xsend, uint32_t S, uint32_t xcap, const uint32_t* qc) {
  const uint32_t p = threadIdx.x;
  if (p >= S) return;
  const uint32_t G = x_slices(xcap), cs = x_slice_cap(xcap);
  uint32_t w[8];
#pragma unroll
  for (uint32_t g = 0; g < 8; ++g) w[g] = g < G ? min(qc[(3u * kNSub + p * kXSlices + g) << 5], cs) : 0u;
  uint4* h = reinterpret_cast<uint4*>(xsend + (size_t)p * xcap);
  h[0] = make_uint4(w[0], w[1], w[2], w[3]);
  h[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// Receive: every exchanged record is due this window (only due records cross shards) and joins the
// deliveries. Send side: a wheel copy the extraction sent to a peer leaves its sender's queue.
// `split` blocks per (peer, slice), about two slots of the slice's capacity per thread, walk only the
// slice's counted records (the header's words) - the capacity slots past the count are not touched.
__host__ __device__ inline uint32_t recv_split(uint32_t xcap) {
  const uint32_t cs = x_slice_cap(xcap);
  return cs > 2u * kBlock ? (cs + 2u * kBlock - 1u) / (2u * kBlock) : 1u;
}
__global__ __launch_bounds__(kBlock) void k_recv(const tgsim_record* xrecv, const tgsim_record* xsend, uint32_t S,
                                                 uint32_t shard, uint32_t xcap, Queues Q, PendRef pend,
                                                 uint32_t lo, uint32_t nloc) {
  const int64_t t_end = Q.sc->t_end;
  const uint32_t G = x_slices(xcap), cs = x_slice_cap(xcap), split = recv_split(xcap);
  const uint32_t b = blockIdx.x / split, part = blockIdx.x % split;
  const uint32_t p = b / G, g = b % G;  // block-uniform
  if (p >= S || p == shard) return;
  const size_t h = (size_t)p * xcap;
  // the slice's counts: a header word (G > 1), or the whole t (one slice); out of range: corrupt
  const int64_t nr = G > 1 ? (int64_t)reinterpret_cast<const uint32_t*>(xrecv + h)[g] : xrecv[h].t;
  const int64_t ns = G > 1 ? (int64_t)reinterpret_cast<const uint32_t*>(xsend + h)[g] : xsend[h].t;
  const bool okr = nr >= 0 && nr <= (int64_t)cs, oks = ns > 0 && ns <= (int64_t)cs;
  if (!okr && part == 0 && threadIdx.x == 0) atomicOr(&Q.sc->err, ERR_EXCH_HDR);
  const uint32_t cr = okr ? (uint32_t)nr : 0u, cn = oks ? (uint32_t)ns : 0u;
  const uint32_t top = cr > cn ? cr : cn;
  const size_t base = h + 1 + (size_t)g * cs;
  uint32_t it = 0;
  for (uint32_t o0 = part * kBlock; o0 < top; o0 += kBlock * split, ++it) {  // block-uniform trip count
    const uint32_t o = o0 + threadIdx.x;
    int q = -1;
    tgsim_record rec;
    if (o < cr) {
      load_rec(xrecv + base + o, rec);
      rec.meta &= ~(uint32_t)TGSIM_F_WHEEL;
      if (rec.t < t_end) q = Q_D;
      else atomicOr(&Q.sc->err, ERR_EXCH_HDR);
    }
    if (o < cn) {
      const uint4 bb = reinterpret_cast<const uint4*>(xsend + base + o)[1];
      if (bb.z & TGSIM_F_WHEEL) {
        const uint32_t src = reinterpret_cast<const uint4*>(xsend + base + o)[0].z;
        if (src - lo < nloc) atomicSub(&pend[src - lo], 1u);
      }
    }
    Q.push(q, rec, it);
  }
}

// ============================================================================================
// workload generator: gossip storm round
// ============================================================================================

struct StormArgs {
  uint32_t lo, nloc, N, round;
  int64_t t0;
  uint32_t F, Fp, fp_log2, size;
  uint32_t peer_m, peer_sh1, peer_sh2;  // u % (N - 1) by 32-bit multiply-shift (exact for every u32)
  int64_t spread;
  SlotDiv spread_div;        // u % spread by multiply-shift (tgsim_slotdiv.h, exact for every u)
  uint32_t key0, key1, base;
  uint32_t* m_src;
  uint32_t* m_dst;
  uint32_t* m_seq;
  uint32_t* m_size;
  int64_t* m_t;
};

// u mod d for the launch-invariant divisor d = a.spread > 0 (slot_div; its constants from the host).
__device__ __forceinline__ uint64_t spread_mod(const StormArgs& a, uint64_t u) {
  return u - slot_div(a.spread_div, u) * (uint64_t)a.spread;
}

// The peer draw out[0] % (N - 1), the same construction at 32 bits (no emulated integer division).
__device__ __forceinline__ uint32_t peer_mod(const StormArgs& a, uint32_t u) {
  const uint32_t t = __umulhi(a.peer_m, u);
  const uint32_t q = (t + ((u - t) >> a.peer_sh1)) >> a.peer_sh2;
  return u - q * (a.N - 1);
}

// One storm round: every instance sends F messages to F distinct random peers and signals `state`
// at its latest send time. A group of Fp (power of two >= F) lanes per instance, one message per
// lane. Peer k is the first Philox draw of (g, round, k) unless it repeats one of the k earlier
// peers, then further attempts (ctr word 2 = k << 16 | attempt) - the serial restatement
// tgo_gen_storm_round. All first draws are checked with F shuffles; only a wave holding a group that
// drew a repeat (probability ~F^2/2N per group) walks the group lane by lane, each lane redrawing
// against the final peers of the lanes before it. Stores are coalesced (message l*F + k at lane
// l*Fp + k). The signals are reduced to per-block partials in the same launch (k_sig_commit
// finishes them).
// FIX != 0: fanout FIX = its power of two, known at compile time (the shuffle loops unroll); 0: any.
template <uint32_t FIX>
__device__ __forceinline__ void gen_storm_body(const StormArgs& a, const SigState& sg, uint32_t bid, uint32_t nb) {
  const uint32_t F = FIX ? FIX : a.F, Fp = FIX ? FIX : a.Fp, fp_log2 = FIX ? (uint32_t)__builtin_ctz(FIX ? FIX : 1u) : a.fp_log2;
  const int64_t t0 = a.t0 == INT64_MIN ? sg.sc->t_end : a.t0;  // TGSIM_T_NOW: the device's window start
  const uint32_t total = a.nloc * Fp;
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (uint32_t b0 = bid * kBlock; b0 < total; b0 += nb * kBlock) {  // block-uniform loop
    const uint32_t tid = b0 + threadIdx.x;
    const uint32_t l = tid >> fp_log2, k = tid & (Fp - 1u);
    const uint32_t lane = lane_id(), gbase = lane - k;
    const bool inst = l < a.nloc, msg = inst && k < F;
    const uint32_t g = a.lo + l;
    uint32_t p = 0xFFFFFFFFu;
    int64_t t = t0;
    if (msg) {
      uint32_t out[4];
      philox4x32_10(g, a.round, k << 16, kStormSalt, a.key0, a.key1, out);
      const uint64_t u = ((uint64_t)out[2] << 32) | out[1];
      t = t0 + (a.spread > 0 ? (int64_t)spread_mod(a, u) : 0);
      p = peer_mod(a, out[0]);
      if (p >= g) ++p;
    }
    bool dup = false;
    for (uint32_t j = 0; j + 1 < F; ++j) {  // lane k compares its draw with lanes j < k of its group
      const uint32_t q = __shfl(p, (int)(gbase + j));
      dup |= msg && j < k && q == p;
    }
    if (__ballot(dup)) {  // wave-uniform, rare: lanes k = 1 .. F-1 in turn settle against lanes j < k
      uint32_t attempt = 0;
      for (uint32_t kk = 1; kk < F; ++kk) {
        for (;;) {
          bool again = false;
          for (uint32_t j = 0; j < kk; ++j) {
            const uint32_t q = __shfl(p, (int)(gbase + j));
            again |= msg && k == kk && q == p;
          }
          if (!__ballot(again)) break;
          if (again) {
            uint32_t out[4];
            philox4x32_10(g, a.round, (k << 16) | ++attempt, kStormSalt, a.key0, a.key1, out);
            p = peer_mod(a, out[0]);
            if (p >= g) ++p;
          }
        }
      }
    }
    if (msg) {
      const uint32_t i = a.base + l * F + k;
      stn(a.m_src + i, g); stn(a.m_dst + i, p); stn(a.m_seq + i, a.round * F + k); stn(a.m_size + i, a.size);
      stn(a.m_t + i, t);
    }
    // the instance's signal time: its latest send
    for (uint32_t o = Fp >> 1; o > 0; o >>= 1) {
      const int64_t v = __shfl_xor(t, (int)o);
      t = v > t ? v : t;
    }
    if (inst && k == 0) { mn = t < mn ? t : mn; mx = t > mx ? t : mx; }
  }
  sig_block_partial(sg, mn, mx, bid);
}

template <uint32_t FIX>
__global__ __launch_bounds__(kBlock) void k_gen_storm(StormArgs a, SigState sg) {
  gen_storm_body<FIX>(a, sg, blockIdx.x, gridDim.x);
}

// The wheel insert of window r with the storm round r + 1 generated speculatively beside it
// (DESIGN.md 5): blocks [0, kRadixBlocks) scatter, then g generator blocks, then the long inboxes.
// The scatter streams records while the generator is bound by integer multiplies, so they overlap
// on the same CUs; the generator writes only the staged arrays (consumed by this window's netem
// pass) and the signal partials (consumed by this window's start).
__global__ __launch_bounds__(kBlock) void k_wheel_scatter_gen(BktSrc src, DevScalars* sc, const tgsim_record* L,
                                                              tgsim_record* arena, uint32_t* dirs, uint32_t slots,
                                                              const uint32_t* hist, const uint32_t* tot, PendRef pend,
                                                              uint32_t lo, uint32_t nloc, EmitPolicy p,
                                                              const uint32_t* keys, const uint32_t* vals,
                                                              const uint32_t* off, const uint32_t* medium,
                                                              const LargeSeg* large, uint64_t* K1a, uint64_t* K2a,
                                                              uint32_t* K3a, uint64_t* K1b, uint64_t* K2b, uint32_t* K3b,
                                                              StormArgs ga, SigState sg, uint32_t g) {
  if (blockIdx.x < (uint32_t)kRadixBlocks)
    wheel_scatter_body(src, sc, L, arena, dirs, slots, hist, tot, pend, lo, nloc);
  else if (blockIdx.x < (uint32_t)kRadixBlocks + g)
    gen_storm_body<8>(ga, sg, blockIdx.x - kRadixBlocks, g);
  else
    rest_body(p, keys, vals, off, medium, large, sc, K1a, K2a, K3a, K1b, K2b, K3b, blockIdx.x - kRadixBlocks - g,
              gridDim.x - kRadixBlocks - g);
}

// ============================================================================================
// host-side pipeline drivers
// ============================================================================================

#define TG_CHECK(x)                    \
  do {                                 \
    hipError_t e__ = (x);              \
    if (e__ != hipSuccess) return e__; \
  } while (0)

static inline unsigned grid_for(uint64_t n);
static inline int bits_for(uint32_t K) { return K <= 1 ? 0 : 32 - __builtin_clz(K - 1); }

hipError_t sync_scalars(Dev& d) {
  TG_CHECK(hipMemcpyAsync(d.h_sc, d.sc, sizeof(DevScalars), hipMemcpyDeviceToHost, d.stream));
  TG_CHECK(hipStreamSynchronize(d.stream));
  if (!d.prof.pending.empty()) prof_resolve(d);
  return hipSuccess;
}

SigState sig_state(Dev& d) {
  SigState g;
  g.count = d.st_count; g.last = d.st_last; g.nchunks = d.st_nchunks; g.chunks = d.st_chunks; g.log = d.sig_log;
  g.w_state = d.w_state; g.w_target = d.w_target; g.w_twait = d.w_twait; g.w_release = d.w_release;
  g.red = d.sig_red; g.part = d.sig_part; g.sc = d.sc;
  return g;
}

static WindowArgs window_args(Dev& d, int mode, int64_t t_end, const int64_t* src, int64_t offset) {
  WindowArgs a;
  a.sc = d.sc; a.qc = d.qc; a.mode = mode; a.t_end_arg = t_end; a.src = src; a.offset = offset;
  a.slot_ns = d.slot_ns; a.regions = d.regions; a.dirs = d.dirs; a.slots = d.slots; a.plan_start = d.plan_start;
  a.plan_off = d.plan_off;
  return a;
}

static hipError_t window_start(Dev& d, int mode, int64_t t_end, const int64_t* src, int64_t offset) {
  hipLaunchKernelGGL(k_window_start, dim3(1), dim3(kBlock), 0, d.stream, window_args(d, mode, t_end, src, offset));
  return hipGetLastError();
}

hipError_t launch_set_window(Dev& d, int64_t t_end) { return window_start(d, WIN_EXPLICIT, t_end, nullptr, 0); }

hipError_t launch_set_window_barrier(Dev& d, uint32_t waiter, int64_t offset_ns) {
  return window_start(d, WIN_BARRIER, 0, d.w_release + waiter, offset_ns);
}

SigState sig_state(Dev& d);
static WaiterAdd waiter_add(Dev& d, bool add, uint32_t state, uint32_t target, int64_t t_wait) {
  WaiterAdd wa;
  wa.w_state = d.w_state; wa.w_target = d.w_target; wa.w_twait = d.w_twait;
  wa.state = state; wa.target = target; wa.t_wait = t_wait; wa.on = add ? 1u : 0u;
  return wa;
}

hipError_t launch_set_window_barrier_commit(Dev& d, uint32_t waiter, int64_t offset_ns, uint32_t nparts, uint32_t n,
                                            uint32_t st, uint32_t nw, bool add, uint32_t add_state,
                                            uint32_t add_target, int64_t add_twait) {
  hipLaunchKernelGGL(k_window_start_commit, dim3(1), dim3(kBlock), 0, d.stream, sig_state(d), nparts, n, st, nw,
                     waiter_add(d, add, add_state, add_target, add_twait),
                     window_args(d, WIN_BARRIER, 0, d.w_release + waiter, offset_ns));
  return hipGetLastError();
}

hipError_t launch_set_window_dev(Dev& d, const int64_t* t_end_dev, int64_t offset_ns) {
  return window_start(d, WIN_DEVICE, 0, t_end_dev, offset_ns);
}

hipError_t launch_reset_tb(Dev& d, const uint32_t* locals_dev, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_reset_tb, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, d.stream, d.X, locals_dev, n);
  return hipGetLastError();
}

static inline unsigned grid_for(uint64_t n) {
  uint64_t g = (n + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > (uint64_t)kStreamBlocks) g = kStreamBlocks;
  return (unsigned)g;
}

static uint32_t bkt_width_fused(const Dev& d, uint32_t K);
static Queues make_queues(Dev& d) {
  Queues Q;
  Q.sc = d.sc; Q.qc = d.qc; Q.xq = d.qc + ((size_t)(3 * kNSub) << 5); Q.xg = x_slices(d.xcap); Q.xcs = x_slice_cap(d.xcap); Q.A = d.A; Q.D = d.D; Q.L = d.L; Q.X = d.xsend; Q.subcap = d.subcap; Q.xcap = d.xcap;
  Q.KA = d.KA; Q.KD = d.KD; Q.KL = d.KL; Q.lo = d.lo; Q.slots = d.slots; Q.slot_ns = d.slot_ns; Q.sdiv = d.slot_div;
  // the fused consumers' buckets (bkt_width_fused over the local keys) in xcd_major order: XCD x
  // runs buckets [x q + min(x, r), (x+1) q + min(x+1, r)) with q = B / 8, r = B % 8
  const uint32_t w = bkt_width_fused(d, d.nloc), B = (d.nloc + w - 1) / w, q8 = B >> 3, r8 = B & 7u;
  for (uint32_t j = 1; j < 8; ++j) Q.gb[j - 1] = (j * q8 + std::min(j, r8)) * w;
  return Q;
}

// Bucket shift: <= 2048 buckets of <= 2^kBktMaxKeyBits keys, 128 keys per bucket where possible.
// fine: as few keys per bucket as 2048 buckets allow (one per key when K <= 2048) - for batches with
// many items per key (the deferred messages of queue-heavy senders: 1000 senders x 999 messages in
// eight 128-key buckets took 221 us per group-by in one workgroup per bucket).
static int bkt_shift(uint32_t K, bool fine = false) {
  const int bits = bits_for(K);
  return std::max(bits - kMaxDigitBits, fine ? 0 : std::min(7, bits));
}

static BktDiv bkt_div(uint32_t w) {
  BktDiv b;
  b.w = w;
  b.m = ((1ull << 32) + w - 1) / w;
  return b;
}

// Keys per bucket of the fused consumers: few enough buckets that they all run in one wave of
// workgroups (TG_BKT_WGS_PER_CU per CU: ~98 keys, ~780 items of a storm per workgroup); <= 512
// keys; at least TG_BKT_MIN_KEYS (24 with four workgroups per CU: 12.5k-instance shards -6 %, 25k -3 %,
// 50k and 100k unchanged; 48 was best with three per CU).
static uint32_t bkt_width_fused(const Dev& d, uint32_t K) {
#ifndef TG_BKT_MIN_KEYS
#define TG_BKT_MIN_KEYS 24u  // small shards (strong scaling): more, smaller buckets
#endif
  // a context whose windows carry bkt_load times the packets per key (TCP acks: an ACK per data
  // packet) splits its keys over as many more buckets, so a bucket still fits kBktCap items
  const uint32_t slots = (uint32_t)TG_BKT_WGS_PER_CU * (uint32_t)d.n_cu * d.bkt_load;
  // No floor when one key per bucket fits the wave of workgroups (K <= slots): a 1000-instance
  // context (config 2) at 24 keys per bucket made 42 buckets of up to ~11k deliveries (its receivers
  // get up to ~480 each in a window), every one over kBktCap, so all its deliveries took the global
  // form and k_rest's medium segments (a floor of K / (4 n_cu) measured the same on config 2 and
  // slower on config 3's 10k instances)
  const uint32_t floor_keys = K <= slots ? 1u : std::min<uint32_t>(TG_BKT_MIN_KEYS, K);
  uint32_t w = std::max<uint32_t>((K + slots - 1) / slots, floor_keys);
  w = std::min<uint32_t>(w, 1u << kBktFusedKeyBits);
  // never more than kMaxBins buckets (the partition's LDS histograms and d.poff rows are that wide)
  w = std::max<uint32_t>(w, (K + kMaxBins - 1) / kMaxBins);
  return std::max<uint32_t>(w, 1u);
}

// Passes 1-2 of the bucketed group-by: (keys1, vals1) in bucket order, bucket totals in d.tot; with
// g.on (one key per bucket) that is the final grouping, and the scatter writes the key offsets too.
static hipError_t bkt_partition(Dev& d, const BktSrc& src, BktDiv bd, uint32_t B, const BktDirect& g = BktDirect()) {
  {
    ProfScope ps_(d, KID_BKT_HIST);
    hipLaunchKernelGGL(k_bkt_hist, dim3(kRadixBlocks), dim3(kBlock), 0, d.stream, src, d.sc, bd, B, d.hist);
  }
  {
    ProfScope ps_(d, KID_RADIX_ROWS);
    hipLaunchKernelGGL(k_radix_rows, dim3(B), dim3(kRadixBlocks), 0, d.stream, src, d.hist, d.histx, d.tot, B);
  }
  {
    ProfScope ps_(d, KID_BKT_SCATTER);
    hipLaunchKernelGGL(k_bkt_scatter, dim3(kRadixBlocks), dim3(kBlock), 0, d.stream, src, d.keys1, d.vals1, bd, B,
                       d.histx, d.tot, d.bstart, g);
  }
  return hipGetLastError();
}

// Partition for the fused consumers: (keys1, vals1) chunked per partition block, offsets in d.poff.
static hipError_t bkt_local(Dev& d, const BktSrc& src, BktDiv bd, uint32_t B) {
  ProfScope ps_(d, KID_BKT_SCATTER);
  hipLaunchKernelGGL(k_bkt_local, dim3(kRadixBlocks), dim3(kBlock), 0, d.stream, src, d.sc, bd, B, d.kv1, d.poff);
  return hipGetLastError();
}

// Group a batch by key (unstable; see k_bkt_hist): results in *keys / *vals ((d.keys0, d.vals0), or
// (d.keys1, d.vals1) for one key per bucket), segment offsets in
// d.seg_off (and off2), medium / large lists in d.medium / d.large. K <= 2^24 (checked at create).
static hipError_t group_by_bkt(Dev& d, const BktSrc& src, uint32_t K, uint32_t medium_above, uint32_t* off2,
                               uint32_t** keys, uint32_t** vals, bool fine = false, uint32_t* vals_copy = nullptr) {
  const int bs = bkt_shift(K, fine);
  if (bs > kBktMaxKeyBits) return hipErrorInvalidValue;
  const uint32_t B = (K + (1u << bs) - 1) >> bs;
  const BktDiv bd = bkt_div(1u << bs);
  if (bs == 0) {  // one key per bucket: the scatter writes the groups and the offsets (no pass 3);
    // the result stays in (keys1, vals1) - the source may be (keys0, vals0) (k_keys_corr's output)
    *keys = d.keys1;
    *vals = d.vals1;
    BktDirect g;
    g.on = 1; g.off = d.seg_off; g.off2 = off2; g.vout2 = vals_copy; g.medium = d.medium; g.large = d.large;
    g.sc = d.sc; g.medium_above = medium_above;
    return bkt_partition(d, src, bd, B, g);
  }
  TG_CHECK(bkt_partition(d, src, bd, B));
  {
    ProfScope ps_(d, KID_BKT_SORT);
    hipLaunchKernelGGL(k_bkt_sort, dim3(B), dim3(kBlock), 0, d.stream, d.keys1, d.vals1, d.keys0, d.vals0, bd, B, K,
                       d.tot, d.seg_off, off2, medium_above, d.medium, d.large, d.sc, vals_copy);
  }
  *keys = d.keys0;
  *vals = d.vals0;
  return hipGetLastError();
}

static BktSrc bkt_queue(Dev& d, int q) {
  BktSrc s;
  s.keys = q == Q_A ? d.KA : (q == Q_D ? d.KD : d.KL);
  s.vals = nullptr; s.qc = d.qc; s.q = q; s.mode = q; s.subcap = d.subcap; s.n_ptr = nullptr; s.cap = d.cap_rec;
  s.regions = d.regions; s.cap_arena = d.cap_arena; s.slot_ns = d.slot_ns;
  return s;
}

template <class P>
static hipError_t launch_rest(Dev& d, const P& p, const uint32_t* keys, const uint32_t* vals) {
  ProfScope ps_(d, KID_SEG_REST);
  hipLaunchKernelGGL(k_rest<P>, dim3(kListBlocks), dim3(kBlock), 0, d.stream, p, keys, vals, d.seg_off, d.medium,
                     d.large, d.sc, d.K1a, d.K2a, d.K3a, d.K1b, d.K2b, d.K3b);
  return hipGetLastError();
}

// Token bucket: partition the due copies by sender bucket, then one workgroup per bucket groups
// and runs the GCRA in LDS (k_tb_bucket); long senders finish in k_rest.
static TBPolicy tb_policy(Dev& d) {
  TBPolicy p;
  p.A = d.A; p.shape = d.tbs; p.X = d.X; p.pend = pend_ref(d); p.lo = d.lo; p.geo = make_geo(d); p.Q = make_queues(d);
  p.sc = d.sc;
  return p;
}

static hipError_t run_token_bucket(Dev& d) {
  const TBPolicy p = tb_policy(d);
  const BktDiv bd = bkt_div(bkt_width_fused(d, d.nloc));
  const uint32_t B = (d.nloc + bd.w - 1) / bd.w;  // <= kMaxBins (bkt_width_fused)
  if (B > (uint32_t)kMaxBins) return hipErrorInvalidValue;
  const BktSrc src = bkt_queue(d, Q_A);
  TG_CHECK(bkt_local(d, src, bd, B));
  {
    ProfScope ps_(d, KID_TB);
    hipLaunchKernelGGL(k_tb_bucket, dim3(B), dim3(kBlock), 0, d.stream, p, src, d.poff, d.kv1, d.keys2,
                       d.vals2, d.keys0, d.vals0, bd, B, d.nloc, d.seg_off, d.medium, d.large, d.sc);
  }
  TG_CHECK(hipGetLastError());
#ifndef TGSIM_REST_OWN_LAUNCH  // experiment build: k_rest<TB> in a launch of its own (the round-5 form)
  // nothing reads its outputs before the window end's first launch, which then runs it - unless the
  // last window the host saw (a sync point) had long senders: a busy k_rest<TB> runs faster in a launch
  // of its own (config 5 at two floods per wave: 1.07 against 1.13 ms per window), and such windows
  // come in runs (the hint only picks the launch; both forms give the same results)
  if (d.S == 1 && !d.h_sc->rest_tb_last) {
    d.tb_rest_owed = true;
    return hipSuccess;
  }
#endif
  return launch_rest(d, p, d.keys0, d.vals0);  // sharded: the exchange headers read its copies
}


// k_shape_seq_wide's grid: one workgroup per CU (its 16 waves at <= 128 VGPRs fill the CU), each
// walking its senders one ahead (the next sender's loads in flight); a workgroup per sender left
// every first sender's loads exposed
static uint32_t wide_grid(const Dev& d) {
  return std::min<uint32_t>(std::max<uint32_t>(d.nloc, 1u), (uint32_t)std::max(d.n_cu, 1));
}

// The deferred messages (k_shape: correlated or queue-heavy senders): group by sender, order
// (t_send, seq); the heavy senders' due wheel records (H) grouped by sender; then k_shape_seq.
static hipError_t run_shape_seq(Dev& d, const ShapeArgs& a, uint32_t n_staged) {
  uint32_t* n_dev = &d.sc->n_corr;
  const uint32_t gk = (grid_for(n_staged) + kDeferSub - 1) / kDeferSub * kDeferSub;  // whole sub-list rows
  hipLaunchKernelGGL(k_keys_corr, dim3(gk), dim3(kBlock), 0, d.stream, d.corr_idx,
                     a.heavy.pend ? 1u : 0u, d.qc, a.n_dev, n_staged, d.m_src, n_dev, d.lo, d.keys0, d.vals0, &d.sc->kc[KC_DEFERRED], &d.sc->seq_left, a.heavy.pend ? 0u : 1u);
  TG_CHECK(hipGetLastError());
  BktSrc src = bkt_queue(d, Q_A);
  src.keys = d.keys0; src.vals = d.vals0; src.qc = nullptr; src.mode = 3; src.n_ptr = n_dev;
  uint32_t *keys, *vals;
  CorrPolicy p;
  p.t = d.m_t; p.seq = d.m_seq; p.sorted = d.corr_sorted;
  BktSrc hs = bkt_queue(d, Q_A);
  hs.keys = d.hkeys; hs.vals = d.hvals; hs.qc = nullptr; hs.mode = 3; hs.n_ptr = &d.sc->n_hrec; hs.cap = d.h_cap;
  if (a.heavy.pend && bits_for(d.nloc) <= kMaxDigitBits) {
    // both group-bys one key per bucket: their passes share three launches; the deferred messages'
    // values also go to corr_sorted (k_shape_seq_wide orders each sender there in place), the H
    // list's groups to its own arrays
    BktPass pc, ph;
    pc.src = src; pc.bd = bkt_div(1); pc.B = d.nloc; pc.hist = d.hist; pc.histx = d.histx; pc.tot = d.tot;
    pc.bstart = d.bstart; pc.kout = d.keys1; pc.vout = d.vals1;
    pc.g.on = 1; pc.g.off = d.seg_off; pc.g.off2 = d.moff; pc.g.vout2 = d.corr_sorted; pc.g.medium = d.medium;
    pc.g.large = d.large; pc.g.sc = d.sc; pc.g.medium_above = kNoMedium;
    ph.src = hs; ph.bd = pc.bd; ph.B = d.nloc; ph.hist = d.hhist; ph.histx = d.hhistx; ph.tot = d.htot;
    ph.bstart = d.hbstart; ph.kout = d.hkeys1; ph.vout = d.hvals1;
    ph.g.on = 1; ph.g.off = d.hoff; ph.g.sc = d.sc; ph.g.lists = 0;
    {
      ProfScope ps_(d, KID_BKT_HIST);
      hipLaunchKernelGGL(k_bkt_hist_pair, dim3(2 * kRadixBlocks), dim3(kBlock), 0, d.stream, pc, ph, d.sc);
    }
    {
      ProfScope ps_(d, KID_RADIX_ROWS);
      hipLaunchKernelGGL(k_radix_rows_pair, dim3(2 * d.nloc), dim3(kRadixBlocks), 0, d.stream, pc, ph);
    }
    {
      ProfScope ps_(d, KID_BKT_SCATTER);
      hipLaunchKernelGGL(k_bkt_scatter_pair, dim3(2 * kRadixBlocks), dim3(kBlock), 0, d.stream, pc, ph);
    }
    TG_CHECK(hipGetLastError());
    TG_CHECK(launch_rest(d, p, d.keys1, d.vals1));
    const unsigned g = (unsigned)std::min<uint32_t>(std::max<uint32_t>(d.nloc, 1u), 4096u);
    {
      ProfScope ps_(d, KID_SHAPE_WIDE);
      hipLaunchKernelGGL(k_shape_seq_wide, dim3(wide_grid(d)), dim3(kWide), 0, d.stream, a, d.corr_sorted, d.corr_sorted,
                         d.moff, d.hoff, d.hvals1, d.H, d.seq_done);
    }
    ProfScope ps_(d, KID_SHAPE_SEQ);
    hipLaunchKernelGGL(k_shape_seq, dim3(g), dim3(kSeqChunk), 0, d.stream, a, d.corr_sorted, d.moff, d.hoff, d.hvals1,
                       d.H, d.cor_rho, d.cor_last, d.X, d.seq_done);
    return hipGetLastError();
  }
  // with queue tracking the grouped values also go to corr_sorted, where k_shape_seq_wide orders each
  // sender of <= kTile messages in place (the H group-by below reuses the group-by's output arrays)
  TG_CHECK(group_by_bkt(d, src, d.nloc, kNoMedium, d.moff, &keys, &vals, true,
                        a.heavy.pend ? d.corr_sorted : nullptr));
  if (!a.heavy.pend) {
    ProfScope ps_(d, KID_SEG_SMALL);  // each sender's deferred messages in (t_send, seq) order
    hipLaunchKernelGGL(k_seg_small<CorrPolicy>, dim3(kStreamBlocks), dim3(kBlock), 0, d.stream, p, keys, vals,
                       d.seg_off, n_dev, d.cap_rec);
  }
  TG_CHECK(hipGetLastError());
  TG_CHECK(launch_rest(d, p, keys, vals));
  const uint32_t* hoff = nullptr;
  const uint32_t* hidx = nullptr;
  if (a.heavy.pend) {
    uint32_t *hk, *hv;
    TG_CHECK(group_by_bkt(d, hs, d.nloc, kNoMedium, nullptr, &hk, &hv, true));
    hoff = d.seg_off;
    hidx = hv;
  }
  const unsigned g = (unsigned)std::min<uint32_t>(std::max<uint32_t>(d.nloc, 1u), 4096u);
  // k_shape_seq skips its launch's work when the closed form left it no sender (seq_left 0, set by
  // k_keys_corr above)
  if (a.heavy.pend) {  // the whole-sender closed form first (heavy senders without HTB / correlation)
    ProfScope ps_(d, KID_SHAPE_WIDE);
    hipLaunchKernelGGL(k_shape_seq_wide, dim3(wide_grid(d)), dim3(kWide), 0, d.stream, a, d.corr_sorted, d.corr_sorted,
                       d.moff, hoff, hidx, d.H, d.seq_done);
  } else {
    TG_CHECK(hipMemsetAsync(d.seq_done, 0, std::max<uint32_t>(d.nloc, 1u), d.stream));
  }
  ProfScope ps_(d, KID_SHAPE_SEQ);  // the sequential lane itself
  hipLaunchKernelGGL(k_shape_seq, dim3(g), dim3(kSeqChunk), 0, d.stream, a, d.corr_sorted, d.moff, hoff, hidx,
                     d.H, d.cor_rho, d.cor_last, d.X, d.seq_done);
  return hipGetLastError();
}

hipError_t launch_storm_red(Dev& d, uint32_t nparts, int64_t* red2) {
  hipLaunchKernelGGL(k_storm_red, dim3(1), dim3(kBlock), 0, d.stream, d.sig_part, nparts, red2);
  return hipGetLastError();
}
hipError_t launch_storm_unpack(Dev& d, const int64_t* red2) {
  hipLaunchKernelGGL(k_storm_unpack, dim3(1), dim3(1), 0, d.stream, red2, d.sig_part);
  return hipGetLastError();
}

hipError_t launch_pend_max(Dev& d, const uint32_t* retx, uint32_t inbox_mult, uint32_t mult, uint32_t* host) {
  hipLaunchKernelGGL(k_pend_max, dim3(kRadixBlocks), dim3(kBlock), 0, d.stream, pend_ref(d), retx,
                     inbox_mult ? d.inbox : nullptr, inbox_mult, mult, d.nloc, d.pend_part);
  TG_CHECK(hipGetLastError());
  return hipMemcpyAsync(host, d.pend_part, kRadixBlocks * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream);
}

hipError_t launch_reset_corr(Dev& d, const uint32_t* pairs_dev, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_reset_corr, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, d.stream, pairs_dev, n, d.lo,
                     d.key0, d.key1, d.cor_last);
  return hipGetLastError();
}

hipError_t window_begin(Dev& d, uint32_t n_staged, const uint32_t* n_dev) {
  d.tb_rest_owed = false;
  Queues Q = make_queues(d);  // the extraction plan was made by k_window_start
  if (n_dev) n_staged = d.cap_msgs;  // device-counted: size the launches for the capacity (grid-stride)
  HeavyOut ho;
  ho.hv = n_staged ? d.heavy : Heavy{};  // H feeds only the staged messages' sequential lane
  ho.geo = make_geo(d); ho.H = d.H; ho.hkeys = d.hkeys; ho.hvals = d.hvals; ho.hcap = d.h_cap;
  ho.lo = d.lo;
  if (!n_staged) {
    ProfScope ps_(d, KID_EXTRACT);
    hipLaunchKernelGGL(k_extract, dim3(kStreamBlocks), dim3(kBlock), 0, d.stream, d.regions, d.plan_start,
                       d.plan_off, d.arena, Q, ho);
  }
  TG_CHECK(hipGetLastError());
  if (n_staged) {
    ShapeArgs a;
    a.src = d.m_src; a.dst = d.m_dst; a.seq = d.m_seq; a.size = d.m_size; a.t = d.m_t; a.n = n_staged; a.n_dev = n_dev;
    a.status = d.status; a.shape = d.shape; a.ipf = d.ipf; a.en_bits = d.en_bits; a.rule_off = d.rule_off;
    a.rules = d.rules; a.lo = d.lo; a.nloc = d.nloc; a.data_net = d.data_net; a.data_mask = d.data_mask;
    a.data_len = d.data_len; a.key0 = d.key0; a.key1 = d.key1; a.geo = make_geo(d); a.Q = Q;
    a.stats = d.stats;
    a.corr_idx = d.corr_idx;
    a.heavy = d.heavy;
    a.may_defer = (d.any_corr || d.heavy.pend) ? 1u : 0u;
    const unsigned g = std::min<unsigned>(grid_for(n_staged), (unsigned)d.grid_shape);  // one wave of workgroups
    constexpr uint32_t ne = kStreamBlocks;  // 512 / 1024 / 4096 measured the same
    static_assert(ne % 8 == 0, "extract blocks keep their XCD");
    {
      ProfScope ps_(d, KID_SHAPE);  // extraction + netem
      hipLaunchKernelGGL(d.heavy.pend ? k_extract_shape<true> : k_extract_shape<false>, dim3(ne + g), dim3(kBlock), 0, d.stream, d.regions,
                         d.plan_start, d.plan_off, d.arena, Q, a, ne, ho);
    }
    TG_CHECK(hipGetLastError());
    if (d.any_corr || d.heavy.pend) TG_CHECK(run_shape_seq(d, a, n_staged));
  }
  if (d.ever_limited) TG_CHECK(run_token_bucket(d));  // else A is empty (Dev::ever_limited)
  if (d.S > 1) {
    hipLaunchKernelGGL(k_xheaders, dim3(1), dim3(kMaxShards), 0, d.stream, d.xsend, d.S, d.xcap, d.qc);
    TG_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

// Window end: deliveries and the wheel insert of L, interleaved in three launches -
//   k_local_hist   partition D by receiver bucket | histogram of L by wheel slot
//   k_emit_bucket  one workgroup per receiver bucket: inbox order, SoA deliveries, inbox offsets |
//                  per-slot scans of the L histogram
//   k_wheel_scatter L straight into the arena in slot order (also closes the window's counters) |
//                  long inboxes of the deliveries
static StormArgs storm_args(Dev& d, uint32_t staged_base, uint32_t round, int64_t t0, uint32_t fanout, uint32_t size,
                            int64_t spread_ns);

// spec_round != nullptr: the storm round *spec_round (fanout 8, t0 = the window's end, staged at 0)
// is generated inside the wheel-insert launch; *spec_parts = its signal partials
static hipError_t window_end_impl(Dev& d, const uint32_t* spec_round, uint32_t size, int64_t spread_ns,
                                  uint32_t* spec_parts) {
  if (d.S > 1) {
    Queues Q = make_queues(d);
    const uint32_t nb = d.S * x_slices(d.xcap) * recv_split(d.xcap);
    hipLaunchKernelGGL(k_recv, dim3(nb), dim3(kBlock), 0, d.stream, d.xrecv, d.xsend, d.S, d.shard,
                       d.xcap, Q, pend_ref(d), d.lo, d.nloc);
    TG_CHECK(hipGetLastError());
  }
  EmitPolicy p;
  p.D = d.D; p.pend = pend_ref(d); p.lo = d.lo; p.nloc = d.nloc; p.o_t = d.o_t; p.o_src = d.o_src; p.o_dst = d.o_dst; p.o_seq = d.o_seq;
  p.o_size = d.o_size; p.o_flags = d.o_flags; p.o_coff = d.o_coff;
  const BktDiv bd = bkt_div(bkt_width_fused(d, d.nloc));
  const uint32_t B = (d.nloc + bd.w - 1) / bd.w;
  if (B > (uint32_t)kMaxBins) return hipErrorInvalidValue;
  const BktSrc srcD = bkt_queue(d, Q_D), srcL = bkt_queue(d, Q_L);
  if (d.tb_rest_owed) {
    d.tb_rest_owed = false;
    ProfScope ps_(d, KID_BKT_SCATTER);
    hipLaunchKernelGGL(k_rest_local_hist, dim3(kRestRoles + 2 * kRadixBlocks), dim3(kBlock), 0, d.stream,
                       tb_policy(d), d.keys0, d.vals0, d.seg_off, d.medium, d.large, d.sc, d.K1a, d.K2a, d.K3a,
                       d.K1b, d.K2b, d.K3b, srcD, bd, B, d.kv1, d.poff, srcL, bkt_div(1), d.slots, d.hist, d.qc);
  } else {
    ProfScope ps_(d, KID_BKT_SCATTER);
    hipLaunchKernelGGL(k_local_hist, dim3(2 * kRadixBlocks), dim3(kBlock), 0, d.stream, srcD, d.sc, bd, B, d.kv1,
                       d.poff, srcL, bkt_div(1), d.slots, d.hist);
  }
  TG_CHECK(hipGetLastError());
  {
    ProfScope ps_(d, KID_EMIT);
    hipLaunchKernelGGL(k_emit_bucket, dim3(B + d.slots), dim3(kBlock), 0, d.stream, p, srcD, d.poff, d.kv1, d.keys2,
                       d.vals2, d.keys0, d.vals0, bd, B, d.nloc, d.seg_off, d.inbox, d.medium, d.large, d.sc, srcL,
                       d.hist, d.histx, d.tot, d.slots);
  }
  TG_CHECK(hipGetLastError());
  if (spec_round) {
    ProfScope ps_(d, KID_REGION_FILL);
    const StormArgs ga = storm_args(d, 0, *spec_round, INT64_MIN, 8, size, spread_ns);
    const uint64_t threads = (uint64_t)d.nloc * 8;
    const uint32_t g = (uint32_t)std::min<uint64_t>((threads + kBlock - 1) / kBlock, kSpecGenBlocks);
    hipLaunchKernelGGL(k_wheel_scatter_gen, dim3(kRadixBlocks + g + kListBlocks), dim3(kBlock), 0, d.stream, srcL,
                       d.sc, d.L, d.arena, d.dirs, d.slots, d.histx, d.tot, pend_ref(d), d.lo, d.nloc, p, d.keys0, d.vals0,
                       d.seg_off, d.medium, d.large, d.K1a, d.K2a, d.K3a, d.K1b, d.K2b, d.K3b, ga, sig_state(d), g);
    *spec_parts = g;
  } else if (d.side) {  // the insert beside what follows the window (the flood's reaction)
    TG_CHECK(hipEventRecord(d.main_ev, d.stream));
    TG_CHECK(hipStreamWaitEvent(d.side, d.main_ev, 0));
    {
      ProfScope ps_(d, KID_REGION_FILL, d.side);
      hipLaunchKernelGGL(k_wheel_insert, dim3(kRadixBlocks), dim3(kBlock), 0, d.side, srcL, d.sc, d.L, d.arena, d.dirs,
                         d.slots, d.histx, d.tot, pend_ref(d), d.lo, d.nloc);
    }
    TG_CHECK(hipGetLastError());
    TG_CHECK(hipEventRecord(d.side_ev, d.side));
    d.side_pending = true;
    ProfScope ps_(d, KID_SEG_REST);
    hipLaunchKernelGGL(k_inbox_rest, dim3(kListBlocks), dim3(kBlock), 0, d.stream, d.sc, p, d.keys0, d.vals0,
                       d.seg_off, d.medium, d.large, d.K1a, d.K2a, d.K3a, d.K1b, d.K2b, d.K3b);
  } else {
    ProfScope ps_(d, KID_REGION_FILL);
    hipLaunchKernelGGL(k_wheel_scatter, dim3(kRadixBlocks + kListBlocks), dim3(kBlock), 0, d.stream, srcL, d.sc, d.L,
                       d.arena, d.dirs, d.slots, d.histx, d.tot, pend_ref(d), d.lo, d.nloc, p, d.keys0, d.vals0, d.seg_off,
                       d.medium, d.large, d.K1a, d.K2a, d.K3a, d.K1b, d.K2b, d.K3b);
  }
  return hipGetLastError();
}

// The context stream waits for the side stream's insert (every entry point but the ones that may run
// beside it does this first)
hipError_t join_side(Dev& d) {
  if (!d.side_pending) return hipSuccess;
  d.side_pending = false;
  return hipStreamWaitEvent(d.stream, d.side_ev, 0);
}

hipError_t window_end(Dev& d) { return window_end_impl(d, nullptr, 0, 0, nullptr); }

hipError_t window_end_storm(Dev& d, uint32_t round, uint32_t size, int64_t spread_ns, uint32_t* nparts) {
  return window_end_impl(d, &round, size, spread_ns, nparts);
}

hipError_t signal_batch(Dev& d, uint32_t n, uint32_t kmin, uint32_t kmax, uint64_t log_base, uint32_t n_waiters,
                        bool count_only) {
  if (n) {
    if (count_only) {  // commit and waiters in the same launch
      const unsigned g = grid_for(n);
      hipLaunchKernelGGL(k_sig_count, dim3(g), dim3(kBlock), 0, d.stream, sig_state(d), d.s_t, n);
      return launch_sig_commit(d, g, true, n, kmin, n_waiters, false, 0, 0, 0);
    } else {
      uint32_t* n_dev = &d.sc->sig_n;
      hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, d.stream, n_dev, n);
      const uint32_t K = kmax - kmin + 1;
      hipLaunchKernelGGL(k_keys_sig, dim3(grid_for(n)), dim3(kBlock), 0, d.stream, d.s_state, n_dev, kmin, d.keys0,
                         d.vals0);
      uint32_t *keys, *vals;
      BktSrc src = bkt_queue(d, Q_A);
      src.keys = d.keys0; src.vals = d.vals0; src.qc = nullptr; src.mode = 3; src.n_ptr = n_dev;
      TG_CHECK(group_by_bkt(d, src, K, kNoMedium, nullptr, &keys, &vals));
      SigPolicy p;
      p.inst = d.s_inst; p.t = d.s_t; p.count = d.st_count; p.seq_out = d.s_seq; p.log = d.sig_log;
      p.log_base = log_base; p.kmin = kmin;
      hipLaunchKernelGGL(k_seg_small<SigPolicy>, dim3(kStreamBlocks), dim3(kBlock), 0, d.stream, p, keys, vals,
                         d.seg_off, n_dev, d.cap_rec);
      TG_CHECK(hipGetLastError());
      TG_CHECK(launch_rest(d, p, keys, vals));
      hipLaunchKernelGGL(k_sig_commit, dim3(grid_for(K)), dim3(kBlock), 0, d.stream, d.seg_off, K, kmin, log_base,
                         d.sig_log, d.st_count, d.st_last, d.st_nchunks, d.st_chunks, d.sc);
      TG_CHECK(hipGetLastError());
    }
  }
  return resolve_waiters(d, n_waiters);
}

hipError_t add_waiter(Dev& d, uint32_t idx, uint32_t state, uint32_t target, int64_t t_wait) {
  hipLaunchKernelGGL(k_add_waiter, dim3(1), dim3(1), 0, d.stream, sig_state(d), d.w_state, d.w_target, d.w_twait,
                     idx, state, target, t_wait);
  return hipGetLastError();
}

hipError_t resolve_waiters(Dev& d, uint32_t n_waiters) {
  if (!n_waiters) return hipSuccess;
  hipLaunchKernelGGL(k_waiters, dim3(grid_for(n_waiters)), dim3(kBlock), 0, d.stream, sig_state(d), n_waiters);
  return hipGetLastError();
}

// Grids of the grid-stride kernels whose register use caps residency below 8 waves per SIMD: one
// wave of workgroups (resident blocks per CU x CUs), so no tail of late workgroups.
void init_launch_geometry(Dev& d) {
  int b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_shape, kBlock, 0) == hipSuccess && b > 0)
    d.grid_shape = b * d.n_cu;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_gen_storm<8>, kBlock, 0) == hipSuccess && b > 0)
    d.grid_gen = b * d.n_cu;
}

hipError_t launch_sig_commit(Dev& d, uint32_t nparts, bool commit, uint32_t n, uint32_t st, uint32_t n_waiters,
                             bool add, uint32_t add_state, uint32_t add_target, int64_t add_twait) {
  const WaiterAdd wa = waiter_add(d, add, add_state, add_target, add_twait);
  hipLaunchKernelGGL(k_sig_commit, dim3(1), dim3(kBlock), 0, d.stream, sig_state(d), nparts, commit ? 1u : 0u, n, st,
                     n_waiters, wa);
  return hipGetLastError();
}

// slot_div_make at 32 bits for the peer draw (d = N - 1 >= 1): m = floor(2^32 (2^l - d) / d) + 1 < 2^32.
static void peer_divisor(uint32_t d, uint32_t& m, uint32_t& sh1, uint32_t& sh2) {
  uint32_t l = 0;
  while (l < 32 && (1ull << l) < d) ++l;
  m = (uint32_t)((((unsigned __int128)1 << 32) * ((1ull << l) - d)) / d + 1);
  sh1 = l < 1 ? l : 1;
  sh2 = l > 1 ? l - 1 : 0;
}

// k_gen_storm only: the batch's per-block partials wait in sig_part for launch_sig_commit (the
// runtime defers it so that a barrier registered next rides in the same launch). *nparts = grid.
static StormArgs storm_args(Dev& d, uint32_t staged_base, uint32_t round, int64_t t0, uint32_t fanout, uint32_t size,
                            int64_t spread_ns) {
  StormArgs a;
  a.lo = d.lo; a.nloc = d.nloc; a.N = d.N; a.round = round; a.t0 = t0; a.F = fanout;
  a.Fp = 1; a.fp_log2 = 0;
  while (a.Fp < fanout) { a.Fp <<= 1; ++a.fp_log2; }
  peer_divisor(d.N > 1 ? d.N - 1 : 1, a.peer_m, a.peer_sh1, a.peer_sh2);
  a.size = size; a.spread = spread_ns; a.key0 = d.key0;
  a.spread_div = slot_div_make(spread_ns > 0 ? (uint64_t)spread_ns : 0); a.key1 = d.key1; a.base = staged_base;
  a.m_src = d.m_src; a.m_dst = d.m_dst; a.m_seq = d.m_seq; a.m_size = d.m_size; a.m_t = d.m_t;
  return a;
}

hipError_t launch_gen_storm(Dev& d, uint32_t staged_base, uint32_t round, int64_t t0, uint32_t fanout,
                            uint32_t size, int64_t spread_ns, uint32_t* nparts) {
  ProfScope ps_(d, KID_GEN);
  const StormArgs a = storm_args(d, staged_base, round, t0, fanout, size, spread_ns);
  const uint64_t threads = (uint64_t)d.nloc * a.Fp;
  const unsigned g = (unsigned)std::min<uint64_t>((threads + kBlock - 1) / kBlock,
                                                  std::min<uint64_t>(kSigParts, (uint64_t)d.grid_gen));
  if (fanout == 8) hipLaunchKernelGGL(k_gen_storm<8>, dim3(g), dim3(kBlock), 0, d.stream, a, sig_state(d));
  else hipLaunchKernelGGL(k_gen_storm<0>, dim3(g), dim3(kBlock), 0, d.stream, a, sig_state(d));
  *nparts = g;
  return hipGetLastError();
}

}  // namespace tgsim

#ifdef TGSIM_PHASE_PROF
// debug builds only: the phase clocks of the last k_tb_bucket / k_emit_bucket launches
extern "C" int tgsim_debug_phases(uint64_t* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgsim::g_tg_ph), sizeof(tgsim::g_tg_ph));
}
// ... and of the last k_shape_seq_wide launch (per block)
extern "C" int tgsim_debug_wide_phases(uint64_t* out) {  // [4096][12]
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgsim::g_wide_ph), sizeof(tgsim::g_wide_ph));
}
// ... and of the last task-parallel long-segment pass (per task; then the last chunk sort's two clocks)
extern "C" int tgsim_debug_task_phases(uint64_t* out) {
  const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgsim::g_task_ph), sizeof(tgsim::g_task_ph));
  if (rc) return rc;
  return (int)hipMemcpyFromSymbol(out + 4 * 4096, HIP_SYMBOL(tgsim::g_chunk_ph), sizeof(tgsim::g_chunk_ph));
}
// ... and of the last whole-inbox sort (whole_sort)
extern "C" int tgsim_debug_whole_phases(uint64_t* out) {  // [8]
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgsim::g_whole_ph), sizeof(tgsim::g_whole_ph));
}
// ... and of the last k_shape_seq launch (per block: its last sender)
extern "C" int tgsim_debug_seq_phases(uint64_t* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgsim::g_seq_ph), sizeof(tgsim::g_seq_ph));
}
#endif
