/* tgsim_netstat.h — per-instance traffic counters accumulated on the device.
 *
 * What `ip -s link` / `tc -s qdisc show` would print for one instance, and the totals behind the
 * plans' bytes.sent / bytes.read counters: while enabled, every window adds its statuses (by sender)
 * and its deliveries (by receiver) into 64-bit counters in device memory, with no host read. The
 * counters are read on demand, as host copies or as device pointers.
 *
 * Off by default; a context that never enables it launches and behaves exactly as without this header.
 * The facility exists on the device only (its reference is a reduction of the per-window outputs the
 * CPU oracle already pins), so these entry points live here and not in tgsim.h.
 *
 * TX, per staged message i a window decides, s = src[i] (a local sender), st its status byte:
 *   tx_msgs[s] += 1, tx_bytes[s] += size[i], tx_status[s][st & 0x0F] += 1 (codes 0..8),
 *   tx_queued_bytes[s] += size[i] when the code is TGSIM_ST_QUEUED,
 *   tx_dup / tx_clone_lost / tx_dup_cancel / tx_orig_overlimit[s] += 1 per status flag 0x10 / 0x20 / 0x40 / 0x80.
 * RX, per delivery j of the window, r = dst[j] (always local):
 *   rx_packets[r] += 1, rx_bytes[r] += size[j], rx_corrupt / rx_clones / rx_reordered / rx_local[r] += 1
 *   per TGSIM_F_CORRUPT / _CLONE / _REORDERED / _LOCAL, rx_t_last[r] = max(rx_t_last[r], t_deliver[j])
 *   (INT64_MIN while there is none; late deliveries make times non-monotone across windows).
 * In TCP mode the unit is the packet (data segments, retransmissions, ACKs); with probes or the storm
 * reactor the staged message. Counting starts with the first window that begins after enabling.
 */
#ifndef TGSIM_NETSTAT_H
#define TGSIM_NETSTAT_H

#include "tgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGSIM_NETSTAT_CODES 9 /* status codes TGSIM_ST_QUEUED .. TGSIM_ST_OVERLIMIT */

typedef struct tgsim_netstat_soa {   /* any pointer may be NULL (field not wanted) */
  uint64_t *tx_msgs, *tx_bytes, *tx_queued_bytes;
  uint64_t *tx_status;               /* [n * TGSIM_NETSTAT_CODES], instance-major */
  uint64_t *tx_dup, *tx_clone_lost, *tx_dup_cancel, *tx_orig_overlimit;
  uint64_t *rx_packets, *rx_bytes, *rx_corrupt, *rx_clones, *rx_reordered, *rx_local;
  int64_t  *rx_t_last;
} tgsim_netstat_soa;

/* on = 1: count from the next window on (the counters are allocated and zeroed at the first use);
 * on = 0: stop counting, the values stay readable. TGSIM_ESTATE between advance_begin and advance_end. */
int tgsim_netstat_enable(tgsim_ctx* ctx, int32_t on);
/* Zero the counters, rx_t_last = INT64_MIN. */
int tgsim_netstat_reset(tgsim_ctx* ctx);
/* Host copies of the rows of the global instances [first_instance, first_instance + n), which must lie
 * inside this shard's range (else TGSIM_EINVAL). Synchronises the stream. */
int tgsim_netstat_copy(tgsim_ctx* ctx, uint32_t first_instance, size_t n, const tgsim_netstat_soa* out);
/* The device arrays, indexed by local instance (global id - the shard's lo); valid until tgsim_destroy. */
int tgsim_netstat_device(tgsim_ctx* ctx, tgsim_netstat_soa* out_device_ptrs);
/* Every call but tgsim_netstat_enable returns TGSIM_ESTATE while netstat was never enabled. A snapshot of
 * a context that enabled netstat carries the counters; it restores only into a context that enabled
 * netstat before the restore; an image without them only into one that never did. */

#ifdef __cplusplus
}
#endif
#endif
