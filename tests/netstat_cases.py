"""Netstat (include/tgsim_netstat.h): the reference reduction and the seeded drivers of
tests/test_netstat_cpu.py and tests/test_netstat.py.

The reference is a numpy reduction of per-window outputs the CPU oracle already pins: statuses by
sender, deliveries by receiver, exactly the tables of DESIGN.md 2.15. The drivers enqueue explicitly, so
src / size of every window are known; each takes (binding, on_sim, on_window) and so runs on both
bindings: on_sim(sim) right after a context is created, on_window(w, sim, win) after window w with
win = dict(src, size, status, deliv) - it may return another Simulator to continue on (checkpoint /
resume). A driver returns the list of its windows and, last, dict(stats=tgsim_stats at the end)."""
from __future__ import annotations

import functools

import numpy as np

from testground_amd import _abi as A
from testground_amd.sim import SimConfig, Simulator, int_to_ip, make_rule, make_shape
from tests import scenarios as S

MS = S.MS
I64_MIN = -(1 << 63)
TX_FLAGS = (("tx_dup", A.ST_FLAG_DUP), ("tx_clone_lost", A.ST_FLAG_CLONE_LOST),
            ("tx_dup_cancel", A.ST_FLAG_DUP_CANCEL), ("tx_orig_overlimit", A.ST_FLAG_OVERLIMIT))
RX_FLAGS = (("rx_corrupt", A.F_CORRUPT), ("rx_clones", A.F_CLONE), ("rx_reordered", A.F_REORDERED),
            ("rx_local", A.F_LOCAL))


# ---- the reference ----------------------------------------------------------------------------

def empty(n: int) -> dict:
    """Counters of instances 0..n-1 as tgsim_netstat_reset leaves them."""
    acc = {f: np.zeros((n, A.NETSTAT_CODES) if f == "tx_status" else n, np.uint64) for f in A.NETSTAT_FIELDS}
    acc["rx_t_last"] = np.full(n, I64_MIN, np.int64)
    return acc


def add_window(acc: dict, src, size, status, deliv) -> dict:
    """One window into acc (global instance rows): np.bincount by sender / receiver."""
    n = len(acc["tx_msgs"])
    src = np.asarray(src, np.int64)
    size = np.asarray(size, np.int64)
    st = np.asarray(status, np.int64)
    assert len(src) == len(size) == len(st), (len(src), len(size), len(st))

    def count(idx, mask=None):
        return np.bincount(idx if mask is None else idx[mask], minlength=n).astype(np.uint64)

    def total(idx, w, mask=None):  # integer sums: add.at is exact where float weights would round
        out = np.zeros(n, np.uint64)
        np.add.at(out, idx if mask is None else idx[mask], (w if mask is None else w[mask]).astype(np.uint64))
        return out

    code = st & 0x0F
    acc["tx_msgs"] += count(src)
    acc["tx_bytes"] += total(src, size)
    acc["tx_queued_bytes"] += total(src, size, code == A.ST_QUEUED)
    for c in range(A.NETSTAT_CODES):
        acc["tx_status"][:, c] += count(src, code == c)
    for name, bit in TX_FLAGS:
        acc[name] += count(src, (st & bit) != 0)
    dst = np.asarray(deliv["dst"], np.int64)
    fl = np.asarray(deliv["flags"], np.int64)
    acc["rx_packets"] += count(dst)
    acc["rx_bytes"] += total(dst, np.asarray(deliv["size"], np.int64))
    for name, bit in RX_FLAGS:
        acc[name] += count(dst, (fl & bit) != 0)
    np.maximum.at(acc["rx_t_last"], dst, np.asarray(deliv["t_deliver"], np.int64))
    return acc


def reduce_windows(wins, n: int) -> dict:
    acc = empty(n)
    for w in wins:
        add_window(acc, w["src"], w["size"], w["status"], w["deliv"])
    return acc


def assert_rows(got: dict, acc: dict, lo: int = 0, hi: int | None = None, what: str = "netstat"):
    """got (a shard's rows, Simulator.netstat()) equals rows [lo, hi) of the reference, field by field."""
    hi = len(acc["tx_msgs"]) if hi is None else hi
    assert set(got) == set(A.NETSTAT_FIELDS)
    for f in A.NETSTAT_FIELDS:
        want = acc[f][lo:hi]
        assert got[f].dtype == want.dtype and got[f].shape == want.shape, (what, f, got[f].dtype, got[f].shape)
        if not np.array_equal(got[f], want):
            bad = np.argwhere(got[f] != want)[:8]
            raise AssertionError(f"{what}: {f} differs at rows {bad.tolist()}: "
                                 f"{[got[f][tuple(b)] for b in bad]} vs {[want[tuple(b)] for b in bad]}")


def stats_sums(acc: dict) -> dict:
    """The shard sums that equal tgsim_stats deltas (overlimit counts copies and equals none)."""
    st = acc["tx_status"].sum(axis=0)
    return dict(msgs_in=int(acc["tx_msgs"].sum()), lost=int(st[1]), dropped=int(st[2]), rejected=int(st[3]),
                unreachable=int(st[4]), external=int(st[5]), dest_down=int(st[6]), local=int(st[7]),
                delivered=int(acc["rx_packets"].sum()))


# ---- drivers ------------------------------------------------------------------------------------

def _window(sim, w, batch, t_end, out, on_window):
    """Stage batch = (src, dst, seq, size, t) or None, run the window, collect, call the hook."""
    if batch is not None and len(batch[0]):
        sim.enqueue(*batch)
    sim.advance(t_end)
    src, size = (batch[0], batch[3]) if batch is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    win = dict(src=np.asarray(src, np.int64), size=np.asarray(size, np.int64), status=sim.status(),
               deliv=sim.deliveries())
    out.append(win)
    if on_window is not None:
        nxt = on_window(w, sim, win)
        if nxt is not None:
            sim = nxt
    return sim


def _finish(sim, out):
    out.append(dict(stats=sim.stats()))
    sim.close()
    return out


def random_plan(seed: int, n_inst: int, get_ip, windows: int = 6, msgs: int = 300, window_ns: int = 40 * MS):
    """scenarios.run_random's workload as a plan every shard of a run can follow: ("cfg", f) with
    f(sim) a configuration step, ("win", batch, t_end) a window. Sizes include 0 and 65536; rules, an
    external destination, loopback and a disabled link are present; the three drain windows stage
    nothing, and a last window of 1 ns neither stages nor delivers anything."""
    rng = np.random.default_rng(seed)
    seqc = np.zeros(n_inst, np.int64)
    for g in range(n_inst):
        shp = S.random_shape(rng)
        allow = rng.random() < 0.3
        yield "cfg", (lambda sim, g=g, shp=shp, allow=allow:
                      (sim.set_shape(g, shp), allow and sim.set_policy(g, A.POLICY_ALLOW_ALL)))
    for g in rng.choice(n_inst, size=n_inst // 3, replace=False):
        rl = []
        for _ in range(int(rng.integers(1, 6))):
            ip = get_ip(int(rng.integers(0, n_inst)))
            plen = int(rng.choice([32, 32, 30, 24, 16, 0]))
            mask = (0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF if plen else 0
            f = int(rng.choice([A.FILTER_DROP, A.FILTER_REJECT, A.FILTER_ACCEPT]))
            rl.append(make_rule(f"{int_to_ip(ip & mask)}/{plen}", f))
        yield "cfg", (lambda sim, g=int(g), rl=rl: sim.add_rules(g, rl))
    t0 = 0
    for w in range(windows):
        if w == windows // 2:  # mid-run: new shapes, an address change, a disabled link
            for g in rng.choice(n_inst, size=4, replace=False):
                shp = S.random_shape(rng)
                yield "cfg", (lambda sim, g=int(g), shp=shp: sim.set_shape(g, shp))
            g = int(rng.integers(0, n_inst))
            ip = get_ip(g) + 1000
            yield "cfg", (lambda sim, g=g, ip=ip: (sim.set_enabled(g, True, ip=ip),
                                                   sim.set_enabled((g + 3) % n_inst, False)))
        src = rng.integers(0, n_inst, msgs)
        dst = rng.integers(0, n_inst, msgs)
        dst[rng.random(msgs) < 0.03] = A.DST_EXTERNAL
        loc = rng.random(msgs) < 0.02
        dst[loc] = src[loc]
        seq = np.zeros(msgs, np.int64)
        for i in range(msgs):
            seq[i] = seqc[src[i]]
            seqc[src[i]] += 1
        size = rng.choice([0, 1, 64, 1024, 4096, 65536], msgs)
        t = t0 + np.sort(rng.integers(0, window_ns, msgs))
        if rng.random() < 0.5:
            t[: msgs // 4] = t0
        t0 += window_ns
        yield "win", (src, dst, seq, size, t), t0
    for _ in range(3):
        t0 += 10 * window_ns
        yield "win", None, t0
    yield "win", None, t0 + 1  # slow token buckets still hold copies: a 1 ns window that delivers nothing


def drv_random(binding, on_sim=None, on_window=None, seed: int = 1, n_inst: int = 24):
    sim = Simulator(SimConfig(n_instances=n_inst, seed=1000 + seed), binding=binding)
    if on_sim is not None:
        on_sim(sim)
    base = sim.get_ip(0)  # addresses at the start: data subnet + 2 + id (the plan is the same for every shard)
    out, w = [], 0
    for step in random_plan(seed, n_inst, lambda g: base + g):
        if step[0] == "cfg":
            step[1](sim)
        else:
            sim = _window(sim, w, step[1], step[2], out, on_window)
            w += 1
    return _finish(sim, out)


def drv_random_sharded(make_sim, exchange, world: int, on_window=None, seed: int = 1, n_inst: int = 25):
    """drv_random over `world` shards of one process (scenarios.run_random_sharded's protocol: every
    shard gets every configuration call and its own senders' messages; begin, exchange, end).
    make_sim(cfg) -> Simulator; on_window(w, sims). Returns nothing: the single run is the reference."""
    sims = [make_sim(SimConfig(n_instances=n_inst, seed=1000 + seed, **S.shard_cfg(world, k, exchange_cap=4096)))
            for k in range(world)]
    base = sims[0].get_ip(0)
    w = 0
    for step in random_plan(seed, n_inst, lambda g: base + g):
        if step[0] == "cfg":
            for s in sims:
                step[1](s)
            continue
        if step[1] is not None:
            src = step[1][0]
            for s in sims:
                m = (src >= s.lo) & (src < s.hi)
                if m.any():
                    s.enqueue(*(x[m] for x in step[1]))
        for s in sims:
            s.advance_begin(step[2])
        exchange(sims)
        for s in sims:
            s.advance_end()
        if on_window is not None:
            on_window(w, sims)
        w += 1
    for s in sims:
        s.close()


TX_RUN_KINDS = ("random", "sorted1000", "one_sender", "single")


def drv_tx_runs(binding, on_sim=None, on_window=None, kind: str = "random", n_inst: int = 16):
    """One window whose senders arrive fully random (3001 messages), sorted by sender in runs of 1000
    (6037: runs cross waves and workgroups), all from one sender (4099, past the queue limit) or as a
    single message - counts that are no multiple of 4, 64 or 256 - then a drain window."""
    rng = np.random.default_rng(TX_RUN_KINDS.index(kind) + 7)
    sim = Simulator(SimConfig(n_instances=n_inst, seed=77), binding=binding)
    if on_sim is not None:
        on_sim(sim)
    for g in range(n_inst):
        sim.set_shape(g, make_shape(latency_ns=(5 + g % 3) * MS, loss=10.0, duplicate=10.0))
    n = dict(random=3001, sorted1000=6037, one_sender=4099, single=1)[kind]
    src = dict(random=rng.integers(0, n_inst, n), sorted1000=(np.arange(n) // 1000) % n_inst,
               one_sender=np.full(n, 3), single=np.full(n, n_inst - 1))[kind]
    dst = (src + rng.integers(1, n_inst, n)) % n_inst
    size = rng.choice([0, 64, 1500, 65536], n)
    t = np.sort(rng.integers(0, 10 * MS, n))
    out = []
    sim = _window(sim, 0, (src, dst, np.arange(n), size, t), 10 * MS, out, on_window)
    sim = _window(sim, 1, None, 100 * MS, out, on_window)
    return _finish(sim, out)


def drv_burst(binding, on_sim=None, on_window=None, seed: int = 1, n_inst: int = 10, windows: int = 5,
              per_sender: int = 1400, window_ns: int = 4 * MS):
    """scenarios.run_burst's queue-limit bursts (OVERLIMIT and all four status flags), with hooks."""
    rng = np.random.default_rng(seed)
    sim = Simulator(SimConfig(n_instances=n_inst, seed=2000 + seed, max_msgs_per_window=1 << 16,
                              max_records=1 << 18), binding=binding)
    if on_sim is not None:
        on_sim(sim)
    shapes = [
        make_shape(latency_ns=10 * MS, jitter_ns=3 * MS),
        make_shape(latency_ns=2 * MS, bandwidth_bps=100_000_000),
        make_shape(latency_ns=5 * MS, duplicate=30.0, loss=5.0),
        make_shape(latency_ns=1 * MS, jitter_ns=1 * MS, reorder=20.0, corrupt=10.0, bandwidth_bps=400_000_000),
        make_shape(latency_ns=8 * MS, duplicate=20.0, duplicate_corr=50.0, reorder=10.0, reorder_corr=30.0),
        make_shape(),
    ]
    for g, shp in enumerate(shapes):
        sim.set_shape(g, shp)
    seqc = np.zeros(n_inst, np.int64)
    out, t0 = [], 0
    for w in range(windows + 4):
        src, ts = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        if w < windows:
            for g in range(len(shapes)):
                k = per_sender if (w + g) % 3 else per_sender // 4
                t = t0 + np.sort(rng.integers(0, window_ns // 2, k))
                t[: k // 4] = t0
                src.append(np.full(k, g)); ts.append(t)
            src.append(rng.integers(len(shapes), n_inst, 50)); ts.append(t0 + rng.integers(0, window_ns, 50))
            if w > 0:   # reactions at the horizon: sent before this window's start
                src.append(rng.integers(0, len(shapes), 120)); ts.append(t0 - rng.integers(1, window_ns, 120))
        src, ts = np.concatenate(src), np.concatenate(ts)
        n = len(src)
        dst = (src + rng.integers(1, n_inst, n)) % n_inst
        seq = np.zeros(n, np.int64)
        for i in range(n):
            seq[i] = seqc[src[i]]
            seqc[src[i]] += 1
        size = rng.choice([64, 1000, 1500], n)
        t0 += window_ns if w < windows else 60 * MS
        sim = _window(sim, w, (src, dst, seq, size, ts) if n else None, t0, out, on_window)
    return _finish(sim, out)


def drv_long_inbox(binding, on_sim=None, on_window=None, n_inst: int = 64, n_long: int = 9001):
    """One receiver's inbox of 9001 deliveries (over 8192: the rest roles write it, its RX run spans
    many waves) among 64 instances whose other inboxes are empty or at most 2 long."""
    rng = np.random.default_rng(31)
    sim = Simulator(SimConfig(n_instances=n_inst, seed=31), binding=binding)
    if on_sim is not None:
        on_sim(sim)
    for g in range(n_inst):
        sim.set_shape(g, make_shape(latency_ns=(1 + g % 4) * MS, jitter_ns=(g % 2) * MS))
    hot = 5
    src = rng.integers(0, n_inst - 1, n_long)
    src[src >= hot] += 1
    few = rng.choice(np.delete(np.arange(n_inst), hot), size=20, replace=False)
    dst = np.r_[np.full(n_long, hot), few, few[:12]]
    src = np.r_[src, (dst[n_long:] + 1 + rng.integers(0, n_inst - 2, 32)) % n_inst]
    src[n_long:][src[n_long:] == dst[n_long:]] = hot
    n = len(src)
    order = rng.permutation(n)
    src, dst = src[order], dst[order]
    out = []
    batch = (src, dst, np.arange(n), rng.choice([64, 1500], n), np.sort(rng.integers(0, 5 * MS, n)))
    sim = _window(sim, 0, batch, 20 * MS, out, on_window)
    sim = _window(sim, 1, None, 40 * MS, out, on_window)
    return _finish(sim, out)


DRIVERS = dict(random=drv_random, burst=drv_burst, long_inbox=drv_long_inbox,
               **{"tx_" + k: functools.partial(drv_tx_runs, kind=k) for k in TX_RUN_KINDS})


@functools.lru_cache(maxsize=None)
def oracle_run(name: str):
    """The CPU oracle's run of DRIVERS[name], computed once per session; read-only."""
    from oracle.pyoracle import oracle_binding
    return DRIVERS[name](oracle_binding())


def storm_windows(out, fanout: int = 8, size: int = 1024):
    """scenarios.run_storm's rounds as windows: message i of a round is sender i // fanout's."""
    return [dict(src=np.arange(len(x["status"])) // fanout, size=np.full(len(x["status"]), size),
                 status=x["status"], deliv=x["deliv"]) for x in out[:-1]]
