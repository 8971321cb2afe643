"""The fused bucket consumers (k_tb_bucket, k_emit_bucket) at the shapes where their LDS phases can
go wrong, HIP against the oracle: multi-key buckets (1200 instances: 24 keys per bucket, 50
buckets), every run length from 0 to 12 with ties on the first sort key, the rank limit (512 / 513
copies of one sender), the item capacity (1536 / 1537 items in a bucket, an empty bucket beside
them), a bucket whose times span more than 2^32 ns, and the ladder again on two shards of one
device. Every scenario also checks on the oracle's output alone that it produces what it claims."""
import numpy as np
import pytest

from testground_amd import _abi as A
from testground_amd.sim import SimConfig, Simulator, make_shape

from tests import scenarios as S

MS = S.MS
N = 1200           # > 1024 instances: bkt_width_fused gives 24 keys per bucket, 50 buckets
KEYS = 24
LADDER = {0, 1, 2, 3, 4, 5, 7, 8, 9, 12}
SEQ_STRIDE = 16    # seq = window * SEQ_STRIDE + index: a delivery names the window it was sent in


def _drive(sims, ranges, exchange, windows, ends, counters=None):
    """windows: per window (src, dst, seq, size, t) or None (drain); ends: the window ends. Every
    context gets its own senders' messages; returns per context the observables of S.run_storm."""
    outs = [[] for _ in sims]
    for msgs, t_end in zip(windows, ends):
        if msgs is not None:
            src = msgs[0]
            for s, (lo, hi) in zip(sims, ranges):
                m = (src >= lo) & (src < hi)
                if m.any():
                    s.enqueue(*[x[m] for x in msgs])
        if exchange is None:
            for s in sims:
                s.advance(t_end)
        else:
            for s in sims:
                s.advance_begin(t_end)
            exchange(sims)
            for s in sims:
                s.advance_end()
        for o, s in zip(outs, sims):
            o.append(dict(now=s.now, status=s.status(), deliv=s.deliveries(), inbox=s.inbox_offsets()))
        if counters is not None:
            counters.append(sims[0].kernel_counters())
    for o, s in zip(outs, sims):
        o.append(dict(stats=S.parity_stats(s)))
        s.close()
    return outs


def _run_single(binding, shapes, windows, ends, seed, counters=None):
    sim = Simulator(SimConfig(n_instances=N, seed=seed, max_msgs_per_window=1 << 16, max_records=1 << 18),
                    binding=binding)
    sim.set_shapes(np.arange(N), shapes)
    return _drive([sim], [(0, N)], None, windows, ends, counters)[0]


def _all_deliveries(out):
    return {f: np.concatenate([w["deliv"][f] for w in out[:-1]]) for f in out[0]["deliv"]}


# ---- the run-length ladder ----------------------------------------------------------------------

def _ladder_inputs():
    """Sender g sends g % 13 messages a window, all at the window start, to one receiver (a
    permutation of the instances, so the inbox runs repeat the senders' ladder). No jitter: the
    copies of an unlimited sender (odd g) tie on the netem time and arrive together, seq and the
    clone bit decide; an even sender's 1 Mbit/s bucket (8 ms per 1000-B packet against 1-3 ms of
    latency) binds, so its departures replace the netem times and run over the window ends."""
    rng = np.random.default_rng(11)
    perm = rng.permutation(N)
    fixed = np.flatnonzero(perm == np.arange(N))
    for g in fixed:  # nobody sends to itself
        o = (g + 1) % N
        perm[g], perm[o] = perm[o], perm[g]
    assert not (perm == np.arange(N)).any()
    shapes = [make_shape(latency_ns=(1 + g % 3) * MS, duplicate=50.0, bandwidth_bps=0 if g % 2 else 1_000_000)
              for g in range(N)]
    per = np.arange(N) % 13
    src = np.repeat(np.arange(N), per)
    idx = np.concatenate([np.arange(k) for k in per])
    windows, ends = [], []
    for w in range(3):
        windows.append((src, perm[src], w * SEQ_STRIDE + idx, np.full(len(src), 1000), np.full(len(src), w * 10 * MS)))
        ends.append((w + 1) * 10 * MS)
    windows.append(None)  # drain: the slowest sender holds 3 * 12 * 2 copies of 8 ms each
    ends.append(30 * MS + 2000 * MS)
    return shapes, windows, ends


_cache = {}


def _ladder_oracle(oracle):
    if "ladder" not in _cache:
        shapes, windows, ends = _ladder_inputs()
        _cache["ladder"] = _run_single(oracle, shapes, windows, ends, seed=21)
    return _cache["ladder"]


def _check_ladder_claims(out):
    runs = set()
    for w in out[:-1]:
        runs |= set(np.diff(w["inbox"].astype(np.int64)).tolist())
    assert LADDER <= runs, sorted(runs)
    d = _all_deliveries(out)
    copies = np.bincount(d["src"].astype(np.int64) * 3 + d["seq"].astype(np.int64) // SEQ_STRIDE, minlength=3 * N)
    assert LADDER <= set(copies.tolist()), sorted(set(copies.tolist()))
    pair = clone_tie = bound = 0
    for w in out[:-1]:
        x = w["deliv"]
        same = (x["dst"][1:] == x["dst"][:-1]) & (x["t_deliver"][1:] == x["t_deliver"][:-1]) & \
               (x["src"][1:] == x["src"][:-1])
        pair += int((same & (x["seq"][1:] != x["seq"][:-1])).sum())
        clone = (x["flags"] & A.F_CLONE) != 0
        clone_tie += int((same & (x["seq"][1:] == x["seq"][:-1]) & clone[:-1] & ~clone[1:]).sum())
        # a limited sender's later copies leave after their netem time (t_send + latency <= 3 ms)
        sent = (x["seq"].astype(np.int64) // SEQ_STRIDE) * 10 * MS
        bound += int(((x["src"] % 2 == 0) & (x["t_deliver"] > sent + 3 * MS)).sum())
    assert pair > 0 and clone_tie > 0 and bound > 0, (pair, clone_tie, bound)


def test_ladder_claims(oracle):
    _check_ladder_claims(_ladder_oracle(oracle))


@pytest.mark.gpu
def test_run_length_ladder(hip, oracle):
    """Runs of 0-12 with ties in both consumers, token state carried over three windows and a drain."""
    shapes, windows, ends = _ladder_inputs()
    S.assert_same(_run_single(hip, shapes, windows, ends, seed=21), _ladder_oracle(oracle))


@pytest.mark.gpu
def test_ladder_two_shards(hip, oracle):
    """The ladder on two contexts of one device (the X runs of k_tb_bucket) against the single one."""
    import ctypes as C
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def exchange(sims):
        n = len(sims)
        bufs = [s.exchange_buffers() for s in sims]
        blk = bufs[0][2] // n
        for s in sims:
            s.sync()
        for q in range(n):
            for p in range(n):
                assert hiprt.hipMemcpy(bufs[p][1] + q * blk, bufs[q][0] + p * blk, blk, 3) == 0  # device to device
        assert hiprt.hipDeviceSynchronize() == 0

    shapes, windows, ends = _ladder_inputs()
    sims = []
    for k in range(2):
        s = Simulator(SimConfig(n_instances=N, seed=21, max_msgs_per_window=1 << 16, max_records=1 << 18,
                                **S.shard_cfg(2, k, exchange_cap=1 << 15)), binding=hip)
        s.set_shapes(np.arange(N), shapes)
        sims.append(s)
    outs = _drive(sims, [S.shard_range(N, k, 2) for k in range(2)], exchange, windows, ends)
    S.assert_storm_sharded(outs, _ladder_oracle(oracle), 2, N)


# ---- the rank limit: 512 copies are ranked in LDS, 513 go to k_rest<TB> ---------------------------

def _rank_limit_inputs():
    rng = np.random.default_rng(12)
    shapes = [make_shape(latency_ns=MS, bandwidth_bps=1_000_000_000) for _ in range(N)]
    per = np.arange(N) % 3
    per[30], per[700] = 512, 513
    windows, ends = [], []
    for w in range(2):
        if w == 1:
            per = np.arange(N) % 3
        src = np.repeat(np.arange(N), per)
        dst = rng.integers(0, N, len(src))
        dst[dst == src] = (dst[dst == src] + 1) % N
        seq = w * 1024 + np.concatenate([np.arange(k) for k in per])
        windows.append((src, dst, seq, np.full(len(src), 1000), w * 10 * MS + rng.integers(0, 2 * MS, len(src))))
        ends.append((w + 1) * 10 * MS)
    windows.append(None)
    ends.append(200 * MS)
    return shapes, windows, ends


def _rank_limit_oracle(oracle):
    if "rank" not in _cache:
        _cache["rank"] = _run_single(oracle, *_rank_limit_inputs(), seed=22)
    return _cache["rank"]


def _check_rank_limit_claims(out):
    d = out[0]["deliv"]  # 1 ms of latency, 8 us a packet: the first window delivers all it sent
    copies = np.bincount(d["src"], minlength=N)
    assert copies[30] == 512 and copies[700] == 513, (copies[30], copies[700])
    assert copies.sum() == 512 + 513 + (np.arange(N) % 3).sum() - 30 % 3 - 700 % 3  # no loss, no duplicates


def test_rank_limit_claims(oracle):
    _check_rank_limit_claims(_rank_limit_oracle(oracle))


@pytest.mark.gpu
def test_rank_limit_boundary(hip, oracle):
    kc = []
    a = _run_single(hip, *_rank_limit_inputs(), seed=22, counters=kc)
    S.assert_same(a, _rank_limit_oracle(oracle))
    assert kc[0]["long_tb"] == 513 and kc[-1]["long_tb"] == 513, kc  # the 513 sender's copies, nothing else


# ---- the item capacity: 1536 items fused, 1537 in the global form, an empty bucket ---------------

def _capacity_inputs():
    """Senders 0-23 (bucket 0) send 64 each = 1536; senders 24-47 (bucket 1) 64 each and one more =
    1537; senders 48-71 (bucket 2) nothing. Sender g's messages go to receiver g + 600, so receiver
    buckets 25, 26 and 27 hold 1536, 1537 and 0 deliveries; receivers 48-71 get nothing either."""
    rng = np.random.default_rng(13)
    shapes = [make_shape(latency_ns=MS, bandwidth_bps=10_000_000_000) for _ in range(N)]
    per = np.zeros(N, np.int64)
    per[:48] = 64
    per[24] = 65
    per[100:600] = 2
    src = np.repeat(np.arange(N), per)
    dst = np.where(src < 48, src + 600, 700 + src % 400)
    seq = np.concatenate([np.arange(k) for k in per])
    windows = [(src, dst, seq, np.full(len(src), 100), rng.integers(0, 2 * MS, len(src))), None]
    return shapes, windows, [10 * MS, 100 * MS]


def _capacity_oracle(oracle):
    if "cap" not in _cache:
        _cache["cap"] = _run_single(oracle, *_capacity_inputs(), seed=23)
    return _cache["cap"]


def _check_capacity_claims(out):
    d = out[0]["deliv"]
    by_src = np.bincount(d["src"] // KEYS, minlength=N // KEYS)
    by_dst = np.bincount(d["dst"] // KEYS, minlength=N // KEYS)
    assert (by_src[0], by_src[1], by_src[2]) == (1536, 1537, 0), by_src[:3]
    assert (by_dst[25], by_dst[26], by_dst[27], by_dst[2]) == (1536, 1537, 0, 0), by_dst
    assert len(out[1]["deliv"]["src"]) == 0  # everything left in the first window


def test_capacity_claims(oracle):
    _check_capacity_claims(_capacity_oracle(oracle))


@pytest.mark.gpu
def test_capacity_boundary(hip, oracle):
    kc = []
    a = _run_single(hip, *_capacity_inputs(), seed=23, counters=kc)
    S.assert_same(a, _capacity_oracle(oracle))
    # every key of an over-full bucket goes to k_rest, no key of a full one does
    assert kc[-1]["long_tb"] == 1537 and kc[-1]["long_emit"] == 1537, kc


# ---- a bucket whose times span more than 2^32 ns ---------------------------------------------------

def _wide_span_inputs():
    """One window of 6 s. Sender 100 has 5 s of latency, its bucket neighbours (96-119) 1 ms; its 24
    messages go to receivers 240-263 (bucket 10), which also hear from the others."""
    rng = np.random.default_rng(14)
    shapes = [make_shape(latency_ns=5000 * MS if g == 100 else MS, bandwidth_bps=1_000_000_000) for g in range(N)]
    per = np.full(N, 5)
    per[100] = 24
    src = np.repeat(np.arange(N), per)
    dst = rng.integers(0, N, len(src))
    dst[src == 100] = 240 + np.arange(24)
    dst[(src >= 96) & (src < 120) & (src != 100)] = 240 + rng.integers(0, 24, int(((src >= 96) & (src < 120)).sum()) - 24)
    dst[dst == src] = (dst[dst == src] + 1) % N
    seq = np.concatenate([np.arange(k) for k in per])
    windows = [(src, dst, seq, np.full(len(src), 1000), rng.integers(0, 100 * MS, len(src))), None]
    return shapes, windows, [6000 * MS, 6100 * MS]


def _wide_span_oracle(oracle):
    if "wide" not in _cache:
        _cache["wide"] = _run_single(oracle, *_wide_span_inputs(), seed=24)
    return _cache["wide"]


def _check_wide_span_claims(out):
    d = out[0]["deliv"]
    t = d["t_deliver"]
    for m in (d["src"] // KEYS == 100 // KEYS, d["dst"] // KEYS == 10):
        assert int(t[m].max()) - int(t[m].min()) > 1 << 32
    assert len(out[1]["deliv"]["src"]) == 0


def test_wide_span_claims(oracle):
    _check_wide_span_claims(_wide_span_oracle(oracle))


@pytest.mark.gpu
def test_wide_span_bucket(hip, oracle):
    S.assert_same(_run_single(hip, *_wide_span_inputs(), seed=24), _wide_span_oracle(oracle))
