"""The A / D / L queue appends (Queues::push_batch, Queues::push and k_tb_bucket's staged output),
HIP against the oracle, at the shapes where a wrong base, key or position would show: neighbouring
lanes of one wave appending to all three queues at once, times on both sides of 2^32 ns (where the
old slot division took another path), wheel slot widths that are no power of two, a power of two,
above 2^32, and an 8-slot wheel whose clamped last slot re-inserts, and the same through the
exchange on two shards of one device. 1200 instances (24 keys per bucket, 50 buckets), a few thousand
messages a window. Every scenario also checks on the oracle's output alone what it claims to produce.

The traffic: sender g has shape g % 4 - 0: 1 ms of latency, unlimited; 1: 1 ms, 1 Mbit/s; 2: 50 ms,
unlimited; 3: 50 ms, 1 Mbit/s - and duplicates 50 %, three 10 ms windows and a drain. Messages are
in sender order, so neighbouring lanes of the netem pass take D (shape 0), A (1 and 3) and L (2) in
one push_batch<2>; the windows after the first extract wheel records that go to A, D and back to L
in one push_batch<4>.

What the issue claimed for this traffic - every window but the drain holds deliveries of both
unlimited classes - cannot hold as written: 50 ms of latency against 30 ms of windows puts every
delivery of shape 2 into the drain. The claim asserted here is what the traffic does give: every
window but the drain holds deliveries of the 1 ms unlimited class, the 50 ms unlimited class is
delivered in the drain exactly 50 ms after it was sent (it crossed the wheel), and the limited
senders' deliveries run past the end of the window they were sent in. test_long_run adds ten
windows of the same traffic, where windows 5-9 do hold deliveries of every class."""
import numpy as np
import pytest

from testground_amd.sim import SimConfig, Simulator, make_shape

from tests import scenarios as S

MS = S.MS
N = 1200
SEQ_STRIDE = 16   # seq = window * SEQ_STRIDE + index: a delivery names the window it was sent in
W = 10 * MS
TWO32 = 1 << 32


def _shapes():
    return [make_shape(latency_ns=(1 if g % 4 < 2 else 50) * MS, duplicate=50.0,
                       bandwidth_bps=1_000_000 if g % 2 else 0) for g in range(N)]


def _traffic(t0, n_send, n_win, drain):
    """n_send windows of messages from t0 on (sender g: 1 + g % 3 a window, sent in the first 9 ms),
    n_win windows of 10 ms in all, then one drain window of `drain` ns."""
    rng = np.random.default_rng(31)
    per = 1 + np.arange(N) % 3
    src = np.repeat(np.arange(N), per)
    idx = np.concatenate([np.arange(k) for k in per])
    windows, ends = [], []
    for w in range(n_win):
        if w < n_send:
            dst = rng.integers(0, N, len(src))
            dst[dst == src] = (dst[dst == src] + 1) % N
            windows.append((src, dst, w * SEQ_STRIDE + idx, np.full(len(src), 1000),
                            t0 + w * W + rng.integers(0, 9 * MS, len(src))))
        else:
            windows.append(None)
        ends.append(t0 + (w + 1) * W)
    windows.append(None)
    ends.append(t0 + n_win * W + drain)
    return windows, ends


def _drive(sims, ranges, exchange, windows, ends):
    """Per context, after every window: clock, statuses, deliveries, inbox offsets and stats."""
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
            o.append(dict(now=s.now, status=s.status(), deliv=s.deliveries(), inbox=s.inbox_offsets(),
                          stats=S.parity_stats(s)))
    for s in sims:
        s.close()
    return outs


def _run_single(binding, windows, ends, **cfg):
    sim = Simulator(SimConfig(n_instances=N, seed=41, max_msgs_per_window=1 << 16, max_records=1 << 18, **cfg),
                    binding=binding)
    sim.set_shapes(np.arange(N), _shapes())
    return _drive([sim], [(0, N)], None, windows, ends)[0]


# A drain of 2 s: the slowest limited sender holds 3 windows * 3 messages * 2 copies of 8 ms each.
DRAIN = 2000 * MS
BASE = (0, 3, 3, DRAIN)

_cache = {}


def _oracle_run(oracle, name, make):
    if name not in _cache:
        windows, ends = make()
        _cache[name] = _run_single(oracle, windows, ends)
    return _cache[name]


def _base_oracle(oracle):
    return _oracle_run(oracle, "base", lambda: _traffic(*BASE))


def _sent_in(x, t0):
    """End of the window a delivery was sent in."""
    return t0 + ((x["seq"].astype(np.int64) // SEQ_STRIDE) + 1) * W


def _check_base_claims(out, t0=0, n_win=3):
    late_limited = 0
    for w in out[:n_win]:
        x = w["deliv"]
        assert ((x["src"] % 4 == 0)).any()                       # the 1 ms unlimited class, every window
        assert not (x["src"] % 4 == 2).any()                     # 50 ms of latency: none before the drain
        late_limited += int(((x["src"] % 2 == 1) & (x["t_deliver"] >= _sent_in(x, t0))).sum())
    x = out[n_win]["deliv"]
    far = x["src"] % 4 == 2
    assert far.any() and (x["t_deliver"][far] >= t0 + 50 * MS).all() and (x["t_deliver"][far] < t0 + 79 * MS).all()
    late_limited += int(((x["src"] % 2 == 1) & (x["t_deliver"] >= _sent_in(x, t0))).sum())
    assert late_limited > 0
    # every queue took records: deliveries in the window they were sent in (D from the netem pass),
    # limited ones (A), and ones that waited in the wheel (L)
    assert (out[0]["deliv"]["src"] % 4 == 1).any()


def test_base_claims(oracle):
    _check_base_claims(_base_oracle(oracle))


@pytest.mark.gpu
def test_three_queues_in_one_wave(hip, oracle):
    windows, ends = _traffic(*BASE)
    S.assert_same(_run_single(hip, windows, ends), _base_oracle(oracle))


# ---- ten windows: the extraction appends to A, D and L in one batch --------------------------------

LONG = (0, 10, 10, DRAIN)


def _long_oracle(oracle):
    return _oracle_run(oracle, "long", lambda: _traffic(*LONG))


def _check_long_claims(out):
    for w in out[5:10]:
        x = w["deliv"]
        for c in range(4):
            assert (x["src"] % 4 == c).any(), c


def test_long_claims(oracle):
    _check_long_claims(_long_oracle(oracle))


@pytest.mark.gpu
def test_long_run(hip, oracle):
    windows, ends = _traffic(*LONG)
    S.assert_same(_run_single(hip, windows, ends), _long_oracle(oracle))


# ---- times across 2^32 ns ---------------------------------------------------------------------------

def _late_traffic():
    """Empty windows to 4 280 ms, then the base traffic in 10 ms windows to 4 330 ms and the drain."""
    windows, ends = _traffic(4280 * MS, 3, 5, DRAIN)
    empty = [1000 * MS, 2000 * MS, 3000 * MS, 4280 * MS]
    return [None] * len(empty) + windows, empty + ends


def _late_oracle(oracle):
    return _oracle_run(oracle, "late", _late_traffic)


def _check_late_claims(out):
    for w in out[:4]:
        assert len(w["deliv"]["src"]) == 0
    t = out[5]["deliv"]["t_deliver"].astype(np.int64)  # the window [4 290 ms, 4 300 ms)
    assert (t < TWO32).any() and (t >= TWO32).any(), (t.min(), t.max())


def test_late_claims(oracle):
    _check_late_claims(_late_oracle(oracle))


@pytest.mark.gpu
def test_times_across_two_to_the_32(hip, oracle):
    windows, ends = _late_traffic()
    S.assert_same(_run_single(hip, windows, ends), _late_oracle(oracle))


# ---- slot widths --------------------------------------------------------------------------------------

WIDTHS = [dict(wheel_slot_ns=1_000_000), dict(wheel_slot_ns=3_000_000, wheel_slots=8), dict(wheel_slot_ns=999_983),
          dict(wheel_slot_ns=1 << 20), dict(wheel_slot_ns=(1 << 32) + 3)]


def _check_small_wheel_claim(out):
    """Some copy is delivered more than 8 * 3 ms after the end of the window it was sent in, with
    windows in between: it sat in the clamped last slot of the 8-slot wheel and was inserted again."""
    x = out[3]["deliv"]
    sent = _sent_in(x, 0)
    assert ((x["t_deliver"] > sent + 8 * 3 * MS) & (sent < 30 * MS)).any()


def test_small_wheel_claim(oracle):
    _check_small_wheel_claim(_base_oracle(oracle))


def test_oracle_ignores_the_wheel(oracle):
    """The wheel's geometry is not observable: one oracle run is the reference of every width."""
    windows, ends = _traffic(*BASE)
    S.assert_same(_run_single(oracle, windows, ends, wheel_slot_ns=3_000_000, wheel_slots=8), _base_oracle(oracle))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", WIDTHS, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_slot_widths(hip, oracle, cfg):
    windows, ends = _traffic(*BASE)
    S.assert_same(_run_single(hip, windows, ends, **cfg), _base_oracle(oracle))


# ---- two shards on one device ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_shards(hip, oracle):
    """The base traffic on two contexts of one device, through the exchange, against the single run."""
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

    windows, ends = _traffic(*BASE)
    sims = []
    for k in range(2):
        s = Simulator(SimConfig(n_instances=N, seed=41, max_msgs_per_window=1 << 16, max_records=1 << 18,
                                **S.shard_cfg(2, k, exchange_cap=1 << 15)), binding=hip)
        s.set_shapes(np.arange(N), _shapes())
        sims.append(s)
    outs = _drive(sims, [S.shard_range(N, k, 2) for k in range(2)], exchange, windows, ends)
    single = _base_oracle(oracle)
    # assert_storm_sharded reads the counters from a last element of their own
    S.assert_storm_sharded([o + [dict(stats=o[-1]["stats"])] for o in outs], single + [dict(stats=single[-1]["stats"])],
                           2, N)
    for r in range(len(single)):  # and the counters after every window
        tot = {}
        for o in outs:
            for name, v in o[r]["stats"].items():
                tot[name] = tot.get(name, 0) + v
        assert tot == single[r]["stats"], (r, tot, single[r]["stats"])
