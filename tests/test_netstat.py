"""GPU: netstat's device counters equal the numpy reduction of the CPU oracle's per-window outputs
(tests/netstat_cases.py) exactly, after every window, on every staging path and run structure."""
import ctypes as C

import numpy as np
import pytest

from testground_amd import _abi as A
from testground_amd.sim import SimConfig, Simulator, make_shape
from tests import netstat_cases as NC
from tests import scenarios as S

pytestmark = pytest.mark.gpu
MS = S.MS


def _enable(sim):
    sim.netstat_enable()


def _checker(ref, n_inst, lo=0, hi=None):
    """on_window hook: after window w the counters equal the reference accumulated over ref[0..w]."""
    acc = NC.empty(n_inst)

    def on_window(w, sim, win):
        x = ref[w]
        NC.add_window(acc, x["src"], x["size"], x["status"], x["deliv"])
        NC.assert_rows(sim.netstat(), acc, lo, hi, f"after window {w}")
    return on_window


def _run_checked(hip, name, n_inst):
    ref = NC.oracle_run(name)
    got = NC.DRIVERS[name](hip, _enable, _checker(ref, n_inst))
    assert len(got) == len(ref)


def test_random_windows(hip):
    _run_checked(hip, "random", 24)


@pytest.mark.parametrize("kind", NC.TX_RUN_KINDS)
def test_tx_run_structure(hip, kind):
    _run_checked(hip, "tx_" + kind, 16)


def test_queue_limit_bursts(hip):
    _run_checked(hip, "burst", 10)


def test_long_inbox(hip):
    _run_checked(hip, "long_inbox", 64)


def test_storm_rounds_at_the_device_clock(hip, oracle):
    """bench.py's loop: rounds at TGSIM_T_NOW, the next one generated inside the window end's last
    launch - over the staged arrays the TX pass reads, so the pass must have run before it."""
    n, rounds = 300, 6
    ref = NC.storm_windows(S.run_storm(oracle, n_inst=n, rounds=rounds, t_now=True))
    seen = []

    def collect(r, sim):
        seen.append(sim.netstat())
        return sim
    S.run_storm(hip, n_inst=n, rounds=rounds, t_now=True, setup=_enable, restart=collect)
    acc = NC.empty(n)
    assert len(seen) == rounds == len(ref)
    for r, x in enumerate(ref):
        assert len(x["status"]) == n * 8
        NC.add_window(acc, x["src"], x["size"], x["status"], x["deliv"])
        NC.assert_rows(seen[r], acc, what=f"after round {r}")


@pytest.mark.parametrize("shift", [0, 1])
def test_enqueue_device_in_place(hip, oracle, shift):
    """A torch device batch as the window's first (and only) staging is read in place: the TX pass
    reads the caller's arrays too - 16-byte aligned (shift 0) or not (shift 1: the scalar-load form)."""
    import torch
    dev = torch.device("cuda:0")
    n_inst, n = 8, 2503
    rng = np.random.default_rng(41 + shift)
    sims = [Simulator(SimConfig(n_instances=n_inst, seed=9), binding=b) for b in (hip, oracle)]
    sims[0].netstat_enable()
    for sm in sims:
        for g in range(n_inst):
            sm.set_shape(g, make_shape(latency_ns=(1 + g % 4) * MS, jitter_ns=300_000, loss=5.0, duplicate=5.0))
    acc = NC.empty(n_inst)
    for w in range(3):
        src = rng.integers(0, n_inst, n)
        dst = rng.integers(0, n_inst, n)
        seq = np.arange(n) + w * n
        size = rng.choice([0, 100, 1500], n)
        t = w * 2 * MS + np.sort(rng.integers(0, 2 * MS, n))
        pad = np.zeros(shift, np.int64)
        cols = [torch.from_numpy(np.r_[pad, x].astype(np.int32)).to(dev) for x in (src, dst, seq, size)]
        cols.append(torch.from_numpy(np.r_[pad, t].astype(np.int64)).to(dev))
        torch.cuda.synchronize()
        sims[0].enqueue_device(*(c[shift:].data_ptr() for c in cols), n)
        sims[1].enqueue(src, dst, seq, size, t)
        for sm in sims:
            sm.advance((w + 1) * 2 * MS)
        NC.add_window(acc, src, size, sims[1].status(), sims[1].deliveries())
        NC.assert_rows(sims[0].netstat(), acc, what=f"after window {w}")
        del cols
    for sm in sims:
        sm.close()


def test_flood_device_counted_staging(hip, oracle):
    """The flood's forwards are staged on the device behind a device-side count: RX per window against
    the oracle's deliveries; TX per sender at the end - nothing is lost, so a sender's messages are
    the deliveries that name it as source."""
    n = 300
    shapes = [make_shape(latency_ns=(10 + 7 * (g % 5)) * MS) for g in range(n)]
    kw = dict(n_inst=n, pubs_per_wave=1, waves=1, degree=4, shapes=shapes, size=512)
    ref = S.run_flood(oracle, **kw)
    box, seen = {}, []
    got = S.run_flood(hip, setup=lambda sim: (box.update(sim=sim), sim.netstat_enable()),
                      on_window=lambda w, d, fwd: seen.append(box["sim"].netstat()), **kw)
    assert len(got) == len(ref) == len(seen) + 1 and ref[-1]["tot"]["delivered"] > n
    acc = NC.empty(n)
    none = np.zeros(0, np.int64)
    for w, x in enumerate(ref[:-1]):
        NC.add_window(acc, none, none, none, x["deliv"])
        for f in A.NETSTAT_FIELDS:
            if f.startswith("rx_"):
                assert np.array_equal(seen[w][f], acc[f]), (w, f)
    by_src = np.bincount(np.concatenate([x["deliv"]["src"] for x in ref[:-1]]), minlength=n)
    assert np.array_equal(seen[-1]["tx_msgs"], by_src.astype(np.uint64))
    assert np.array_equal(seen[-1]["tx_bytes"], (by_src * 512).astype(np.uint64))
    assert np.array_equal(seen[-1]["tx_status"][:, A.ST_QUEUED], by_src.astype(np.uint64))


def test_two_shards_in_one_process(hip, oracle):
    """Each shard keeps the rows of its own [lo, hi): they equal the single run's reference rows."""
    n_inst, world = 25, 2
    ref = NC.drv_random(oracle, n_inst=n_inst)
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def make(cfg):
        sim = Simulator(cfg, binding=hip)
        sim.netstat_enable()
        return sim

    def exchange(sims):  # device-to-device block copies between the contexts' exchange buffers
        bufs = [s.exchange_buffers() for s in sims]
        blk = bufs[0][2] // len(sims)
        for s in sims:
            s.sync()
        for q in range(len(sims)):
            for p in range(len(sims)):
                assert hiprt.hipMemcpy(bufs[p][1] + q * blk, bufs[q][0] + p * blk, blk, 3) == 0
        assert hiprt.hipDeviceSynchronize() == 0

    acc = NC.empty(n_inst)

    def on_window(w, sims):
        x = ref[w]
        NC.add_window(acc, x["src"], x["size"], x["status"], x["deliv"])
        for s in sims:
            NC.assert_rows(s.netstat(), acc, s.lo, s.hi, f"shard [{s.lo}, {s.hi}) after window {w}")
            with pytest.raises(A.TgsimError) as e:   # rows of another shard
                s.netstat(first=s.lo - 1 if s.lo else s.hi - 1, n=2)
            assert e.value.code == A.EINVAL
    NC.drv_random_sharded(make, exchange, world, on_window, n_inst=n_inst)


def test_enable_freeze_reset(hip):
    """Counting starts with the first window after enabling, on = 0 freezes the values, reset zeroes
    them; a context that never enables netstat computes what the oracle does and has no counters."""
    ref = NC.oracle_run("random")
    acc, zero = NC.empty(24), NC.empty(24)

    def on_window(w, sim, win):
        S.assert_same(dict(status=win["status"], deliv=win["deliv"]),
                      dict(status=ref[w]["status"], deliv=ref[w]["deliv"]), f"window {w}")
        if w < 2:       # never enabled so far
            for call in (sim.netstat, sim.netstat_reset, sim.netstat_device):
                with pytest.raises(A.TgsimError) as e:
                    call()
                assert e.value.code == A.ESTATE
        if w == 1:
            sim.netstat_enable()
            NC.assert_rows(sim.netstat(), zero, what="just enabled")
        if 2 <= w < 5:
            NC.add_window(acc, ref[w]["src"], ref[w]["size"], ref[w]["status"], ref[w]["deliv"])
        if w >= 2:
            NC.assert_rows(sim.netstat(), acc, what=f"after window {w}")
        if w == 4:
            sim.netstat_enable(False)
        if w == 7:
            assert acc["rx_packets"].sum() > 0 and (acc["rx_t_last"] > NC.I64_MIN).any()
            ptrs = sim.netstat_device()
            assert set(ptrs) == set(A.NETSTAT_FIELDS) and all(ptrs.values()) and len(set(ptrs.values())) == 15
            sim.netstat_reset()
            NC.assert_rows(sim.netstat(), zero, what="after reset")
            NC.assert_rows(sim.netstat(first=3, n=5), zero, 3, 8, what="a range")
            for first, n in ((24, 1), (20, 5), (0, 25)):
                with pytest.raises(A.TgsimError) as e:
                    sim.netstat(first=first, n=n)
                assert e.value.code == A.EINVAL
            assert len(sim.netstat(first=24, n=0)["tx_msgs"]) == 0
            for k in list(acc):
                acc[k] = zero[k].copy()
    NC.drv_random(hip, None, on_window)


def test_never_enabled_context_equals_the_oracle(hip):
    """Netstat is off by default: such a context's windows and statistics are the oracle's."""
    ref = NC.oracle_run("random")
    got = NC.drv_random(hip)
    S.assert_same([dict(status=x["status"], deliv=x["deliv"]) for x in got[:-1]],
                  [dict(status=x["status"], deliv=x["deliv"]) for x in ref[:-1]])
    for k in ("msgs_in", "copies", "lost", "dropped", "rejected", "unreachable", "external", "dest_down",
              "local", "delivered", "overlimit"):
        assert got[-1]["stats"][k] == ref[-1]["stats"][k], k


def test_enable_inside_a_window_is_refused(hip):
    sim = Simulator(SimConfig(n_instances=4, seed=3), binding=hip)
    sim.advance_begin(MS)
    for call in (lambda: sim.netstat_enable(), lambda: sim.netstat_enable(False)):
        with pytest.raises(A.TgsimError) as e:
            call()
        assert e.value.code == A.ESTATE
    sim.advance_end()
    sim.netstat_enable()
    sim.advance_begin(2 * MS)
    with pytest.raises(A.TgsimError) as e:
        sim.netstat_enable(False)
    assert e.value.code == A.ESTATE
    sim.advance_end()
    sim.close()


def test_snapshot_carries_the_counters(hip):
    """Snapshot after window 2 with copies in flight, destroy, restore into a fresh context that
    enabled netstat, continue: every later window's counters equal the uninterrupted reference. The
    image restores only into a context that enabled netstat, and a plain image only into one that did not."""
    ref = NC.oracle_run("random")
    check = _checker(ref, 24)
    sizes = {}

    def on_window(w, sim, win):
        check(w, sim, win)
        if w != 2:
            return None
        assert sim.stats()["inflight"] > 0
        image, cfg = sim.snapshot(), sim.cfg
        sim.close()
        plain = Simulator(cfg, binding=hip)
        sizes["plain"] = len(plain.snapshot())
        with pytest.raises(A.TgsimError) as e:
            plain.restore(image)
        assert e.value.code == A.EINVAL
        plain_image = plain.snapshot()
        plain.close()
        new = Simulator(cfg, binding=hip)
        new.netstat_enable()
        with pytest.raises(A.TgsimError) as e:
            new.restore(plain_image)
        assert e.value.code == A.EINVAL
        sizes["netstat"] = len(new.snapshot())
        new.restore(image)
        NC.assert_rows(new.netstat(), NC.reduce_windows(ref[:3], 24), what="restored")
        return new
    NC.drv_random(hip, _enable, on_window)
    assert sizes["netstat"] - sizes["plain"] == 24 * (13 + 9 + 1) * 8   # the counters are all the image gains
