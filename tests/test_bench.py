"""bench.py's command line beyond the timed region: --full gates the probe, and --dump-outputs writes
the last step's observables, the same from run to run and bounded in size (CPU oracle, no GPU)."""
import os
import sys

import numpy as np

import bench
from testground_amd._abi import T_NOW
from testground_amd.sim import Simulator


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default_and_sets_the_probe(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "40", "--warmup", "3")
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (40, 3)
    assert bench.probe_steps(a) == 10
    a = _args(monkeypatch, "--steps", "40", "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d" and bench.probe_steps(a) == 40
    assert bench.probe_steps(_args(monkeypatch, "--steps", "4", "--full")) == 10


def test_storm_context_has_a_sync_state_per_round(oracle, monkeypatch):
    """Every storm round's barrier is a sync state of its own: a run of more rounds than the default
    4096 states sizes its context for them (round 4999's barrier is then a valid state), a shorter
    one keeps the default."""
    a = _args(monkeypatch, "--instances", "50", "--max-records", str(1 << 16))
    assert bench.sim_config(a).max_states == 4096 and bench.sim_config(a, rounds=66).max_states == 4096
    cfg = bench.sim_config(a, rounds=5000)
    assert cfg.max_states == 5001
    sim = Simulator(cfg, binding=oracle)
    sim.gen_storm_round(4999, T_NOW, a.fanout, a.size, 10 * bench.MS, 4999)
    sim.advance_to_barrier(sim.barrier(4999, 50, T_NOW), bench.MS)
    assert sim.stats()["msgs_in"] == 50 * a.fanout
    sim.close()


def _storm_dump(oracle, monkeypatch, out_dir, n=400, rounds=12):
    a = _args(monkeypatch, "--instances", str(n), "--max-records", str(1 << 18))
    sim = Simulator(bench.sim_config(a), binding=oracle)
    sim.set_shapes(np.arange(n), bench.storm_shapes(n, a.seed))
    for r in range(rounds):
        sim.gen_storm_round(r, T_NOW, a.fanout, a.size, 10 * bench.MS, r)
        sim.advance_to_barrier(sim.barrier(r, n, T_NOW), bench.MS)
    want = dict(status=sim.status(), inbox_offsets=sim.inbox_offsets(), now=np.array([sim.now]),
                **{f"deliv_{k}": v for k, v in sim.deliveries().items()})
    bench.dump_outputs(sim, str(out_dir))
    sim.close()
    return want


def test_dump_outputs_whole_and_repeatable(oracle, monkeypatch, tmp_path):
    want = _storm_dump(oracle, monkeypatch, tmp_path / "a")
    _storm_dump(oracle, monkeypatch, tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in want)
    assert len(want["deliv_dst"]) > 2000 and len(want["status"]) == 400 * 8
    for k, v in want.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v.astype(np.float64)), k
        assert np.array_equal(got, np.load(tmp_path / "b" / (k + ".npy"))), k


def test_dump_outputs_samples_past_the_bound(oracle, monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "OUTPUT_BYTES", 10 * 8 * 1000)  # 1000 elements per array
    want = _storm_dump(oracle, monkeypatch, tmp_path / "a")
    _storm_dump(oracle, monkeypatch, tmp_path / "b")
    total = 0
    for k, v in want.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        total += got.nbytes
        assert len(got) == min(len(v), 1000), k
        assert np.array_equal(got, np.load(tmp_path / "b" / (k + ".npy"))), k
        if len(v) > 1000:  # the fixed sample: increasing positions of the whole array
            idx = np.sort(np.random.default_rng(0).choice(len(v), 1000, replace=False))
            assert np.array_equal(got, v[idx].astype(np.float64)), k
        else:
            assert np.array_equal(got, v.astype(np.float64)), k
    assert total <= 10 * 8 * 1000
