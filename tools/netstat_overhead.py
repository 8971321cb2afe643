#!/usr/bin/env python3
"""What netstat (include/tgsim_netstat.h) costs on bench.py's storm step.

Two contexts of bench.py's configuration (bench.sim_config, the storm loop at TGSIM_T_NOW) in one
process, one with netstat enabled and one without. After a warm-up, blocks of timed steps alternate
between them (each block ends in a synchronise), so both see the same machine state; the medians and
the spread of ms/step are reported for both. A separate profiled pass then gives k_netstat's average
launch time (HIP events around its two launches per step) and the launch counts per kernel class of
both contexts over 20 steps: the context without netstat must issue no k_netstat launch and the
same launches otherwise. Byte model of the passes: TX 9 B per staged message, RX 24 B per
delivery (with rx_t_last), plus the counter rows touched.

    python tools/netstat_overhead.py [--block 40 --alternations 6 --warmup 60] [bench.py's storm options]
Writes profiles/r07/netstat/overhead_storm.json and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=40, help="timed steps per block")
    ap.add_argument("--alternations", type=int, default=6, help="blocks per context (at least five)")
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "netstat", "overhead_storm.json"))
    a, rest = ap.parse_known_args()
    assert a.alternations >= 5
    import numpy as np
    import torch
    import bench
    from testground_amd._abi import T_NOW
    from testground_amd.sim import Simulator

    sys.argv = [sys.argv[0]] + rest
    args = bench.parse()
    assert args.workload == "storm" and not args.tcp and args.gpus == 1
    if not torch.cuda.is_available():
        raise SystemExit("netstat_overhead.py measures on the GPU: no HIP device")
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rounds = a.warmup + 2 * a.profile_steps + a.block * a.alternations + 1
    shapes = bench.storm_shapes(args.instances, args.seed)
    N, F = args.instances, args.fanout
    spread, rtt = int(args.spread_ms * bench.MS), int(args.rtt_ms * bench.MS)
    sims = {}
    for name in ("off", "on"):
        sim = Simulator(bench.sim_config(args, 0, 1, 0, rounds))
        sim.set_stream(stream.cuda_stream)
        sim.set_shapes(np.arange(sim.lo, sim.hi), shapes)
        if name == "on":
            sim.netstat_enable()
        sims[name] = sim
    nxt = dict(off=0, on=0)

    def steps(name, k):
        sim = sims[name]
        for r in range(nxt[name], nxt[name] + k):
            sim.gen_storm_round(r, T_NOW, F, args.size, spread, r)
            sim.advance_to_barrier(sim.barrier(r, N, T_NOW), rtt)
        nxt[name] += k
        sim.sync()

    for name in sims:
        steps(name, a.warmup)
    ms = dict(off=[], on=[])
    for i in range(a.alternations):
        for name in (("off", "on") if i % 2 == 0 else ("on", "off")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(name, a.block)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.block)
    # profiled passes, apart from the timing: all classes' launch counts, then k_netstat alone
    counts = {}
    for name, sim in sims.items():
        sim.profile(None)
        base = sim.profile_read()
        steps(name, a.profile_steps)
        now = sim.profile_read()
        counts[name] = {k: now[k][1] - base[k][1] for k in now if now[k][1] - base[k][1]}
        sim.profile([])
    on = sims["on"]
    s0 = on.stats()
    on.profile(["k_netstat"])
    base = on.profile_read()["k_netstat"]
    steps("on", a.profile_steps)
    got = on.profile_read()["k_netstat"]
    on.profile([])
    s1 = on.stats()
    launches = got[1] - base[1]
    k_ms = (got[0] - base[0]) / max(launches, 1)
    msgs = (s1["msgs_in"] - s0["msgs_in"]) / a.profile_steps
    deliv = (s1["delivered"] - s0["delivered"]) / a.profile_steps
    model_bytes = 9 * msgs + 24 * deliv
    per_step_ms = k_ms * launches / a.profile_steps
    ns = on.netstat()
    st = on.stats()
    assert int(ns["tx_msgs"].sum()) == st["msgs_in"] and int(ns["rx_packets"].sum()) == st["delivered"]

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), blocks=v)
    out = dict(
        workload="storm", instances=N, fanout=F, size=args.size, block_steps=a.block, alternations=a.alternations,
        warmup=a.warmup, ms_per_step=dict(netstat_off=summary(ms["off"]), netstat_on=summary(ms["on"])),
        delta_ms_per_step=statistics.median(ms["on"]) - statistics.median(ms["off"]),
        k_netstat=dict(launches_per_step=launches / a.profile_steps, avg_ms_per_launch=k_ms, ms_per_step=per_step_ms,
                       msgs_per_step=msgs, deliveries_per_step=deliv, model_bytes_per_step=model_bytes,
                       model_bytes_per_s=model_bytes / (per_step_ms * 1e-3) if per_step_ms else None),
        launches_per_class={k: v for k, v in counts.items()}, profile_steps=a.profile_steps,
        launch_counts_equal_but_netstat={k: v for k, v in counts["on"].items() if k != "k_netstat"} == counts["off"],
        device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    for sim in sims.values():
        sim.close()


if __name__ == "__main__":
    main()
