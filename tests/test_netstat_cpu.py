"""CPU: netstat's ABI surface, its device source's static checks, and the reference the GPU tests use.

* the library exports every function include/tgsim_netstat.h declares and the ctypes binding has them;
* tgsim_netstat_soa's ctypes mirror has the C compiler's size and offsets;
* tgsim_netstat.hip compiles for gfx950 and tools/loopexit_audit.py finds nothing in it;
* on the CPU oracle alone: the reference reducer's sums equal the tgsim_stats deltas for every driver
  of tests/netstat_cases.py, and the drivers reach the cases they are there for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from testground_amd import _abi as A
from tests import netstat_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tgsim_netstat.h")
HIPCC = "/opt/rocm/bin/hipcc"


def test_library_exports_and_binds_the_netstat_header():
    syms = A.header_symbols(HEADER)
    assert {"tgsim_netstat_enable", "tgsim_netstat_reset", "tgsim_netstat_copy", "tgsim_netstat_device"} <= set(syms)
    assert os.path.exists(A.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = C.CDLL(A.LIB_PATH)
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    bound = {"tgsim_" + k for k in list(A._SIGS) + list(A._SIGS_HIP)}
    assert set(syms) <= bound, set(syms) - bound
    hip = A.hip_library()
    for s in syms:
        assert callable(getattr(hip, s[len("tgsim_"):]))
    # the facility has no CPU meaning: tgsim.h (whose every function needs an oracle twin) does not declare it
    assert not [s for s in A.header_symbols() if "netstat" in s]
    names = [hip.kernel_name(k).decode() for k in range(hip.kernel_classes())]
    assert names[-1] == "k_netstat" and hip.abi_version() == 2


def test_netstat_soa_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tgsim_netstat.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(tgsim_netstat_soa));', f'  printf("codes %d\\n", TGSIM_NETSTAT_CODES);']
    for f, _ in A.NetstatSoA._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(tgsim_netstat_soa, {f}));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(A.NetstatSoA) and int(got["codes"]) == A.NETSTAT_CODES
    assert len(got) == 2 + len(A.NETSTAT_FIELDS)
    for f, _ in A.NetstatSoA._fields_:
        assert int(got[f]) == getattr(A.NetstatSoA, f).offset, f


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_netstat_source_compiles_and_passes_the_loop_exit_audit(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loopexit_audit as LA
    out = tmp_path / "tgsim_netstat.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S", "-o",
                           str(out), os.path.join(ROOT, "testground_amd", "csrc", "tgsim_netstat.hip")],
                          stderr=subprocess.DEVNULL)
    assert LA.audit(str(out)) == []
    txt = out.read_text()
    assert "k_netstat_tx" in txt and "k_netstat_rx" in txt
    assert "global_atomic_add_x2" in txt and "cmpswap" not in txt   # 64-bit adds, no compare-and-swap loop
    assert "scratch_" not in txt                                      # nothing spills


@pytest.mark.parametrize("name", sorted(NC.DRIVERS))
def test_reference_sums_equal_the_stats_deltas(name):
    run = NC.oracle_run(name)
    stats = run[-1]["stats"]
    n_inst = dict(random=24, burst=10, long_inbox=64).get(name, 16)
    acc = NC.reduce_windows(run[:-1], n_inst)
    assert NC.stats_sums(acc) == {k: stats[k] for k in NC.stats_sums(acc)}
    assert int(acc["tx_status"].sum()) == stats["msgs_in"] and (acc["tx_status"].sum(axis=1) == acc["tx_msgs"]).all()


def _codes(run):
    st = np.concatenate([w["status"] for w in run[:-1]])
    return np.bincount(st & 0x0F, minlength=A.NETSTAT_CODES), st


def _delivery_flags(run):
    return np.concatenate([w["deliv"]["flags"] for w in run[:-1]])


def test_random_case_reaches_what_it_claims():
    run = NC.oracle_run("random")
    codes, _ = _codes(run)
    assert (codes[:8] > 0).all(), codes                      # every code QUEUED .. LOCAL
    fl = _delivery_flags(run)
    for bit in (A.F_CLONE, A.F_CORRUPT, A.F_REORDERED, A.F_LOCAL):
        assert (fl & bit).any(), bit
    sizes = np.concatenate([w["size"] for w in run[:-1]])
    assert (sizes == 0).any() and (sizes == 65536).any()
    assert any(len(w["src"]) == 0 for w in run[:-1])          # a window with no staged message
    assert any(len(w["deliv"]["dst"]) == 0 for w in run[:-1])  # a window with no delivery
    assert any(len(w["src"]) == 0 and len(w["deliv"]["dst"]) > 0 for w in run[:-1])  # late deliveries alone


def test_burst_case_reaches_what_it_claims():
    codes, st = _codes(NC.oracle_run("burst"))
    assert codes[A.ST_OVERLIMIT] > 1000, codes
    for bit in (A.ST_FLAG_DUP, A.ST_FLAG_CLONE_LOST, A.ST_FLAG_DUP_CANCEL, A.ST_FLAG_OVERLIMIT):
        assert (st & bit).any(), hex(bit)


def test_long_inbox_case_reaches_what_it_claims():
    run = NC.oracle_run("long_inbox")
    per = np.bincount(run[0]["deliv"]["dst"], minlength=64)
    assert per.max() > 8192 and np.sort(per)[-2] <= 2 and (per == 0).any()


def test_tx_run_cases_reach_what_they_claim():
    for kind, n in (("random", 3001), ("sorted1000", 6037), ("one_sender", 4099), ("single", 1)):
        src = NC.oracle_run("tx_" + kind)[0]["src"]
        assert len(src) == n and n % 4 and n % 64 and n % 256
    src = NC.oracle_run("tx_sorted1000")[0]["src"]
    runs = np.diff(np.flatnonzero(np.r_[True, src[1:] != src[:-1], True]))
    assert runs.max() == 1000 and len(runs) == 7
    assert len(set(NC.oracle_run("tx_one_sender")[0]["src"])) == 1
    codes, _ = _codes(NC.oracle_run("tx_one_sender"))
    assert codes[A.ST_OVERLIMIT] > 0   # 4099 messages of one sender overrun the 1000-packet queue
