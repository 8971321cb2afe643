"""The division-free slot of a time (testground_amd/csrc/tgsim_slotdiv.h), checked by a stand-alone
host program built with -fsanitize=undefined: slot_div against n / d over the divisors and numerators
where a multiply-shift can go wrong (1, powers of two and their neighbours, every k d - 1 / k d /
k d + 1 up to the largest k that fits, 10^6 seeded 63-bit values per divisor), and the whole L key
(slot_key: signed quotient, base slot, clamp) against the expression it replaced for negative and
non-negative times. The same module compiles tgsim_kernels.hip for gfx950 and holds the two
append-heavy kernels to their register budgets."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "testground_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "tgsim_slotdiv.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // xorshift64*, seeded
static uint64_t rnd() {
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static long checked = 0, failed = 0;

static void check_div(const SlotDiv& s, uint64_t d, uint64_t n) {
  ++checked;
  const uint64_t got = slot_div(s, n), want = n / d;
  if (got != want) {
    if (failed++ < 10) std::printf("slot_div(%llu, %llu) = %llu, want %llu\n", (unsigned long long)n,
                                   (unsigned long long)d, (unsigned long long)got, (unsigned long long)want);
  }
}

// Queues::key_of for an L record as it was before the helper
static uint32_t old_key(int64_t t, int64_t slot_ns, int64_t base_slot, uint32_t slots) {
  int64_t s = t / slot_ns - base_slot;
  s = s < 0 ? 0 : (s > (int64_t)slots - 1 ? (int64_t)slots - 1 : s);
  return (uint32_t)s;
}

static void check_key(const SlotDiv& s, int64_t d, int64_t t) {
  static const uint32_t kSlots[3] = {1024, 8, 2};
  const int64_t q = t / d;
  for (int a = 0; a < 3; ++a) {
    const uint32_t slots = kSlots[a];
    // base slots that put the key below, on and above both clamps, and far away on either side
    const int64_t off[7] = {-2, 0, 1, (int64_t)slots - 2, (int64_t)slots - 1, (int64_t)slots + 5, 1 << 20};
    for (int b = 0; b < 7; ++b) {
      for (int sg = -1; sg <= 1; sg += 2) {
        // (a quotient near either end of int64 only takes base slots towards zero: the replaced
        // expression itself overflows beyond)
        const int64_t step = sg * off[b];
        if ((q > INT64_MAX / 2 && step < 0) || (q < INT64_MIN / 2 && step > 0)) continue;
        const int64_t base = q - step;
        ++checked;
        const uint32_t got = slot_key(s, t, base, slots), want = old_key(t, d, base, slots);
        if (got != want) {
          if (failed++ < 10) std::printf("slot_key(t=%lld, d=%lld, base=%lld, slots=%u) = %u, want %u\n", (long long)t,
                                         (long long)d, (long long)base, slots, got, want);
        }
      }
    }
  }
}

static void both(const SlotDiv& s, uint64_t d, uint64_t n) {
  check_div(s, d, n);
  if (n <= (uint64_t)INT64_MAX) {
    check_key(s, (int64_t)d, (int64_t)n);
    check_key(s, (int64_t)d, -(int64_t)n);
  }
}

int main() {
  const uint64_t ds[13] = {1, 2, 3, 7, 999983, 1000000, 3000000, 1ull << 20, (1ull << 32) - 1, 1ull << 32,
                           (1ull << 32) + 3, (1ull << 40) + 1, 1ull << 62};
  for (int i = 0; i < 13; ++i) {
    const uint64_t d = ds[i];
    const SlotDiv s = slot_div_make(d);
    both(s, d, 0);
    both(s, d, d - 1); both(s, d, d); both(s, d, d + 1);
    const uint64_t kmax = UINT64_MAX / d;  // the largest k with k d <= 2^64 - 1
    const uint64_t ks[6] = {2, 3, 1ull << 16, 1ull << 31, 1ull << 32, kmax};
    for (int j = 0; j < 6; ++j) {
      const uint64_t k = ks[j];
      if (k > kmax) continue;  // k d does not fit 64 bits
      const uint64_t kd = k * d;
      both(s, d, kd - 1); both(s, d, kd);
      if (kd != UINT64_MAX) both(s, d, kd + 1);
    }
    both(s, d, (1ull << 32) - 1); both(s, d, 1ull << 32); both(s, d, (uint64_t)INT64_MAX);
    check_div(s, d, UINT64_MAX); check_div(s, d, 1ull << 63);
    check_key(s, (int64_t)d, INT64_MIN);
    for (int r = 0; r < 1000000; ++r) {
      const uint64_t n = rnd() >> 1;  // 63 bits
      check_div(s, d, n);
      if ((r & 63) == 0) { check_key(s, (int64_t)d, (int64_t)n); check_key(s, (int64_t)d, -(int64_t)n); }
    }
  }
  std::printf("checked %ld failed %ld\n", checked, failed);
  return failed ? 1 : 0;
}
"""


def test_slot_div_matches_division(tmp_path):
    src = tmp_path / "slotdiv_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "slotdiv_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"checked (\d+) failed (\d+)", r.stdout)
    assert m and int(m.group(1)) > 13 * 1000000 and int(m.group(2)) == 0, r.stdout[-500:]


LDS_PER_CU = 160 * 1024  # gfx950


def _resource_usage(tmp_path):
    out = tmp_path / "tgsim_kernels.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "tgsim_kernels.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_append_kernels_keep_their_register_budgets(tmp_path):
    usage = _resource_usage(tmp_path)
    extract = {k: v for k, v in usage.items() if "k_extract_shapeILb" in k}
    assert len(extract) == 2, sorted(usage)
    for name, u in extract.items():
        print(name, u)
        assert u["VGPRs"] <= 96 and u["Occupancy"] == 5 and u["ScratchSize"] == 0, (name, u)
    tb = [v for k, v in usage.items() if "11k_tb_bucketE" in k]
    assert len(tb) == 1, sorted(usage)
    print("k_tb_bucket", tb[0])
    assert tb[0]["VGPRs"] <= 128 and tb[0]["ScratchSize"] == 0, tb[0]
    # its LDS is what it was (40208 bytes a workgroup): four workgroups share a CU
    assert tb[0]["LDS"] == 40208 and 4 * tb[0]["LDS"] <= LDS_PER_CU, tb[0]
    # the other appenders compile without scratch as well (k_shape_seq_wide had 92 bytes a lane
    # before this check existed and is held to that)
    for k, u in usage.items():
        if re.search(r"k_shapeE|k_extractE|11k_shape_seqE|6k_recvE|k_restINS_8TBPolicy|k_rest_local_hist", k):
            print(k, u)
            assert u["ScratchSize"] == 0, (k, u)
        if "k_shape_seq_wide" in k:
            print(k, u)
            assert u["ScratchSize"] <= 92, (k, u)
