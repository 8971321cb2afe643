// tgsim_slotdiv.h — n / d for a divisor that is fixed long before the quotient is needed (the
// timing-wheel slot width of a context, the storm's spread): a multiply-high and two shifts,
//   t = mulhi(m, n),  q = (t + ((n - t) >> sh1)) >> sh2,
// exact for every 64-bit n (Granlund & Montgomery 1994, fig. 4.1, at N = 64). The constants are made
// once on the host; the quotient is host and device code, so that a host program can check it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TG_SLOTDIV_HD __host__ __device__
#else
#define TG_SLOTDIV_HD
#endif

struct SlotDiv {
  uint64_t m;
  uint32_t sh1, sh2;
};

// l = ceil(log2 d), m = floor(2^64 (2^l - d) / d) + 1, sh1 = min(l, 1), sh2 = max(l - 1, 0), for
// 1 <= d <= 2^63 (every positive int64 and 2^63); d = 0 gives zeros (the quotient is then unused).
static inline SlotDiv slot_div_make(uint64_t d) {
  SlotDiv s = {0, 0, 0};
  if (d == 0) return s;
  uint32_t l = 0;
  while (l < 64 && ((uint64_t)1 << l) < d) ++l;
  const unsigned __int128 two_l = (unsigned __int128)1 << l;
  s.m = (uint64_t)((((unsigned __int128)1 << 64) * (two_l - d)) / d + 1);
  s.sh1 = l < 1 ? l : 1;
  s.sh2 = l > 1 ? l - 1 : 0;
  return s;
}

TG_SLOTDIV_HD static inline uint64_t slot_div_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(n / d), d the divisor s was made for.
TG_SLOTDIV_HD static inline uint64_t slot_div(const SlotDiv& s, uint64_t n) {
  const uint64_t t = slot_div_mulhi(s.m, n);
  return (t + ((n - t) >> s.sh1)) >> s.sh2;
}

// t / d as C++ divides int64 (towards zero), for every int64 t: the magnitude's quotient with the
// sign put back (2^63, the magnitude of INT64_MIN, is a valid numerator).
TG_SLOTDIV_HD static inline int64_t slot_div_signed(const SlotDiv& s, int64_t t) {
  const bool neg = t < 0;
  const uint64_t a = neg ? (uint64_t)0 - (uint64_t)t : (uint64_t)t;
  const uint64_t q = slot_div(s, a);
  return (int64_t)(neg ? (uint64_t)0 - q : q);
}

// The timing-wheel slot of a time relative to base_slot, clamped to [0, slots - 1]
// (Queues::key_of for an L record; here so that a host program can mirror it).
TG_SLOTDIV_HD static inline uint32_t slot_key(const SlotDiv& s, int64_t t, int64_t base_slot, uint32_t slots) {
  int64_t k = slot_div_signed(s, t) - base_slot;
  k = k < 0 ? 0 : (k > (int64_t)slots - 1 ? (int64_t)slots - 1 : k);
  return (uint32_t)k;
}
