// legacy_mt.h — NumPy's legacy RandomState restated for the host cores, shared
// by libsparc_amp.so (sa_draw_reps, sa_make_ordering) and libldpc_bp.so
// (lb_draw_blocks).  Host code only.
#ifndef LEGACY_MT_H
#define LEGACY_MT_H

#include <cmath>
#include <cstdint>

namespace legacy_rng {

// ---- NumPy legacy RandomState, restated ------------------------------------
// (numpy/random: mt19937_seed, mt19937_next32 / next_double,
// buffered_bounded_masked_uint32, legacy_gauss; the published MT19937 of
// Matsumoto & Nishimura.)  Plain IEEE binary64 operations in NumPy's order
// and the C library's log / sqrt, no contraction: the same bits.
struct LegacyMT {
  uint32_t key[624];
  int pos = 624;
  bool has_gauss = false;
  double gauss = 0.0;

  explicit LegacyMT(uint32_t seed) {
    key[0] = seed;
    for (int i = 1; i < 624; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
  }
  void twist() {
    constexpr uint32_t U = 0x80000000u, Lo = 0x7fffffffu, A = 0x9908b0dfu;
    int i = 0;
    for (; i < 624 - 397; ++i) {
      const uint32_t y = (key[i] & U) | (key[i + 1] & Lo);
      key[i] = key[i + 397] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    }
    for (; i < 623; ++i) {
      const uint32_t y = (key[i] & U) | (key[i + 1] & Lo);
      key[i] = key[i + 397 - 624] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    }
    const uint32_t y = (key[623] & U) | (key[0] & Lo);
    key[623] = key[396] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    pos = 0;
  }
  uint32_t next32() {
    if (pos == 624) twist();
    uint32_t y = key[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  double next_double() {
#pragma clang fp contract(off)
    const int32_t a = (int32_t)(next32() >> 5), b = (int32_t)(next32() >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
  }
  // randint(0, M) of the legacy generator: the smallest all-ones mask over
  // M - 1, rejection of the masked 32-bit draws above M - 1
  int32_t bounded(uint32_t rng) {
    if (rng == 0) return 0;  // no draw
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v;
    while ((v = next32() & mask) > rng) {
    }
    return (int32_t)v;
  }
  double gaussian() {  // legacy_gauss: the polar method, the second value kept
#pragma clang fp contract(off)
    if (has_gauss) {
      has_gauss = false;
      const double t = gauss;
      gauss = 0.0;
      return t;
    }
    double x1, x2, r2;
    do {
      x1 = 2.0 * next_double() - 1.0;
      x2 = 2.0 * next_double() - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double f = std::sqrt(-2.0 * std::log(r2) / r2);
    gauss = f * x1;
    has_gauss = true;
    return f * x2;
  }
};

}  // namespace legacy_rng

#endif  // LEGACY_MT_H
