// legacy_mt_dev.h — NumPy's legacy RandomState on the device: the twin of
// legacy_mt.h (host cores) for the kernels of sa_mc.hip and ldpc_mc.hip that
// draw a Monte-Carlo rep or an LDPC block from its seed.  Device code only.
//
// One workgroup of kThreads draws one seed's values.  The 624-word MT19937
// state lives in LDS; lane 0 seeds it (init_genrand, the integer seeding of
// LegacyMT's constructor), the twist runs as three parallel phases, and the
// tempered output words are kept two 624-word blocks at a time, so that word
// g of the generator's output stream is  w[(g / 624) & 1][g % 624]  for the
// two newest blocks.
//
// The stream is consumed by position, not by a running cursor:
//   * bounded integers whose range is its own mask (randint(0, M) with M a
//     power of two): draw l is word l & (M - 1), nothing is rejected;
//   * randn: polar-method trial j reads words base + 4 j .. base + 4 j + 3
//     whatever earlier trials did, is accepted when 0 < r2 < 1, and the a-th
//     accepted trial yields output 2 a (f x2) and output 2 a + 1 (f x1, the
//     value legacy_gauss caches).  A chunk of kTrials trials is one 624-word
//     span; the accept flags go through a workgroup prefix sum;
//   * random_sample: value i reads words base + 2 i, base + 2 i + 1.
// The floating-point operations are those of LegacyMT::next_double / gaussian
// in their order, no contraction.  Only log differs from the host's (the
// device library's against the C library's, both within an ulp).
#ifndef LEGACY_MT_DEV_H
#define LEGACY_MT_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace legacy_rng_dev {

constexpr int kThreads = 256;      // workgroup size of a drawing kernel
constexpr int kWords = 624;        // MT19937 state / output block
constexpr int kTrials = kWords / 4;   // polar trials per chunk
constexpr int kSamples = kWords / 2;  // random_sample values per chunk

struct State {
  uint32_t key[kWords];
  uint32_t w[2][kWords];  // tempered output blocks B - 1 and B, block b in w[b & 1]
  int cnt[kThreads / 64];
};

// chunks of kTrials trials after which randn gives up: four times what n
// values need at the polar method's acceptance of pi / 4 (no stream of
// NumPy's gets there; a workgroup that does reports it and ends)
inline int randn_chunk_cap(long long n) {
  const long long pairs = (n + 1) / 2;
  return (int)(4 * (pairs * 1000 / 785 / kTrials + 2));
}

__device__ __forceinline__ uint32_t temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__device__ __forceinline__ uint32_t twist_word(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// init_genrand(seed) by lane 0: 624 dependent steps
__device__ __forceinline__ void seed_state(State& s, uint32_t seed) {
  if (threadIdx.x == 0) {
    uint32_t k = seed;
    s.key[0] = k;
    for (int i = 1; i < kWords; ++i) {
      k = 1812433253u * (k ^ (k >> 30)) + (uint32_t)i;
      s.key[i] = k;
    }
  }
  __syncthreads();
}

// One twist, then the tempered words into w[blk & 1].  Three phases over
// i in [0, 227), [227, 454), [454, 624): a phase reads key[i], key[i + 1]
// (rewritten by its neighbour lane in the same phase) and its third operand
// (final since the phase before), passes a barrier and only then writes.
// Word 623 reads the new key[0] and key[396].
__device__ __forceinline__ void next_block(State& s, int blk) {
  const int t = threadIdx.x;
  uint32_t v = 0;
  if (t < 227) v = twist_word(s.key[t], s.key[t + 1], s.key[t + 397]);
  __syncthreads();
  if (t < 227) s.key[t] = v;
  __syncthreads();
  if (t < 227) v = twist_word(s.key[t + 227], s.key[t + 228], s.key[t]);
  __syncthreads();
  if (t < 227) s.key[t + 227] = v;
  __syncthreads();
  if (t < 170) v = twist_word(s.key[t + 454], s.key[t == 169 ? 0 : t + 455], s.key[t + 227]);
  __syncthreads();
  if (t < 170) s.key[t + 454] = v;
  __syncthreads();
  uint32_t* w = s.w[blk & 1];
  for (int i = t; i < kWords; i += kThreads) w[i] = temper(s.key[i]);
  __syncthreads();
}

// blocks 0 .. blk drawn (have: the number drawn so far, workgroup-uniform)
__device__ __forceinline__ void ensure_block(State& s, int& have, int blk) {
  while (have <= blk) {
    next_block(s, have);
    ++have;
  }
}

// output word g of the stream; its block is one of the two newest
__device__ __forceinline__ uint32_t word_at(const State& s, int g) {
  const int b = g / kWords;
  return s.w[b & 1][g - b * kWords];
}

// next_double on words g, g + 1
__device__ __forceinline__ double double_at(const State& s, int g) {
#pragma clang fp contract(off)
  const int32_t a = (int32_t)(word_at(s, g) >> 5), b = (int32_t)(word_at(s, g + 1) >> 6);
  return (a * 67108864.0 + b) / 9007199254740992.0;
}

// the polar trial on words g .. g + 3: its point and squared radius
__device__ __forceinline__ double polar_r2(const State& s, int g, double& x1, double& x2) {
#pragma clang fp contract(off)
  x1 = 2.0 * double_at(s, g) - 1.0;
  x2 = 2.0 * double_at(s, g + 2) - 1.0;
  return x1 * x1 + x2 * x2;
}

// `count` draws next32() & mask (mask + 1 a power of two: none rejected) from
// word `base` on, draw l (word base + l) handed to put(l, value).  The block
// of word `base` must be one of the two newest, or not drawn yet.
template <typename Put>
__device__ __forceinline__ void draw_masked_from(State& s, int& have, int base, int count, uint32_t mask, Put put) {
  const int last = base + count;
  for (int b = base / kWords; b * kWords < last; ++b) {
    ensure_block(s, have, b);
    const int beg = base > b * kWords ? base : b * kWords;
    const int end = last < (b + 1) * kWords ? last : (b + 1) * kWords;
    for (int g = beg + (int)threadIdx.x; g < end; g += kThreads) put(g - base, s.w[b & 1][g - b * kWords] & mask);
  }
}

// the same from word 0 on
template <typename Put>
__device__ __forceinline__ void draw_masked(State& s, int& have, int count, uint32_t mask, Put put) {
  draw_masked_from(s, have, 0, count, mask, put);
}

// randn(n) from word `base` on into out[0 .. n) (times sigma when scaled, a
// rounding of its own as in noise *= sigma).  false: the chunk cap was hit
// before n values were accepted (workgroup-uniform).
__device__ __forceinline__ bool draw_randn(State& s, int& have, int base, int n, bool scaled, double sigma,
                                           double* __restrict__ out, int max_chunks) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int pairs = (n + 1) / 2;
  int count = 0;  // accepted so far
  for (int c = 0; count < pairs; ++c) {
    if (c >= max_chunks) return false;
    const int g0 = base + c * kWords;
    ensure_block(s, have, (g0 + kWords - 1) / kWords);
    bool acc = false;
    double x1 = 0.0, x2 = 0.0, r2 = 0.0;
    if (t < kTrials) {
      r2 = polar_r2(s, g0 + 4 * t, x1, x2);
      acc = !(r2 >= 1.0 || r2 == 0.0);
    }
    const unsigned long long m = __ballot(acc);
    if (lane == 0) s.cnt[wv] = __popcll(m);
    __syncthreads();
    int a = count + __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < kThreads / 64; ++k) {
      const int ck = s.cnt[k];
      if (k < wv) a += ck;
      count += ck;
    }
    if (acc && a < pairs) {
      const double f = sqrt(-2.0 * log(r2) / r2);
      double v0 = f * x2, v1 = f * x1;
      if (scaled) {
        v0 = v0 * sigma;
        v1 = v1 * sigma;
      }
      out[2 * (size_t)a] = v0;
      if (2 * a + 1 < n) out[2 * (size_t)a + 1] = v1;  // n odd: the cached partner is dropped
    }
    // (s.cnt is next written behind the barriers of the next chunk's twist)
  }
  return true;
}

// random_sample(n) from word `base` on: exact
__device__ __forceinline__ void draw_samples(State& s, int& have, int base, int n, double* __restrict__ out) {
  for (int c = 0; c * kSamples < n; ++c) {
    const int g0 = base + c * kWords;
    ensure_block(s, have, (g0 + kWords - 1) / kWords);
    const int end = n < (c + 1) * kSamples ? n : (c + 1) * kSamples;
    for (int i = c * kSamples + (int)threadIdx.x; i < end; i += kThreads) out[i] = double_at(s, base + 2 * i);
  }
}

}  // namespace legacy_rng_dev

#endif  // LEGACY_MT_DEV_H
