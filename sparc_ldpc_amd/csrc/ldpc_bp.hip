// ldpc_bp.hip — MI355X (gfx950) LDPC belief-propagation decoder + C ABI.
//
// Replaces ldpc/src/c_ldpc.c (sumprod2 :138-206 with Lxfb :294-314 and Lxor
// :234-251; sumprod :32-113; minsum :339-381), bound by code.decode in
// ldpc/py/ldpc.py:855-930.
//
// Flooding schedule, one workgroup per codeword.  The message array (one
// binary64 per edge, in check-node order as the reference lays it out) lives
// in LDS when it fits (802.16 rate 5/6 z=192: 15360 edges = 120 KB of the
// 160 KB per CU), otherwise in a per-codeword HBM slice.  Per iteration:
//   variable phase: thread per variable node, sum channel + incoming edges
//     in port order (c_ldpc.c:171-178), write extrinsics and app;
//   check phase: thread per check node, forward/backward Lxor pass over its
//     contiguous edges (c_ldpc.c:294-314) with the forward values in
//     registers and the backward value carried, outputs written in place;
//   stop when every check's full XOR LLR b[0] is > 0 (c_ldpc.c:191-197).
// Every node performs the reference's operations in the reference's order,
// so results differ from the reference C build only through last-ulp
// differences between ROCm's and glibc's exp/log.  The path is bound by fp64
// transcendental throughput (3(dc-2)+... Lxor per check, 2 exp + 2 log each),
// not by memory: the only HBM traffic per iteration is ch and app.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "ldpc_bp_int.h"

#pragma clang fp contract(off)

#define LB_VERSION "ldpc_bp 0.1 gfx950"

namespace {

thread_local std::string g_err;

}  // namespace

namespace lb {

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

}  // namespace lb

using namespace lb;

namespace {

// ---------------------------------------------------------------------------
// Node rules
// ---------------------------------------------------------------------------
// Lxor (c_ldpc.c:234-251): sign product times min |.|, plus the two
// log(1+exp(-|.|)) corrections for the exact sum-product rule.  Symmetric in
// its arguments, bit for bit.
//
// The logarithm's argument is 1 + exp(-|x|), in [1, 2]: log12 evaluates it in
// the structure of fdlibm's e_log.c (u = 2^k m, m in [sqrt(2)/2, sqrt(2)],
// f = m - 1 exact, s = f / (2 + f), log(1 + f) = f - hfsq + s (hfsq + R(s^2)),
// |error| < 1 ulp) instead of ROCm's general log, whose double-double steps
// cost 46 of the 224 instructions of an Lxor: the check kernels are bound by
// this arithmetic.  Against glibc's log on the arguments Lxor produces (u = 1
// + exp(-x), x in [0, 40], 2e7 samples) 0.51 % of the results differ, by one
// ulp, never more (the reference's own build differs from ROCm's log by last
// ulps as well).  -DLB_OCML_LOG restores ROCm's log.
__host__ __device__ __forceinline__ double log12(double u) {
#ifdef LB_OCML_LOG
  return log(u);
#else
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  // branch-free: k = 0 gives 0 - ((hfsq - (s (hfsq + R) + 0)) - f), which is
  // e_log.c's f - (hfsq - s (hfsq + R)) bit for bit (f = m - 1 is never -0)
  const double k = u > 1.41421356237309504880 ? 1.0 : 0.0;
  const double m = u * (1.0 - 0.5 * k);
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * fma(w, fma(w, Lg6, Lg4), Lg2);
  const double t2 = z * fma(w, fma(w, fma(w, Lg7, Lg5), Lg3), Lg1);
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  return k * ln2_hi - ((hfsq - (s * (hfsq + R) + k * ln2_lo)) - f);
#endif
}

template <bool CORR>
__device__ __forceinline__ double lxor(double a, double b) {
  double L = (signbit(a) == signbit(b)) ? 1.0 : -1.0;
  L *= fmin(fabs(a), fabs(b));
  if (CORR) {
    L += log12(1.0 + exp(-fabs(a + b)));
    L -= log12(1.0 + exp(-fabs(a - b)));
  }
  return L;
}

// Binary32 twin (the layered decoders with LB_F32; tests/ldpc_f32_ref.py is its
// statement): the same sign rule and minimum, and the corrections c(|a + b|) -
// c(|a - b|), c(x) = log(1 + exp(-x)), every operation rounded to binary32.
// exp and log are the hardware's v_exp_f32 / v_log_f32 (base 2, the constants
// folded in): about ten instructions an Lxor against the binary64 rule's 140.
// 1 + exp(-x) lies in [1, 2], so v_log_f32 sees no subnormal, and a v_exp_f32
// result under 2^-126 (flushed) is lost in 1 + . anyway.  -DLB_F32_OCML takes
// the device library's expf / logf instead (DESIGN.md section 10 has both timed).
__device__ __forceinline__ float corr32(float x) {
#ifdef LB_F32_OCML
  return logf(1.0f + expf(-x));
#else
  return 0.693147180559945f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896f * x));
#endif
}

template <bool CORR>
__device__ __forceinline__ float lxor(float a, float b) {
  float L = (signbit(a) == signbit(b)) ? 1.0f : -1.0f;
  L *= fminf(fabsf(a), fabsf(b));
  if (CORR) {
    L += corr32(fabsf(a + b));
    L -= corr32(fabsf(a - b));
  }
  return L;
}

// Lxfb (c_ldpc.c:294-314) in place on one check node's dc messages:
// f[k] = Lxor(f[k-1], L[k]); b[k] = Lxor(b[k+1], L[k]);
// out[0] = b[1], out[dc-1] = f[dc-2], out[k] = Lxor(f[k-1], b[k+1]).
// f stays in registers (unrolled to DCMAX with guards); b is carried down.
// Returns b[0], the LLR of the XOR of all inputs (stopping rule).
template <int DCMAX, bool CORR, typename P>
__device__ __forceinline__ auto lxfb(P L, int dc) {
  using T = std::remove_cv_t<std::remove_reference_t<decltype(L[0])>>;  // double, or float (LB_F32)
  T f[DCMAX];
  f[0] = L[0];
#pragma unroll
  for (int k = 1; k < DCMAX; ++k)
    if (k < dc) f[k] = lxor<CORR>(f[k - 1], L[k]);
  T b = 0;
#pragma unroll
  for (int k = DCMAX - 1; k >= 1; --k) {
    if (k == dc - 1) {
      b = L[k];
      L[k] = f[k - 1];
    } else if (k < dc - 1) {
      const T lk = L[k];
      L[k] = lxor<CORR>(f[k - 1], b);
      b = lxor<CORR>(b, lk);
    }
  }
  const T l0 = L[0];
  L[0] = b;
  return lxor<CORR>(b, l0);
}

// Lxfb for checks of exactly DC edges (a check-regular code, e.g. 802.16
// rate 5/6: dc = 20 everywhere), in the reference's own loop structure
// (c_ldpc.c:294-314): the forward chain f[k] = Lxor(f[k-1], L[k]) and the
// backward chain b[k] = Lxor(b[k+1], L[k]) run side by side, then every
// output Lxor(f[k-1], b[k+1]) at once.  Straight-line code (no degree
// guards), so the two dependent chains interleave: the critical path is
// dc - 1 Lxor latencies plus one, against 2 (dc - 2) in lxfb's
// forward-then-backward form.  The same operations on the same operands:
// bit-identical to lxfb.
template <int DC, bool CORR, typename T>
__device__ __forceinline__ T lxfb_fixed_regs(const T (&l)[DC], T (&o)[DC]) {
  static_assert(DC >= 3, "fixed-degree checks");
  T f[DC - 1], b[DC];
  f[0] = l[0];
  b[DC - 1] = l[DC - 1];
#pragma unroll
  for (int k = 1; k < DC; ++k) {
    if (k < DC - 1) f[k] = lxor<CORR>(f[k - 1], l[k]);  // f[DC-1] is never used
    b[DC - 1 - k] = lxor<CORR>(b[DC - k], l[DC - 1 - k]);
  }
  o[0] = b[1];
  o[DC - 1] = f[DC - 2];
#pragma unroll
  for (int k = 1; k < DC - 1; ++k) o[k] = lxor<CORR>(f[k - 1], b[k + 1]);
  return b[0];  // = Lxor(b[1], L[0]), lxfb's return value
}

template <int DC, bool CORR, typename T>
__device__ __forceinline__ T lxfb_fixed(T* L) {
  T l[DC], o[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) l[k] = L[k];
  const T r = lxfb_fixed_regs<DC, CORR>(l, o);
#pragma unroll
  for (int k = 0; k < DC; ++k) L[k] = o[k];
  return r;
}

// One check node's rule on its dc messages at L (in place): the reference's
// three decoders.  Returns whether the check is unsatisfied (the stopping rule).
// On binary32 messages (sumprod2 and minsum only) corr is rounded to binary32 once.
template <int ALGO, int DCMAX, int DCFIX, typename P>
__device__ __forceinline__ bool check_rule(P L, int dc, double corr) {
  using T = std::remove_cv_t<std::remove_reference_t<decltype(L[0])>>;
  bool bad;
  if (ALGO == LB_SUMPROD) {  // c_ldpc.c:76-102
    double aggr = 1.0;
    for (int k = 0; k < dc; ++k) {
      const double t = tanh(L[k] / 2.0);
      L[k] = t;
      aggr *= t;
    }
    bad = 2.0 * atanh(aggr) <= 0.0;
    for (int k = 0; k < dc; ++k) L[k] = 2.0 * atanh(aggr / L[k]);
  } else if (ALGO == LB_SUMPROD2) {  // c_ldpc.c:183-194
    if constexpr (DCFIX > 0) bad = lxfb_fixed<DCFIX, true>(L) <= T(0);
    else bad = lxfb<DCMAX, true>(L, dc) <= T(0);
  } else {  // minsum, c_ldpc.c:364-372 with node-aligned offsets
    if constexpr (DCFIX > 0) bad = lxfb_fixed<DCFIX, false>(L) <= T(0);
    else bad = lxfb<DCMAX, false>(L, dc) <= T(0);
    const T cf = (T)corr;
    for (int k = 0; k < dc; ++k) L[k] *= cf;
  }
  return bad;
}

struct BpArgs {
  const double* ch;    // [B][Nv]
  double* app;         // [B][Nv]
  int* iters;          // [B]
  double* gmsg;        // [B][Nmsg] when the messages do not fit in LDS
  const int* vedge;    // [maxdv][Nv] message index of port k of variable node j
  const uint8_t* vdeg; // [Nv]
  const int* cstart;   // [Nc+1] first message of each check node
  int Nv, Nc, Nmsg, maxit;
  double corr;
  // hand-off to the tail kernels (tail != 0): a word not converged after
  // maxit iterations leaves its messages in gmsg and its index in active[]
  int tail;
  int* active;   // [B]
  int* nactive;  // [1]
  int* done;     // [B]
  int* lastbad;  // [2][B]: iteration stamp of the last unsatisfied check, by parity
  int B;
};

// DCFIX > 0: every check node has exactly DCFIX edges (lxfb_fixed; launched
// with at most kFixThreads threads, so a thread may hold the two chains in
// registers: 3 waves per SIMD)
template <int ALGO, int DCMAX, bool LDSM, int DCFIX = 0>
__global__ void __launch_bounds__(DCFIX > 0 ? kFixThreads : kMaxThreads) k_bp(BpArgs a) {
  extern __shared__ double lds_msg[];
  __shared__ int unsat[2];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* msg = LDSM ? lds_msg : a.gmsg + (size_t)b * a.Nmsg;
  const double* ch = a.ch + (size_t)b * a.Nv;
  double* app = a.app + (size_t)b * a.Nv;
  const int Nv = a.Nv, Nc = a.Nc;

  for (int i = tid; i < a.Nmsg; i += nt) msg[i] = 0.0;  // calloc (c_ldpc.c:164)
  if (tid < 2) unsat[tid] = 0;
  __syncthreads();

  int it = 0;
  for (; it < a.maxit; ++it) {
    // variable nodes (c_ldpc.c:171-178)
    for (int j = tid; j < Nv; j += nt) {
      const int d = a.vdeg[j];
      double aggr = ch[j];
      for (int k = 0; k < d; ++k) aggr += msg[a.vedge[(size_t)k * Nv + j]];
      for (int k = 0; k < d; ++k) {
        const int e = a.vedge[(size_t)k * Nv + j];
        msg[e] = aggr - msg[e];
      }
      app[j] = aggr;
    }
    // unsat[it & 1] was last read in iteration it-2; the barriers of it-1 order that read first
    if (tid == 0) unsat[it & 1] = 0;
    __syncthreads();
    // check nodes
    for (int c = tid; c < Nc; c += nt) {
      const int s = a.cstart[c], dc = a.cstart[c + 1] - s;
      const bool bad = check_rule<ALGO, DCMAX, DCFIX>(msg + s, dc, a.corr);
      if (bad) unsat[it & 1] = 1;
    }
    __syncthreads();
    if (!unsat[it & 1]) break;  // c_ldpc.c:196-197
  }
  if (a.tail && it == a.maxit) {
    // not converged in the first maxit iterations: the messages go to the
    // word's slice of gmsg (already there without LDS) for k_bp_tail
    if (LDSM) {
      double* g = a.gmsg + (size_t)b * a.Nmsg;
      for (int i = tid; i < a.Nmsg; i += nt) g[i] = msg[i];
    }
    if (tid == 0) {
      a.active[atomicAdd(a.nactive, 1)] = b;
      a.done[b] = 0;
      a.lastbad[((it - 1) & 1) * a.B + b] = it - 1;  // iteration it-1 left a check unsatisfied
      a.lastbad[(it & 1) * a.B + b] = -1;            // no stale stamp from an earlier decode
    }
  } else if (tid == 0) {
    a.iters[b] = it;
  }
}

// ---------------------------------------------------------------------------
// Layered schedule (row-layered / turbo-decoding message passing)
// ---------------------------------------------------------------------------
// One workgroup per word, app on chip for the whole decode.  A sweep walks the
// layers (for a quasi-cyclic code its protograph rows: z consecutive checks
// that share no variable) in order; per layer, over the layer's contiguous
// edges e (v = evar[e]):
//   gather:  app[v] -= r[e]; r[e] = app[v]     (q, rounded once)    all threads
//   check:   check_rule in place on each check's slice of r         thread per check
//   scatter: app[v] += r[e]                                         all threads
// so a later layer sees what the earlier ones have just written.  No variable
// occurs twice in a layer (lb_set_layers checks it): every app[v] has one
// owner per phase, and the result does not depend on the order the checks of
// a layer are taken in.  Before each sweep the stop test: every check has an
// even number of variables with app < 0 and none with app == 0 or NaN.
// iters = the sweeps run before the test passed, or maxit.
// MODE 2: r and app in LDS; 1: app in LDS, r in the word's HBM slice; 0: both
// in HBM (app in the output array itself).
//
// T = float (LB_F32): app, r, q and every Lxor in binary32, the statement being
// tests/ldpc_f32_ref.py.  ch is converted on load, clamped to +-2^100 (NaN and
// the sign of zero kept): with variable degrees up to 255 |app| stays under
// 2^108, so no inf - inf arises from saturated inputs; app is converted back on
// store.  The word's HBM slice of gmsg (Nmsg doubles) holds r as Nmsg floats
// and, in MODE 0, app as Nv <= Nmsg floats behind it.
struct BplArgs {
  const double* ch;   // [B][Nv]
  double* app;        // [B][Nv]
  int* iters;         // [B]
  double* gmsg;       // [B][Nmsg] (MODE < 2)
  const int* evar;    // [Nmsg] variable node of each edge
  const int* cstart;  // [Nc+1] first message of each check node
  const int* lfirst;  // [nlayers+1] first check of each layer
  int Nv, Nc, Nmsg, nlayers, maxit;
  double corr;
};

__device__ __forceinline__ void ch_load(double& dst, double x) { dst = x; }
__device__ __forceinline__ void ch_load(float& dst, double x) {
  const double lim = 0x1p100;
  dst = (float)(x > lim ? lim : (x < -lim ? -lim : x));  // NaN passes both tests
}

// `word` indexes ch; `slot` indexes what the decode owns while it runs: the app
// output, the HBM message slice and iters.  One workgroup per word (k_bpl,
// k_bpl32): both are blockIdx.x.  The persistent kernels (k_bpls, k_bpls32)
// decode many words in one slot.  Returns the sweep count, the same in every
// thread.
template <typename T, int ALGO, int DCMAX, int DCFIX, int MODE>
__device__ __forceinline__ int bpl_word(const BplArgs& a, T* lds, int* unsat, int word, int slot) {
  constexpr bool F32 = sizeof(T) == 4;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int Nv = a.Nv, Nc = a.Nc;
  const double* ch = a.ch + (size_t)word * Nv;
  double* out = a.app + (size_t)slot * Nv;
  T* slice = reinterpret_cast<T*>(a.gmsg + (size_t)slot * a.Nmsg);
  T* app;
  if constexpr (F32) app = MODE >= 1 ? lds : slice + a.Nmsg;
  else app = MODE >= 1 ? lds : out;
  T* r = MODE == 2 ? lds + Nv : slice;

  for (int i = tid; i < Nv; i += nt) ch_load(app[i], ch[i]);
  for (int i = tid; i < a.Nmsg; i += nt) r[i] = 0;
  if (tid < 2) unsat[tid] = 0;
  __syncthreads();

  int it = 0;
  for (; it < a.maxit; ++it) {
    // stop test on the hard decisions
    for (int c = tid; c < Nc; c += nt) {
      const int s = a.cstart[c], e1 = a.cstart[c + 1];
      bool odd = false, undecided = false;
      for (int e = s; e < e1; ++e) {
        const T x = app[a.evar[e]];
        odd ^= x < T(0);
        undecided |= !(x > T(0) || x < T(0));  // +-0 or NaN
      }
      if (odd || undecided) unsat[it & 1] = 1;
    }
    __syncthreads();
    if (!unsat[it & 1]) break;
    // the other flag was last read in sweep it-1, before the barrier above
    if (tid == 0) unsat[(it + 1) & 1] = 0;
    for (int l = 0; l < a.nlayers; ++l) {
      const int c0 = a.lfirst[l], c1 = a.lfirst[l + 1];
      const int e0 = a.cstart[c0], e1 = a.cstart[c1];
      for (int e = e0 + tid; e < e1; e += nt) {
        const int v = a.evar[e];
        const T q = app[v] - r[e];
        app[v] = q;
        r[e] = q;
      }
      __syncthreads();
      for (int c = c0 + tid; c < c1; c += nt) {
        const int s = a.cstart[c], dc = a.cstart[c + 1] - s;
        (void)check_rule<ALGO, DCMAX, DCFIX>(r + s, dc, a.corr);
      }
      __syncthreads();
      for (int e = e0 + tid; e < e1; e += nt) {
        const int v = a.evar[e];
        app[v] = app[v] + r[e];
      }
      __syncthreads();
    }
  }
  if (F32 || MODE >= 1)
    for (int i = tid; i < Nv; i += nt) out[i] = app[i];
  if (tid == 0) a.iters[slot] = it;
  return it;
}

template <int ALGO, int DCMAX, int DCFIX, int MODE>
__global__ void __launch_bounds__(DCFIX > 0 ? kFixThreads : kMaxThreads) k_bpl(BplArgs a) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  (void)bpl_word<double, ALGO, DCMAX, DCFIX, MODE>(a, lds_l, unsat, blockIdx.x, blockIdx.x);
}

// The binary32 instances.  The straight-line dc = 20 instance's second bound
// asks for registers that allow two workgroups' waves on a CU (2 x 768 threads:
// 6 waves per SIMD, at most 80 VGPRs): the 802.16 5/6 z=192 image is 78 KB, so
// two words share a CU.  The general instances keep what 1024 threads imply
// (4 waves per SIMD): DCMAX = 32 holds 32 forward values in registers.
template <int ALGO, int DCMAX, int DCFIX, int MODE>
__global__ void __launch_bounds__(DCFIX > 0 ? kFixThreads : kMaxThreads, DCFIX > 0 ? 6 : 4) k_bpl32(BplArgs a) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  (void)bpl_word<float, ALGO, DCMAX, DCFIX, MODE>(a, reinterpret_cast<float*>(lds_l), unsat, blockIdx.x, blockIdx.x);
}

// ---------------------------------------------------------------------------
// Persistent layered decode-and-count (lb_mc_stream_seeds, ldpc_mc.hip)
// ---------------------------------------------------------------------------
// The grid is `slots` workgroups over one chunk of Monte-Carlo blocks.  Each
// takes the chunk's next block by a ticket, decodes it with bpl_word in its
// own slot (image in LDS, app / message slices in HBM indexed by blockIdx.x),
// counts sum((app < 0) != x) and writes the block's two ints, until the chunk
// is out of tickets.  No workgroup waits for another.
//
// Stop rule (min_errors > 0): a block is skipped (iters = -1, errs = 0) when
// base + *eprev + *ecur >= min_errors: block errors of the chunks the host has
// consumed, of the chunk before, and of this chunk's finished blocks.  The
// counters are all one workgroup reads from another.  *ecur is read before the
// ticket is taken (an acquire load, so that the ticket's atomic cannot be
// issued ahead of it: a load and an L1 invalidate, no write-back): an error
// seen there belongs to a block whose ticket was taken earlier, that is to a
// smaller seed index, so the block asking lies behind the stopping block of
// the sequential rule.  The sum only grows, so an old value only skips later.
struct BplStreamArgs {
  BplArgs w;          // ch: the chunk's words; app, gmsg, iters: one slice per slot
  const uint8_t* x;   // [chunk][Nv] codeword bits
  int* errs;          // [chunk] bit errors
  int* iters;         // [chunk] sweeps, -1: skipped
  int* ticket;        // the chunk's next block
  const int* eprev;   // block errors of the chunk before
  int* ecur;          // block errors among this chunk's finished blocks
  int chunk, base, min_errors;
};

// decode(t, slot): the sweep count of word t of the chunk, decoded in the
// workgroup's slot with app left in the slot's slice of s.w.app
template <typename Decode>
__device__ __forceinline__ void stream_blocks(const BplStreamArgs& s, Decode decode) {
  __shared__ int next[3];  // ticket, skip, the word's bit errors
  const int tid = threadIdx.x, nt = blockDim.x, slot = blockIdx.x, Nv = s.w.Nv;
  for (;;) {
    // the word before is done with next[], unsat[], its image and its slices:
    // the next word's app = ch, r = 0 and unsat = 0 start behind this barrier
    __syncthreads();
    if (tid == 0) {
      int skip = 0;
      if (s.min_errors > 0) {
        const int e0 = __hip_atomic_load(s.eprev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int e1 = __hip_atomic_load(s.ecur, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        skip = s.base + e0 + e1 >= s.min_errors;
      }
      next[0] = __hip_atomic_fetch_add(s.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      next[1] = skip;
      next[2] = 0;
    }
    __syncthreads();
    const int t = next[0];
    if (t >= s.chunk) return;
    if (next[1]) {
      if (tid == 0) {
        s.iters[t] = -1;
        s.errs[t] = 0;
      }
      continue;
    }
    int it = 0;
    const double* v = s.w.ch + (size_t)t * Nv;  // max_iter = 0: app = ch, unrounded, as the batch path has it
    if (s.w.maxit > 0) {
      it = decode(t, slot);
      // every out[i] was written by this thread or in front of a barrier of the decode
      v = s.w.app + (size_t)slot * Nv;
    }
    const uint8_t* xb = s.x + (size_t)t * Nv;
    int cnt = 0;
    for (int i = tid; i < Nv; i += nt) cnt += ((v[i] < 0.0) != (xb[i] != 0)) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&next[2], cnt);
    __syncthreads();
    if (tid == 0) {
      const int sum = next[2];
      s.errs[t] = sum;
      s.iters[t] = it;
      if (sum) (void)__hip_atomic_fetch_add(s.ecur, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, int ALGO, int DCMAX, int DCFIX, int MODE>
__device__ __forceinline__ void bpl_stream(const BplStreamArgs& s, T* lds, int* unsat) {
  stream_blocks(s, [&](int t, int slot) { return bpl_word<T, ALGO, DCMAX, DCFIX, MODE>(s.w, lds, unsat, t, slot); });
}

template <int ALGO, int DCMAX, int DCFIX, int MODE>
__global__ void __launch_bounds__(DCFIX > 0 ? kFixThreads : kMaxThreads) k_bpls(BplStreamArgs s) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  bpl_stream<double, ALGO, DCMAX, DCFIX, MODE>(s, lds_l, unsat);
}

// (the bounds of k_bpl32: two workgroups of the dc = 20 instance share a CU)
template <int ALGO, int DCMAX, int DCFIX, int MODE>
__global__ void __launch_bounds__(DCFIX > 0 ? kFixThreads : kMaxThreads, DCFIX > 0 ? 6 : 4) k_bpls32(BplStreamArgs s) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  bpl_stream<float, ALGO, DCMAX, DCFIX, MODE>(s, reinterpret_cast<float*>(lds_l), unsat);
}

// ---------------------------------------------------------------------------
// Fixed-point layered min-sum (LB_FIXED; tests/ldpc_fixed_ref.py is its statement)
// ---------------------------------------------------------------------------
// The layered schedule on saturating integers: app int16[Nv] and r int8[Nmsg]
// in LDS for the whole decode (2 Nv + Nmsg bytes: 802.16 5/6 z=192 is 24 576
// against binary32's 79 872), one workgroup per word.  The min-sum rule needs
// two minima and a parity per check, not a chain of values, so a layer is not
// bpl_word's gather / check-thread / scatter: a group of G lanes (a power of
// two, within a wave) owns a check.  Lane j of the group reads its edges j,
// j + G, .. once (app[v] and r[e]), keeps q and v in registers, the group folds
// (min1, min2, parity) of |q| with __shfl_xor, packed in one word (15 + 15 + 1
// bits), and every lane writes its own r[e] and app[v]:
//   mag_e = |q_e| == min1 ? min2 : min1      (a tie of the two smallest gives min2 == min1)
//   r[e]  = +-min((alpha mag_e + 8) >> 4, rmax);  app[v] = clip(q_e + r[e], +-amax)
// No variable occurs twice in a layer, so every app[v] and r[e] has one reader
// and one writer, the same lane, within a layer: one barrier per layer, none
// inside.  EPL = the edges a lane may hold (G EPL >= the largest check degree).
// The loops over checks run the same number of passes in every thread, so the
// shuffles are never issued under divergence; a group without a check folds
// neutral values.  A check of degree 1 sees mag = amax (the minimum over no edge).
template <int G, int EPL>
__device__ __forceinline__ int bplq_word(const BplArgs& a, const FixedPar& p, unsigned char* lds, int* unsat, int word,
                                         int slot) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int Nv = a.Nv, Nc = a.Nc;
  const int j = tid & (G - 1), grp = tid / G, cpp = nt / G;  // lane of the group, group, checks per pass
  const int rmax = p.rmax, amax = p.amax, alpha = p.alpha;
  const double* ch = a.ch + (size_t)word * Nv;
  double* out = a.app + (size_t)slot * Nv;
  int16_t* app = reinterpret_cast<int16_t*>(lds);
  int8_t* r = reinterpret_cast<int8_t*>(lds + 2 * (size_t)Nv);

  const double up = (double)(1 << p.frac), down = 1.0 / up;
  for (int i = tid; i < Nv; i += nt) {
    double x = rint(ch[i] * up);  // half to even; +-inf stay
    x = x > (double)rmax ? (double)rmax : (x < (double)-rmax ? (double)-rmax : x);
    app[i] = (int16_t)(x == x ? (int)x : 0);  // NaN -> 0; -0.0 -> 0
  }
  for (int i = tid; i < a.Nmsg; i += nt) r[i] = 0;
  if (tid < 2) unsat[tid] = 0;
  __syncthreads();

  int it = 0;
  for (; it < a.maxit; ++it) {
    // stop test on the hard decisions: bit 0 the check's parity, bit 1 an undecided variable
    for (int cb = 0; cb < Nc; cb += cpp) {
      const int c = cb + grp;
      int w = 0;
      if (c < Nc) {
        const int e1 = a.cstart[c + 1];
        for (int e = a.cstart[c] + j; e < e1; e += G) {
          const int x = app[a.evar[e]];
          w ^= x < 0 ? 1 : 0;
          w |= x == 0 ? 2 : 0;
        }
      }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        const int y = __shfl_xor(w, o, 64);
        w = ((w ^ y) & 1) | ((w | y) & 2);
      }
      if (w && j == 0) unsat[it & 1] = 1;
    }
    __syncthreads();
    if (!unsat[it & 1]) break;
    // the other flag was last read in sweep it-1, before the barrier above
    if (tid == 0) unsat[(it + 1) & 1] = 0;
    for (int l = 0; l < a.nlayers; ++l) {
      const int c0 = a.lfirst[l], c1 = a.lfirst[l + 1];
      for (int cb = c0; cb < c1; cb += cpp) {
        const int c = cb + grp;
        int s = 0, dc = 0;
        if (c < c1) {
          s = a.cstart[c];
          dc = a.cstart[c + 1] - s;
        }
        int q[EPL], v[EPL];
        int m1 = amax, m2 = amax, par = 0;
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const int i = j + k * G;
          if (i < dc) {
            v[k] = a.evar[s + i];
            int x = (int)app[v[k]] - (int)r[s + i];
            x = x > amax ? amax : (x < -amax ? -amax : x);
            q[k] = x;
            const int m = x < 0 ? -x : x;
            par ^= x < 0 ? 1 : 0;
            m2 = min(m2, max(m1, m));
            m1 = min(m1, m);
          }
        }
        int w = m1 | (m2 << 15) | (par << 30);
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
          const int y = __shfl_xor(w, o, 64);
          const int a1 = w & 0x7fff, a2 = (w >> 15) & 0x7fff, b1 = y & 0x7fff, b2 = (y >> 15) & 0x7fff;
          w = min(a1, b1) | (min(max(a1, b1), min(a2, b2)) << 15) | ((w ^ y) & (1 << 30));
        }
        m1 = w & 0x7fff;
        m2 = (w >> 15) & 0x7fff;
        par = (w >> 30) & 1;
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const int i = j + k * G;
          if (i < dc) {
            const int x = q[k];
            const int m = x < 0 ? -x : x;
            const int mag = min((alpha * (m == m1 ? m2 : m1) + 8) >> 4, rmax);
            const int rn = (par ^ (x < 0 ? 1 : 0)) ? -mag : mag;
            r[s + i] = (int8_t)rn;
            const int y = x + rn;
            app[v[k]] = (int16_t)(y > amax ? amax : (y < -amax ? -amax : y));
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < Nv; i += nt) out[i] = (double)app[i] * down;
  if (tid == 0) a.iters[slot] = it;
  return it;
}

struct BplqArgs {
  BplArgs w;  // (gmsg and corr unused)
  FixedPar p;
};

struct BplqStreamArgs {
  BplStreamArgs s;
  FixedPar p;
};

// The second bound follows from the measured residency: the 802.16 5/6 z=192 plan (G = 4, five edges a
// lane, 1024 threads, a 24 KB image) has two workgroups on a CU only at eight waves a SIMD, which the
// persistent instance missed by its scalar registers (103: seven waves).  Instances of up to five
// edges a lane are asked for eight (at most 64 VGPRs, which they use anyway: 35..61); the wider ones
// (up to 105 VGPRs at 32 edges a lane) keep what 1024 threads imply.
constexpr int fixed_waves(int epl) { return epl <= 5 ? 8 : 4; }

template <int G, int EPL>
__global__ void __launch_bounds__(kMaxThreads, fixed_waves(EPL)) k_bplq(BplqArgs a) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  (void)bplq_word<G, EPL>(a.w, a.p, reinterpret_cast<unsigned char*>(lds_l), unsat, blockIdx.x, blockIdx.x);
}

// the persistent ticketed form (lb_mc_stream_seeds)
template <int G, int EPL>
__global__ void __launch_bounds__(kMaxThreads, fixed_waves(EPL)) k_bplsq(BplqStreamArgs a) {
  extern __shared__ double lds_l[];
  __shared__ int unsat[2];
  unsigned char* lds = reinterpret_cast<unsigned char*>(lds_l);
  stream_blocks(a.s, [&](int t, int slot) { return bplq_word<G, EPL>(a.s.w, a.p, lds, unsat, t, slot); });
}

// ---------------------------------------------------------------------------
// Tail: the iterations after the first `tail_at`, for the words still running
// ---------------------------------------------------------------------------
// One workgroup holds one word's whole decode above, so the words that do not
// converge (at the joint simulator's operating point a fifth of them run to
// max_iter) leave most of the chip idle while the launch waits for them: each
// iteration is a fixed ~75 us of one CU's binary64 VALU.  From iteration
// tail_at on, the words still running are spread over the chip, two launches
// per iteration, messages in HBM in two slots (read r_{t-1}, write r_t):
//   k_bp_tail_var: thread per variable node, ch + incoming messages in port
//     order (c_ldpc.c:171-178) -> app[v] (the aggregate itself);
//   k_bp_tail_chk: S workgroups per word, thread per check node, input
//     app[v(e)] - r_{t-1}[e] (the reference's extrinsic, the same subtraction)
//     and the check rule of k_bp.
// Bit-identical to running the whole decode in k_bp.
//
// Two ways to size the tail.  Sized on the host (lb_decode, which blocks
// anyway): one 4-byte read-back gives the number n of words still running
// after tail_at iterations, the grids cover exactly those words, and the host
// stops issuing iterations once a read-back shows every word done.  Sized on
// the device (lb_run / lb_decode_device, which must not block the caller):
// every iteration up to max_iter is queued behind the first phase with grids
// sized from an estimate of n; each kernel reads n and the done count from
// device memory, strides over the words the estimate did not cover, and
// returns at once when every word is done.  Same kernels, same arithmetic in
// the same order: the two are bit-identical.
struct TailArgs {
  const double* ch;      // [B][Nv]
  double* app;           // [B][Nv]
  int* iters;            // [B]
  const double* rold;    // [B][Nmsg] check-to-variable messages of iteration it-1
  double* rnew;          // [B][Nmsg] ... of iteration it
  const int* vedge;      // [maxdv][Nv]
  const uint8_t* vdeg;   // [Nv]
  const int* evar;       // [Nmsg] variable node of each edge
  const int* cstart;     // [Nc+1]
  const int* active;     // [n] words still running
  int* done;             // [B]
  int* ndone;            // [1] words detected as done in the tail (the stop test)
  const int* nactive;    // [1] words entering the tail (device-sized mode)
  int* lastbad;          // [2][B]
  int Nv, Nc, Nmsg, B, n, S, it;
  int dyn;               // 1: n and the stop test from device memory
  double corr;
};

// words still running in this tail launch; 0 when every word is done
__device__ __forceinline__ int tail_words(const TailArgs& a) {
  if (!a.dyn) return a.n;
  const int n = *a.nactive;
  return *a.ndone >= n ? 0 : n;
}

// DV >= the largest variable degree (4, 8 or 12): every port's table entry
// and message loaded at once, summed in port order with exact selects
template <int DV>
__global__ void __launch_bounds__(256) k_bp_tail_var(TailArgs a) {
  const int n = tail_words(a);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  for (int wi = blockIdx.y; wi < n; wi += gridDim.y) {
    const int w = a.active[wi];
    if (a.done[w]) continue;  // converged in an earlier iteration
    if (a.lastbad[((a.it - 1) & 1) * a.B + w] != a.it - 1) {
      // iteration it-1 satisfied every check (c_ldpc.c:196-197): it is the word's last
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.iters[w] = a.it - 1;
        a.done[w] = 1;
        atomicAdd(a.ndone, 1);
      }
      continue;
    }
    if (j >= a.Nv) continue;
    const double* rold = a.rold + (size_t)w * a.Nmsg;
    const int d = a.vdeg[j];
    int e[DV];
#pragma unroll
    for (int k = 0; k < DV; ++k) e[k] = a.vedge[(size_t)(k < d ? k : 0) * a.Nv + j];
    double x[DV];
#pragma unroll
    for (int k = 0; k < DV; ++k) x[k] = rold[e[k]];
    double aggr = a.ch[(size_t)w * a.Nv + j];
#pragma unroll
    for (int k = 0; k < DV; ++k)
      if (k < d) aggr += x[k];
    a.app[(size_t)w * a.Nv + j] = aggr;
  }
}

// the value of the other lane of an even/odd lane pair (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ double swap_pair(double x) {
  const unsigned long long u = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)u, 0xB1, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), 0xB1, 0xF, 0xF, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

template <int ALGO, int DCMAX, int DCFIX>
__global__ void __launch_bounds__(DCFIX > 0 ? kTailFixThreads : kTailThreads) k_bp_tail_chk(TailArgs a) {
  constexpr int ROW = DCMAX + 1;
  __shared__ double rows[DCFIX > 0 ? 1 : kTailThreads * ROW];
  const int n = tail_words(a);
  const int cpw = (a.Nc + a.S - 1) / a.S;
  for (int item = blockIdx.x; item < n * a.S; item += gridDim.x) {
    const int wi = item / a.S, slice = item % a.S;
    const int w = a.active[wi];
    if (a.done[w]) continue;
    const double* rold = a.rold + (size_t)w * a.Nmsg;
    double* rnew = a.rnew + (size_t)w * a.Nmsg;
    const double* app = a.app + (size_t)w * a.Nv;
    const int c0 = slice * cpw, c1 = min(a.Nc, c0 + cpw);
    bool anybad = false;
    if constexpr (DCFIX > 0) {
      // two lanes per check: lane p = 0 runs the forward chain f, lane p = 1
      // the backward chain b (its inputs in reverse order), in one instruction
      // stream; then each takes half of the outputs Lxor(f[k-1], b[k+1]) with
      // the partner's chain values swapped in (DPP).  The same Lxor calls on
      // the same operands in the same order as lxfb_fixed_regs: bit-identical.
      static_assert(DCFIX == 20, "the output split below is written for dc = 20");
      const int p = threadIdx.x & 1;
      for (int c = c0 + ((int)threadIdx.x >> 1); c < c1; c += blockDim.x >> 1) {
        const int s = c * DCFIX;  // check-regular: cstart[c] = c * DCFIX
        int ev[DCFIX];
        double r[DCFIX], l[DCFIX];
#pragma unroll
        for (int k = 0; k < DCFIX; ++k) {
          const int e = s + (p ? DCFIX - 1 - k : k);
          ev[k] = a.evar[e];
          r[k] = rold[e];
        }
#pragma unroll
        for (int k = 0; k < DCFIX; ++k) l[k] = app[ev[k]] - r[k];  // lane 1: l in reverse order
        constexpr bool CORR = ALGO == LB_SUMPROD2;
        double g[DCFIX];  // lane 0: g[i] = f[i]; lane 1: g[i] = b[DC-1-i]
        g[0] = l[0];
#pragma unroll
        for (int i = 1; i < DCFIX; ++i) g[i] = lxor<CORR>(g[i - 1], l[i]);
        double pg[9];  // the partner's g[9..17]
#pragma unroll
        for (int i = 0; i < 9; ++i) pg[i] = swap_pair(g[9 + i]);
        double o[10];
        o[0] = g[18];  // lane 0: o[19] = f[18]; lane 1: o[0] = b[1]
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          // lane 0: k = 1 + i, f[k-1] = g[i], b[k+1] = partner g[17-i]
          // lane 1: k = 10 + i, f[k-1] = partner g[9+i], b[k+1] = g[8-i]
          const double fa = p ? pg[i] : g[i];
          const double bb = p ? g[8 - i] : pg[8 - i];
          o[1 + i] = lxor<CORR>(fa, bb);
        }
        if (ALGO != LB_SUMPROD2) {
#pragma unroll
          for (int i = 0; i < 10; ++i) o[i] *= a.corr;
        }
        rnew[s + (p ? 0 : DCFIX - 1)] = o[0];
#pragma unroll
        for (int i = 0; i < 9; ++i) rnew[s + (p ? 10 : 1) + i] = o[1 + i];
        anybad |= p && g[DCFIX - 1] <= 0.0;  // b[0]: lxfb's return value
      }
    } else {
      for (int c = c0 + (int)threadIdx.x; c < c1; c += blockDim.x) {
        const int s = a.cstart[c], dc = a.cstart[c + 1] - s;
        double* L = rows + threadIdx.x * ROW;
        for (int k = 0; k < dc; ++k) L[k] = app[a.evar[s + k]] - rold[s + k];
        anybad |= check_rule<ALGO, DCMAX, 0>(L, dc, a.corr);
        for (int k = 0; k < dc; ++k) rnew[s + k] = L[k];
      }
    }
    if (anybad) a.lastbad[(a.it & 1) * a.B + w] = a.it;
  }
}

// after the last tail iteration: the iteration count of the words that ran to
// the end (max_iter, or max_iter - 1 when the last iteration converged)
__global__ void k_bp_tail_end(int* iters, const int* active, const int* nactive, const int* done,
                              const int* lastbad, int B, int maxit) {
  const int n = *nactive;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int w = active[i];
    if (!done[w]) iters[w] = lastbad[((maxit - 1) & 1) * B + w] == maxit - 1 ? maxit : maxit - 1;
  }
}

__global__ void k_lxor(double a, double b, int corr, double* out) {
  out[0] = corr ? lxor<true>(a, b) : lxor<false>(a, b);
}

__global__ void k_lxfb(double* L, int dc, int corr, double* out) {
  out[0] = corr ? lxfb<32, true>(L, dc) : lxfb<32, false>(L, dc);
}

using KernelFn = void (*)(BpArgs);

// The pick_* functions take the check-degree class as ldpc_plan.h computed it (GraphPlan::dcmax,
// LayeredLaunch): 8 / 16 / 32, and 20 beside them for the fixed-point kernels.
template <int ALGO, bool LDSM>
KernelFn pick_dc(int dcmax) {
  switch (dcmax) {
    case 8: return k_bp<ALGO, 8, LDSM>;
    case 16: return k_bp<ALGO, 16, LDSM>;
    default: return k_bp<ALGO, 32, LDSM>;
  }
}

KernelFn pick_kernel(int algo, int dcmax, bool lds, bool fixed = false) {
  if (fixed && algo == LB_SUMPROD2) return lds ? k_bp<LB_SUMPROD2, 32, true, 20> : k_bp<LB_SUMPROD2, 32, false, 20>;
  if (fixed && algo == LB_MINSUM) return lds ? k_bp<LB_MINSUM, 32, true, 20> : k_bp<LB_MINSUM, 32, false, 20>;
  // sumprod does not use the register-resident forward values: one instance suffices
  switch (algo) {
    case LB_SUMPROD2: return lds ? pick_dc<LB_SUMPROD2, true>(dcmax) : pick_dc<LB_SUMPROD2, false>(dcmax);
    case LB_SUMPROD: return lds ? k_bp<LB_SUMPROD, 8, true> : k_bp<LB_SUMPROD, 8, false>;
    default: return lds ? pick_dc<LB_MINSUM, true>(dcmax) : pick_dc<LB_MINSUM, false>(dcmax);
  }
}

// A layered instance: the kernel of one workgroup per word and the persistent kernel of the block
// stream, of one template row, so that a class cannot differ between the two.
struct LayeredInst {
  void (*batch)(BplArgs);
  void (*stream)(BplStreamArgs);
};

template <int ALGO, int DCMAX, int DCFIX, int MODE>
LayeredInst layered_row(bool f32) {
  if (f32) return {k_bpl32<ALGO, DCMAX, DCFIX, MODE>, k_bpls32<ALGO, DCMAX, DCFIX, MODE>};
  return {k_bpl<ALGO, DCMAX, DCFIX, MODE>, k_bpls<ALGO, DCMAX, DCFIX, MODE>};
}

template <int ALGO, int MODE>
LayeredInst pick_layered_dc(int dcmax, int dcfix, bool f32) {
  if (dcfix) return layered_row<ALGO, 32, 20, MODE>(f32);
  switch (dcmax) {
    case 8: return layered_row<ALGO, 8, 0, MODE>(f32);
    case 16: return layered_row<ALGO, 16, 0, MODE>(f32);
    default: return layered_row<ALGO, 32, 0, MODE>(f32);
  }
}

// algo: LB_LAYERED_SUMPROD2 or LB_LAYERED_MINSUM; the check rules are the flooding decoders'
LayeredInst pick_layered(int algo, int dcmax, int dcfix, int mode, bool f32) {
  if (algo == LB_LAYERED_SUMPROD2)
    return mode == 2   ? pick_layered_dc<LB_SUMPROD2, 2>(dcmax, dcfix, f32)
           : mode == 1 ? pick_layered_dc<LB_SUMPROD2, 1>(dcmax, dcfix, f32)
                       : pick_layered_dc<LB_SUMPROD2, 0>(dcmax, dcfix, f32);
  return mode == 2   ? pick_layered_dc<LB_MINSUM, 2>(dcmax, dcfix, f32)
         : mode == 1 ? pick_layered_dc<LB_MINSUM, 1>(dcmax, dcfix, f32)
                     : pick_layered_dc<LB_MINSUM, 0>(dcmax, dcfix, f32);
}

// The fixed-point instances: lanes per check G x the check-degree class (8 / 16 / 20 / 32 edges over
// the group's lanes, dc_class_fixed).
struct FixedInst {
  void (*batch)(BplqArgs);
  void (*stream)(BplqStreamArgs);
};

template <int G, int DCMAX>
FixedInst fixed_row() {
  return {k_bplq<G, edges_per_lane(DCMAX, G)>, k_bplsq<G, edges_per_lane(DCMAX, G)>};
}

template <int G>
FixedInst pick_fixed_g(int dcmax) {
  switch (dcmax) {
    case 8: return fixed_row<G, 8>();
    case 16: return fixed_row<G, 16>();
    case 20: return fixed_row<G, 20>();
    default: return fixed_row<G, 32>();
  }
}

FixedInst pick_fixed(int lanes, int dcmax) {
  switch (lanes) {
    case 1: return pick_fixed_g<1>(dcmax);
    case 2: return pick_fixed_g<2>(dcmax);
    case 4: return pick_fixed_g<4>(dcmax);
    case 8: return pick_fixed_g<8>(dcmax);
    default: return pick_fixed_g<16>(dcmax);
  }
}

using TailFn = void (*)(TailArgs);

template <int ALGO>
TailFn pick_tail_dc(int dcmax) {
  switch (dcmax) {
    case 8: return k_bp_tail_chk<ALGO, 8, 0>;
    case 16: return k_bp_tail_chk<ALGO, 16, 0>;
    default: return k_bp_tail_chk<ALGO, 32, 0>;
  }
}

TailFn pick_tail(int algo, int dcmax, bool fixed) {
  if (fixed && algo == LB_SUMPROD2) return k_bp_tail_chk<LB_SUMPROD2, 32, 20>;
  if (fixed && algo == LB_MINSUM) return k_bp_tail_chk<LB_MINSUM, 32, 20>;
  switch (algo) {
    case LB_SUMPROD2: return pick_tail_dc<LB_SUMPROD2>(dcmax);
    case LB_SUMPROD: return pick_tail_dc<LB_SUMPROD>(dcmax);
    default: return pick_tail_dc<LB_MINSUM>(dcmax);
  }
}

TailFn pick_tail_var(int nq) {
  return nq == 1 ? k_bp_tail_var<4> : (nq == 2 ? k_bp_tail_var<8> : k_bp_tail_var<12>);
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int default_device() {
  const char* e = getenv("LDPC_BP_DEVICE");
  if (!e || !*e) e = getenv("LOCAL_RANK");
  return (e && *e) ? atoi(e) : 0;
}

}  // namespace

namespace lb {

void release(lb_ctx* c) {
  if (!c) return;
  mc_release(c);
  (void)hipSetDevice(c->dev);
  (void)hipFree(c->d_vedge);
  (void)hipFree(c->d_vdeg);
  (void)hipFree(c->d_cstart);
  (void)hipFree(c->d_ch);
  (void)hipFree(c->d_app);
  (void)hipFree(c->d_msg);
  (void)hipFree(c->d_it);
  (void)hipFree(c->d_evar);
  (void)hipFree(c->d_lfirst);
  (void)hipFree(c->d_active);
  (void)hipFree(c->d_nact);
  (void)hipFree(c->d_done);
  (void)hipFree(c->d_lastbad);
  if (c->h_nact) (void)hipHostFree(c->h_nact);
  for (hipEvent_t e : c->evc)
    if (e) (void)hipEventDestroy(e);
  if (c->evn) (void)hipEventDestroy(c->evn);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int dev_alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    *p = nullptr;
    return fail(LB_ERR_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  return LB_OK;
}

int ensure_io(lb_ctx* c, int B) {
  if (B <= c->capB) return LB_OK;
  (void)hipFree(c->d_ch);
  (void)hipFree(c->d_app);
  (void)hipFree(c->d_it);
  c->d_ch = c->d_app = nullptr;
  c->d_it = nullptr;
  c->capB = 0;
  int rc;
  if ((rc = dev_alloc((void**)&c->d_ch, (size_t)B * c->Nv * sizeof(double)))) return rc;
  if ((rc = dev_alloc((void**)&c->d_app, (size_t)B * c->Nv * sizeof(double)))) return rc;
  if ((rc = dev_alloc((void**)&c->d_it, (size_t)B * sizeof(int)))) return rc;
  c->capB = B;
  return LB_OK;
}

// message slices: one per word without LDS, two per word (r_{t-1}, r_t)
// for the tail launches; capMsgB counts word slices
int ensure_slices(lb_ctx* c, int need) {
  if (need <= c->capMsgB) return LB_OK;
  (void)hipFree(c->d_msg);
  c->d_msg = nullptr;
  c->capMsgB = 0;
  int rc;
  if ((rc = dev_alloc((void**)&c->d_msg, (size_t)need * c->Nmsg * sizeof(double)))) return rc;
  c->capMsgB = need;
  return LB_OK;
}

int ensure_msg(lb_ctx* c, int B, bool tail) { return ensure_slices(c, tail ? 2 * B : (c->lds ? 0 : B)); }

// (lb::resolve, declared in ldpc_bp_int.h)
int resolve(lb_ctx* c, int algo, double corr, int max_iter, bool for_stream, DecType* t) {
  std::string err;
  const int rc = resolve(*c, *c, *c, algo, corr, max_iter, for_stream, t, err);
  return rc ? fail(rc, err) : LB_OK;
}

// Raise a kernel's dynamic LDS limit, once per context.  The layered instances ask for the whole
// budget, whatever this code needs: contexts of other codes share the instance.
int raise_lds(lb_ctx* c, const void* fn, size_t bytes = kLdsBytes - 64) {
  if (std::find(c->raised.begin(), c->raised.end(), fn) != c->raised.end()) return LB_OK;
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  c->raised.push_back(fn);
  return LB_OK;
}

// How a resolved layered type launches on this context: its batch / stream instance pair
// (floating or fixed point), threads per workgroup and dynamic LDS bytes (layered_launch).
struct LayeredShape {
  LayeredInst fn{};
  FixedInst qfn{};               // DecType::fixed
  const void* kernel = nullptr;  // the one of the pair asked for
  int nt = 0;
  size_t shm = 0;
};

// stream: the persistent kernel of the pair.  Raises that kernel's LDS limit on first use.
int layered_shape(lb_ctx* c, const DecType& t, bool stream, LayeredShape* s) {
  const LayeredLaunch ll = layered_launch(*c, *c, *c, t);
  s->nt = ll.nt;
  s->shm = ll.shm;
  if (t.fixed) {
    s->qfn = pick_fixed(ll.lanes, ll.dcmax);
    s->kernel = stream ? (const void*)s->qfn.stream : (const void*)s->qfn.batch;
  } else {
    s->fn = pick_layered(t.base, ll.dcmax, ll.dcfix, ll.mode, t.f32);
    s->kernel = stream ? (const void*)s->fn.stream : (const void*)s->fn.batch;
  }
  return s->shm ? raise_lds(c, s->kernel) : LB_OK;
}

// workgroups of that kernel a CU holds at once
int residency(lb_ctx* c, const DecType& t, bool stream, int* n, size_t* shm = nullptr) {
  LayeredShape s;
  int rc;
  if ((rc = layered_shape(c, t, stream, &s))) return rc;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(n, s.kernel, s.nt, s.shm));
  if (shm) *shm = s.shm;
  return LB_OK;
}

BplArgs bpl_args(const lb_ctx* c, const double* ch, double* app, int* iters, double* gmsg, double corr, int max_iter) {
  BplArgs a;
  a.ch = ch;
  a.app = app;
  a.iters = iters;
  a.gmsg = gmsg;
  a.evar = c->d_evar;
  a.cstart = c->d_cstart;
  a.lfirst = c->d_lfirst;
  a.Nv = c->Nv;
  a.Nc = c->Nc;
  a.Nmsg = c->Nmsg;
  a.nlayers = c->nlayers;
  a.maxit = max_iter;
  a.corr = corr;
  return a;
}

// the layered schedule: one launch, one workgroup per word, no tail (never waits)
int launch_layered(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, const DecType& t, double corr,
                   int max_iter) {
  int rc;
  std::string err;
  if ((rc = f32_slice_fits(*c, *c, t, err))) return fail(rc, err);
  if ((rc = ensure_slices(c, t.hbm ? B : 0))) return rc;
  LayeredShape s;
  if ((rc = layered_shape(c, t, false, &s))) return rc;
  if (t.fixed) {  // (gmsg and corr unused)
    const BplqArgs q{bpl_args(c, d_ch, d_app, d_it, nullptr, 0.0, max_iter), t.par};
    hipLaunchKernelGGL(s.qfn.batch, dim3(B), dim3(s.nt), s.shm, c->stream, q);
  } else {
    const BplArgs a = bpl_args(c, d_ch, d_app, d_it, c->d_msg, corr, max_iter);
    hipLaunchKernelGGL(s.fn.batch, dim3(B), dim3(s.nt), s.shm, c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return LB_OK;
}

// (lb::stream_plan, declared in ldpc_bp_int.h)
int stream_plan(lb_ctx* c, const DecType& t, int* resident) {
  HIP_TRY(hipSetDevice(c->dev));
  int rc, n = 0;
  if ((rc = residency(c, t, true, &n))) return rc;
  *resident = std::max(1, n);
  return LB_OK;
}

// (lb::launch_stream, declared in ldpc_bp_int.h)
int launch_stream(lb_ctx* c, hipStream_t st, int slots, const StreamChunk& k, const DecType& t, double corr,
                  int max_iter) {
  LayeredShape s;
  int rc;
  if ((rc = layered_shape(c, t, true, &s))) return rc;
  BplStreamArgs a;
  a.w = bpl_args(c, k.ch, k.app, k.slot_iters, k.msg, corr, max_iter);
  a.x = k.x;
  a.errs = k.errs;
  a.iters = k.iters;
  a.ticket = k.ticket;
  a.eprev = k.eprev;
  a.ecur = k.ecur;
  a.chunk = k.chunk;
  a.base = k.base;
  a.min_errors = k.min_errors;
  if (t.fixed) {
    const BplqStreamArgs q{a, t.par};
    hipLaunchKernelGGL(s.qfn.stream, dim3(slots), dim3(s.nt), s.shm, st, q);
  } else {
    hipLaunchKernelGGL(s.fn.stream, dim3(slots), dim3(s.nt), s.shm, st, a);
  }
  HIP_TRY(hipGetLastError());
  return LB_OK;
}

int ensure_tail(lb_ctx* c, int B) {
  if (B <= c->capTailB) return LB_OK;
  (void)hipFree(c->d_active);
  (void)hipFree(c->d_done);
  (void)hipFree(c->d_lastbad);
  c->d_active = c->d_done = c->d_lastbad = nullptr;
  c->capTailB = 0;
  int rc;
  if ((rc = dev_alloc((void**)&c->d_active, (size_t)B * sizeof(int)))) return rc;
  if ((rc = dev_alloc((void**)&c->d_done, (size_t)B * sizeof(int)))) return rc;
  if ((rc = dev_alloc((void**)&c->d_lastbad, (size_t)2 * B * sizeof(int)))) return rc;
  if (!c->d_nact && (rc = dev_alloc((void**)&c->d_nact, 2 * sizeof(int)))) return rc;
  for (hipEvent_t* e : {&c->evc[0], &c->evc[1], &c->evn})
    if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
      *e = nullptr;
      return fail(LB_ERR_HIP, "hipEventCreate failed");
    }
  if (!c->h_nact && hipHostMalloc((void**)&c->h_nact, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    c->h_nact = nullptr;
    return fail(LB_ERR_NOMEM, "hipHostMalloc failed");
  }
  c->capTailB = B;
  return LB_OK;
}

int set_attrs(lb_ctx* c) {
  if (!c->lds) return LB_OK;
  const size_t bytes = (size_t)c->Nmsg * sizeof(double);
  int rc;
  for (int algo = 0; algo < 3; ++algo)
    if ((rc = raise_lds(c, (const void*)pick_kernel(algo, c->dcmax, true, c->fixed), bytes))) return rc;
  return LB_OK;
}

int launch_tail(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, int algo, double corr, int max_iter,
                bool sized_on_host);

// the flooding schedule's first phase: all of max_iter in one launch, or the iterations before the tail
int launch_flooding(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, int algo, double corr,
                    int max_iter, bool sized_on_host) {
  // the tail's variable kernel puts the words on the grid's y dimension (<= 65535)
  const bool tail = c->tail_at > 0 && max_iter > c->tail_at && B <= 65535;
  int rc;
  if ((rc = ensure_msg(c, B, tail))) return rc;
  if ((rc = set_attrs(c))) return rc;
  if (tail && (rc = ensure_tail(c, B))) return rc;
  BpArgs a;
  a.ch = d_ch;
  a.app = d_app;
  a.iters = d_it;
  a.gmsg = c->d_msg;
  a.vedge = c->d_vedge;
  a.vdeg = c->d_vdeg;
  a.cstart = c->d_cstart;
  a.Nv = c->Nv;
  a.Nc = c->Nc;
  a.Nmsg = c->Nmsg;
  a.maxit = tail ? c->tail_at : max_iter;
  a.corr = corr;
  a.tail = tail ? 1 : 0;
  a.active = c->d_active;
  a.nactive = c->d_nact;
  a.done = c->d_done;
  a.lastbad = c->d_lastbad;
  a.B = B;
  // the previous device-sized tail's word count, if it has landed: the estimate
  // the next device-sized tail's grids are sized for
  if (c->est_pending && hipEventQuery(c->evn) == hipSuccess) {
    c->est_n = c->h_nact[3];
    c->est_B = c->est_Bq;
    c->est_pending = false;
  }
  if (tail) HIP_TRY(hipMemsetAsync(c->d_nact, 0, 2 * sizeof(int), c->stream));  // nactive, ndone
  const size_t shm = c->lds ? (size_t)c->Nmsg * sizeof(double) : 0;
  hipLaunchKernelGGL(pick_kernel(algo, c->dcmax, c->lds, c->fixed), dim3(B), dim3(c->nt), shm, c->stream, a);
  HIP_TRY(hipGetLastError());
  return tail ? launch_tail(c, B, d_ch, d_app, d_it, algo, corr, max_iter, sized_on_host) : LB_OK;
}

// The tail launches (k_bp_tail) from iteration tail_at on, over the words that phase one left
// running.  sized_on_host: the tail's shape from the number of those words (one read-back; the
// caller blocks anyway), else sized on the device and queued without waiting (see TailArgs)
int launch_tail(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, int algo, double corr, int max_iter,
                bool sized_on_host) {
  int n = B;
  if (sized_on_host) {
    // how many words are left decides the tail's shape (one 4-byte read-back)
    HIP_TRY(hipMemcpyAsync(c->h_nact, c->d_nact, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    n = *c->h_nact;
    if (n < 0 || n > B) return fail(LB_ERR_HIP, "tail word count out of range");
    if (n == 0) return LB_OK;
  }
  // the straight-line check rule runs on lane pairs
  const bool split = c->fixed && algo != LB_SUMPROD;
  const TailShape ts = tail_shape(B, n, sized_on_host, c->est_n, c->est_B, c->Nc, c->ncu, split);
  const int nsz = ts.nsz, m = ts.m, S = ts.S;
  TailArgs t;
  t.ch = d_ch;
  t.app = d_app;
  t.iters = d_it;
  t.vedge = c->d_vedge;
  t.vdeg = c->d_vdeg;
  t.evar = c->d_evar;
  t.cstart = c->d_cstart;
  t.active = c->d_active;
  t.done = c->d_done;
  t.ndone = c->d_nact + 1;
  t.nactive = c->d_nact;
  t.lastbad = c->d_lastbad;
  t.Nv = c->Nv;
  t.Nc = c->Nc;
  t.Nmsg = c->Nmsg;
  t.B = B;
  t.n = n;
  t.S = S;
  t.dyn = sized_on_host ? 0 : 1;
  t.corr = corr;
  double* slot[2] = {c->d_msg, c->d_msg + (size_t)B * c->Nmsg};
  const TailFn chk = pick_tail(algo, c->dcmax, split);
  const TailFn var = pick_tail_var(c->nq);
  const dim3 vgrid((c->Nv + 255) / 256, nsz);
  const dim3 cgrid((unsigned)nsz * S);
  auto iterate = [&](int it) {
    t.rold = slot[(it - c->tail_at) & 1];
    t.rnew = slot[(it - c->tail_at + 1) & 1];
    t.it = it;
    hipLaunchKernelGGL(var, vgrid, dim3(256), 0, c->stream, t);
    hipLaunchKernelGGL(chk, cgrid, dim3(64 * m), 0, c->stream, t);
  };
  if (!sized_on_host) {
    // every iteration queued; a launch past the last running word returns at once
    for (int it = c->tail_at; it < max_iter; ++it) iterate(it);
    // this tail's word count, for the next one's estimate (read when it has landed)
    HIP_TRY(hipMemcpyAsync(c->h_nact + 3, c->d_nact, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->evn, c->stream));
    c->est_pending = true;
    c->est_Bq = B;
  } else {
    // chunks of kTailChunk iterations; after each, the count of words found
    // done is copied back, and the host stops issuing chunks once the copy of
    // two chunks ago shows every word done (the GPU keeps the latest chunk
    // meanwhile: no stall while words run, no empty launches to max_iter after)
    for (int it0 = c->tail_at, k = 0; it0 < max_iter; it0 += kTailChunk, ++k) {
      if (k >= 2) {
        HIP_TRY(hipEventSynchronize(c->evc[k & 1]));
        if (c->h_nact[1 + (k & 1)] >= n) break;
      }
      for (int it = it0; it < std::min(max_iter, it0 + kTailChunk); ++it) iterate(it);
      HIP_TRY(hipMemcpyAsync(c->h_nact + 1 + (k & 1), c->d_nact + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipEventRecord(c->evc[k & 1], c->stream));
    }
  }
  hipLaunchKernelGGL(k_bp_tail_end, dim3((nsz + 255) / 256), dim3(256), 0, c->stream, d_it, c->d_active, c->d_nact,
                     c->d_done, c->d_lastbad, B, max_iter);
  HIP_TRY(hipGetLastError());
  return LB_OK;
}

// (lb::launch, declared in ldpc_bp_int.h)
int launch(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, const DecType& t, double corr,
           int max_iter, bool sized_on_host) {
  if (B == 0) return LB_OK;
  if (max_iter == 0) {
    // no iteration: the variable phase on zero messages, app = ch (the uncoded
    // hard decision), 0 iterations; k_bp would leave app unwritten
    HIP_TRY(hipMemcpyAsync(d_app, d_ch, (size_t)B * c->Nv * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_it, 0, (size_t)B * sizeof(int), c->stream));
    return LB_OK;
  }
  if (t.base >= LB_LAYERED_SUMPROD2) return launch_layered(c, B, d_ch, d_app, d_it, t, corr, max_iter);
  return launch_flooding(c, B, d_ch, d_app, d_it, t.base, corr, max_iter, sized_on_host);
}

}  // namespace lb

namespace {

// Graph cache for the reference-signature entry points (one decode per call,
// the graph identical across calls in the reference's harness).
struct CacheKey {
  int Nv, Nc, Nmsg, dev;
  uint64_t h;
  bool operator<(const CacheKey& o) const {
    return std::tie(Nv, Nc, Nmsg, dev, h) < std::tie(o.Nv, o.Nc, o.Nmsg, o.dev, o.h);
  }
};
std::mutex g_cache_mu;
std::map<CacheKey, lb_ctx*> g_cache;

uint64_t fnv(uint64_t h, const long* p, int n) {
  for (int i = 0; i < n; ++i) {
    h ^= (uint64_t)p[i];
    h *= 1099511628211ull;
  }
  return h;
}

int cached_ctx(long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg, lb_ctx** out) {
  if (!vdeg || !cdeg || !intrlv || Nv <= 0 || Nc <= 0 || Nmsg <= 0) return fail(LB_ERR_ARG, "null graph");
  const int dev = default_device();
  uint64_t h = 1469598103934665603ull;
  h = fnv(h, vdeg, Nv);
  h = fnv(h, cdeg, Nc);
  h = fnv(h, intrlv, Nmsg);
  const CacheKey k{Nv, Nc, Nmsg, dev, h};
  std::lock_guard<std::mutex> g(g_cache_mu);
  auto it = g_cache.find(k);
  if (it != g_cache.end()) {
    *out = it->second;
    return LB_OK;
  }
  if (g_cache.size() >= 16) {  // bounded: drop everything (a harness uses one or two codes)
    for (auto& kv : g_cache) release(kv.second);
    g_cache.clear();
  }
  lb_ctx* c = nullptr;
  const int rc = lb_create(&c, vdeg, cdeg, intrlv, Nv, Nc, Nmsg, dev);
  if (rc) return rc;
  g_cache[k] = c;
  *out = c;
  return LB_OK;
}

int ref_decode(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg, double* app,
               int algo, double corr) {
  if (!ch || !app) return fail(LB_ERR_ARG, "null ch/app");
  lb_ctx* c = nullptr;
  int rc = cached_ctx(vdeg, cdeg, intrlv, Nv, Nc, Nmsg, &c);
  if (rc) return rc;
  int it = 0;
  rc = lb_decode(c, 1, ch, app, &it, algo, corr, LB_MAX_ITCOUNT);
  return rc ? rc : it;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char* lb_last_error(void) { return g_err.c_str(); }
const char* lb_version(void) { return LB_VERSION; }
int lb_device_count(void) { return device_count(); }

int lb_create(lb_ctx** out, const long* vdeg, const long* cdeg, const long* intrlv, int Nv, int Nc,
              int Nmsg, int device) {
  if (!out) return fail(LB_ERR_ARG, "out is null");
  *out = nullptr;
  // a bad graph is refused on the host, before the device is looked at
  GraphPlan g;
  std::string err;
  int rc = check_graph(vdeg, cdeg, intrlv, Nv, Nc, Nmsg, g, err);
  if (rc) return fail(rc, err);
  const int ndev = device_count();
  if (ndev == 0) return fail(LB_ERR_NO_DEVICE, "no HIP device visible (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(LB_ERR_ARG, "device index out of range");
  const GraphTables t = graph_tables(vdeg, cdeg, intrlv, g);

  lb_ctx* c = new lb_ctx;
  static_cast<GraphPlan&>(*c) = plan_graph(g, read_switches());
  c->dev = device;
  c->h_evar = t.evar;
  c->h_cstart = t.cstart;
  auto bail = [&](int r) { release(c); return r; };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(LB_ERR_HIP, "hipSetDevice failed"));
  if ((rc = dev_alloc((void**)&c->d_vedge, t.vedge.size() * sizeof(int)))) return bail(rc);
  if ((rc = dev_alloc((void**)&c->d_vdeg, (size_t)Nv))) return bail(rc);
  if ((rc = dev_alloc((void**)&c->d_cstart, (size_t)(Nc + 1) * sizeof(int)))) return bail(rc);
  if ((rc = dev_alloc((void**)&c->d_evar, t.evar.size() * sizeof(int)))) return bail(rc);
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->ncu = ncu;
  }
  // (the stream at the device's highest priority, and the tail's waves at the
  // highest issue priority, measured slower / neutral beside a pipelined joint
  // batch's AMP stream, rounds 4-5: default priorities)
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess)
    return bail(fail(LB_ERR_HIP, "stream/event creation failed"));
  // uploads on the context's non-blocking stream, waited for (a pageable
  // hipMemcpy may return before its DMA lands, unordered with this stream)
  if (hipMemcpyAsync(c->d_vedge, t.vedge.data(), t.vedge.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_vdeg, t.vdeg.data(), (size_t)Nv, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_cstart, t.cstart.data(), (size_t)(Nc + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_evar, t.evar.data(), t.evar.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return bail(fail(LB_ERR_HIP, "graph upload failed"));
  *out = c;
  return LB_OK;
}

void lb_destroy(lb_ctx* ctx) { release(ctx); }

int lb_decode(lb_ctx* c, int B, const double* ch, double* app, int* iters, int algo, double corr_factor,
              int max_iter) {
  if (!c) return fail(LB_ERR_ARG, "null context");
  if (B < 0 || (B > 0 && (!ch || !app || !iters))) return fail(LB_ERR_ARG, "bad batch arguments");
  if (B == 0) return LB_OK;
  DecType t;
  int rc;
  if ((rc = resolve(c, algo, corr_factor, max_iter, false, &t))) return rc;
  HIP_TRY(hipSetDevice(c->dev));
  if ((rc = ensure_io(c, B))) return rc;
  const size_t bytes = (size_t)B * c->Nv * sizeof(double);
  HIP_TRY(hipMemcpyAsync(c->d_ch, ch, bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch(c, B, c->d_ch, c->d_app, c->d_it, t, corr_factor, max_iter, true))) return rc;
  HIP_TRY(hipMemcpyAsync(app, c->d_app, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(iters, c->d_it, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

int lb_decode_device(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_iters, int algo,
                     double corr_factor, int max_iter) {
  if (!c) return fail(LB_ERR_ARG, "null context");
  if (B < 0 || (B > 0 && (!d_ch || !d_app || !d_iters))) return fail(LB_ERR_ARG, "bad batch arguments");
  DecType t;
  int rc;
  if ((rc = resolve(c, algo, corr_factor, max_iter, false, &t))) return rc;
  HIP_TRY(hipSetDevice(c->dev));
  return launch(c, B, d_ch, d_app, d_iters, t, corr_factor, max_iter, false);
}

int lb_buffers(lb_ctx* c, int B, double** d_ch, double** d_app, int** d_iters) {
  if (!c || B <= 0) return fail(LB_ERR_ARG, "bad buffer request");
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = ensure_io(c, B))) return rc;
  if (d_ch) *d_ch = c->d_ch;
  if (d_app) *d_app = c->d_app;
  if (d_iters) *d_iters = c->d_it;
  return LB_OK;
}

int lb_stage(lb_ctx* c, int B, const double* ch) {
  if (!c || B <= 0 || !ch) return fail(LB_ERR_ARG, "bad stage arguments");
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = ensure_io(c, B))) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_ch, ch, (size_t)B * c->Nv * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

int lb_run(lb_ctx* c, int B, int algo, double corr_factor, int max_iter) {
  if (!c || B <= 0 || B > c->capB) return fail(LB_ERR_ARG, "run before stage, or B larger than staged");
  DecType t;
  int rc;
  if ((rc = resolve(c, algo, corr_factor, max_iter, false, &t))) return rc;
  HIP_TRY(hipSetDevice(c->dev));
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  if ((rc = launch(c, B, c->d_ch, c->d_app, c->d_it, t, corr_factor, max_iter, false))) return rc;
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  return LB_OK;
}

int lb_wait(lb_ctx* c) {
  if (!c) return fail(LB_ERR_ARG, "null context");
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

int lb_fetch(lb_ctx* c, int B, double* app, int* iters) {
  if (!c || B <= 0 || B > c->capB) return fail(LB_ERR_ARG, "bad fetch arguments");
  HIP_TRY(hipSetDevice(c->dev));
  if (app) HIP_TRY(hipMemcpyAsync(app, c->d_app, (size_t)B * c->Nv * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (iters) HIP_TRY(hipMemcpyAsync(iters, c->d_it, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

double lb_run_event_ms(lb_ctx* c) {
  if (!c) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0;
  return ms;
}

int lb_info(lb_ctx* c, long long* out) {
  if (!c || !out) return fail(LB_ERR_ARG, "null argument");
  out[0] = c->Nv;
  out[1] = c->Nc;
  out[2] = c->Nmsg;
  out[3] = c->maxdv;
  out[4] = c->maxdc;
  out[5] = c->lds ? 1 : 0;
  out[6] = c->nt;
  out[7] = c->dev;
  out[8] = c->fixed ? c->maxdc : 0;
  out[9] = c->tail_at;
  return LB_OK;
}

int lb_set_tail(lb_ctx* c, int tail_at) {
  if (!c) return fail(LB_ERR_ARG, "null context");
  if (tail_at > 0 && !c->nq) return fail(LB_ERR_UNSUPPORTED, "tail launches need variable degrees <= 12");
  c->tail_at = tail_at < 0 ? c->tail_default : tail_at;
  return LB_OK;
}

int lb_set_layers(lb_ctx* c, int nlayers, const int* first_check) {
  if (!c) return fail(LB_ERR_ARG, "bad layer arguments");
  // on the host, before anything is uploaded or changed: the layers checked, the plans made
  LayerPlan lp;
  std::string err;
  int rc = check_layers(*c, c->h_cstart.data(), c->h_evar.data(), nlayers, first_check, lp, err);
  if (rc) return fail(rc, err);
  const Switches sw = read_switches();
  lp = plan_layers(*c, lp, sw);
  const FixedPlan qp = plan_fixed(c->qfrac, c->qmsg, c->qapp, c->maxdc, lp.maxlayer, c->Nv, c->Nmsg, sw);
  HIP_TRY(hipSetDevice(c->dev));
  HIP_TRY(hipStreamSynchronize(c->stream));  // a decode may still read the old table
  int* d = nullptr;
  if ((rc = dev_alloc((void**)&d, (size_t)(nlayers + 1) * sizeof(int)))) return rc;
  if (hipMemcpyAsync(d, first_check, (size_t)(nlayers + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(d);
    return fail(LB_ERR_HIP, "layer upload failed");
  }
  (void)hipFree(c->d_lfirst);
  c->d_lfirst = d;
  static_cast<LayerPlan&>(*c) = lp;
  static_cast<FixedPlan&>(*c) = qp;
  c->raised.clear();
  return LB_OK;
}

int lb_set_fixed(lb_ctx* c, int frac_bits, int msg_bits, int app_bits) {
  if (!c) return fail(LB_ERR_ARG, "null context");
  std::string err;
  if (const int rc = check_widths(frac_bits, msg_bits, app_bits, err)) return fail(rc, err);
  FixedPlan& q = *c;
  q = FixedPlan{frac_bits, msg_bits, app_bits};
  // (the switches of the environment, read again)
  if (c->nlayers) q = plan_fixed(frac_bits, msg_bits, app_bits, c->maxdc, c->maxlayer, c->Nv, c->Nmsg, read_switches());
  return LB_OK;
}

int lb_fixed_info(lb_ctx* c, long long* out) {
  if (!c || !out) return fail(LB_ERR_ARG, "null argument");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = c->qfrac;
  out[1] = c->qmsg;
  out[2] = c->qapp;
  if (!c->nlayers) return LB_OK;
  out[3] = c->qnt;
  out[4] = c->qlanes;
  out[5] = c->qlds;
  out[7] = c->qfit ? 1 : 0;
  if (!c->qfit) return LB_OK;
  HIP_TRY(hipSetDevice(c->dev));
  DecType t;
  t.base = LB_LAYERED_MINSUM;
  t.fixed = true;
  int rc, n = 0;
  if ((rc = residency(c, t, false, &n))) return rc;
  out[6] = n;
  return LB_OK;
}

int lb_layer_info(lb_ctx* c, long long* out) {
  if (!c || !out) return fail(LB_ERR_ARG, "null argument");
  out[0] = c->nlayers;
  out[1] = c->maxlayer;
  out[2] = c->lmode;
  out[3] = c->lnt;
  return LB_OK;
}

int lb_layer_info_ex(lb_ctx* c, int precision, long long* out) {
  if (!c || !out || precision < 0 || precision > 1) return fail(LB_ERR_ARG, "bad layer info arguments");
  const bool f32 = precision == 1;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = c->nlayers;
  out[1] = c->maxlayer;
  out[2] = f32 ? c->lmode32 : c->lmode;
  out[3] = c->lnt;
  out[7] = f32 ? sizeof(float) : sizeof(double);
  if (!c->nlayers) return LB_OK;
  HIP_TRY(hipSetDevice(c->dev));
  for (int k = 0; k < 2; ++k) {  // the sumprod2 and the minsum instance
    DecType t;
    t.base = LB_LAYERED_SUMPROD2 + k;
    t.f32 = f32;
    size_t shm;
    int rc, n = 0;
    if ((rc = residency(c, t, false, &n, &shm))) return rc;
    out[4] = (long long)shm;
    out[5 + k] = n;
  }
  return LB_OK;
}

int sumprod(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg, double* app) {
  return ref_decode(ch, vdeg, cdeg, intrlv, Nv, Nc, Nmsg, app, LB_SUMPROD, 0.0);
}

int sumprod2(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg, double* app) {
  return ref_decode(ch, vdeg, cdeg, intrlv, Nv, Nc, Nmsg, app, LB_SUMPROD2, 0.0);
}

int minsum(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg, double* app,
           double correction_factor) {
  return ref_decode(ch, vdeg, cdeg, intrlv, Nv, Nc, Nmsg, app, LB_MINSUM, correction_factor);
}

static double scalar_kernel(int which, double a, double b, double* L, long dc, int corr) {
  const double nan = std::nan("");
  if (device_count() == 0) {
    fail(LB_ERR_NO_DEVICE, "no HIP device visible (there is no CPU fallback)");
    return nan;
  }
  if (which == 1 && (!L || dc < 1 || dc > 32)) {
    fail(LB_ERR_ARG, "Lxfb needs 1 <= dc <= 32");
    return nan;
  }
  if (hipSetDevice(default_device()) != hipSuccess) return nan;
  double* d = nullptr;
  if (hipMalloc((void**)&d, (33 + (size_t)(which == 1 ? dc : 0)) * sizeof(double)) != hipSuccess) {
    fail(LB_ERR_NOMEM, "hipMalloc failed");
    return nan;
  }
  double r = nan;
  bool ok = true;
  if (which == 0) {
    hipLaunchKernelGGL(k_lxor, dim3(1), dim3(1), 0, 0, a, b, corr, d);
  } else {
    ok = hipMemcpy(d + 1, L, (size_t)dc * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) hipLaunchKernelGGL(k_lxfb, dim3(1), dim3(1), 0, 0, d + 1, (int)dc, corr, d);
  }
  ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
       hipMemcpy(&r, d, sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && which == 1) ok = hipMemcpy(L, d + 1, (size_t)dc * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d);
  if (!ok) {
    fail(LB_ERR_HIP, "scalar kernel failed");
    return nan;
  }
  return r;
}

double Lxor(double L1, double L2, int corr_flag) { return scalar_kernel(0, L1, L2, nullptr, 0, corr_flag); }

double Lxfb(double* L, long dc, int corr_flag) { return scalar_kernel(1, 0, 0, L, dc, corr_flag); }

}  // extern "C"
