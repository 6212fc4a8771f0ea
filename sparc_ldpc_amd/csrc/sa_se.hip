// sa_se.hip — state evolution (SE) of the AMP decoder on one device: the
// scalar recursion that predicts the effective noise variance tau_t^2 and the
// section error rate of a decode, iteration by iteration, without a codeword
// (sa_se, sa_se_draws; context-free like sa_draw_reps).
//
// For an allocation Pl (P = sum Pl), section size M, code length n, noise sigma:
//   tau_0^2 = sigma^2 + P,  c_l = sqrt(n Pl_l),  a = c_l / tau_t,
//   E_l(tau_t) = E[ e^(a^2 + a U_1) / (e^(a^2 + a U_1) + sum_{j >= 2} e^(a U_j)) ],  U_j i.i.d. N(0, 1)
//   x_{t+1} = sum_l (Pl_l / P) E_l(tau_t),  tau_{t+1}^2 = sigma^2 + P (1 - x_{t+1}),
// the decoder's own section softmax (sparc_ldpc.py:213-219) applied to
// s = c e_true + tau U.  A section is missed when a^2 + a U_1 < max_{j >= 2} a U_j.
//
// The expectation is a mean over S rows U[s] of M Gaussians, the same rows for
// every section, iteration and allocation of a call (common random numbers: a
// call is deterministic and two allocations are compared on the same noise).
//
//  * k_se_draw: row s = RandomState(seeds[s]).randn(M), one workgroup per row
//    (legacy_mt_dev.h);
//  * k_se_expect, one launch per iteration: the sections of an allocation that
//    carry the same power (bit for bit) are one class with a multiplicity, the
//    classes of the whole batch form one list.  A workgroup takes a chunk of
//    SC samples (their rows in LDS, loaded once) and kSeClasses classes; a
//    wave takes a (class, sample) pair at a time: only the scalar a changes
//    from class to class, and max_{j >= 2} a U_j = a max_{j >= 2} U_j (rounding
//    is monotone, a >= 0) is taken once per row.  The chunk's posterior sum and
//    miss count of each class go to the workgroup's own slot;
//  * k_se_reduce, one workgroup per allocation: the slots of each class added
//    in a fixed order (lane-strided, then the xor tree), the classes' weighted
//    sum the same way, x_{t+1} and tau_{t+1}^2 written to device memory, where
//    the next iteration's launch reads tau^2.
// No floating-point atomics, no grid-wide barrier: every sum has one order, so
// two calls on the same inputs return the same bits, and an allocation's
// result does not depend on what else is in the batch.  Binary64 throughout.
//
// The second half of the file is the same for spatially coupled SPARCs
// (sa_sc_se; host rules: sa_scse.h): one phi_r per row
// block, one tau_c^2 per column block, classes per (configuration, column
// block), k_scse_expect and k_scse_reduce in the places of the two kernels
// above.
#include "sa_common.h"
#include "legacy_mt_dev.h"
#include "sa_scse.h"

#include <unordered_map>

namespace sa {

// (kSeMaxM, kSeRow, kSeSamples, kSeClasses: sa_scse.h, where the host rules size the chunks)
constexpr int kSeThreads = 256;
constexpr int kSeRedThreads = 1024;

struct SeArgs {
  const double* U;      // [S][M]
  const double* cls_c;  // [K] c = sqrt(n Pl) of the class
  const int* cls_b;     // [K] its allocation
  const double* tau2;   // [B][T1]
  double* part_p;       // [K][NCH] posterior sums per sample chunk
  int* part_m;          // [K][NCH] miss counts
  int S, M, K, NCH, SC, T1, t;
};

__device__ __forceinline__ int se_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long se_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One (class, sample) pair on one wave: the posterior of the true column and
// whether the pair is missed, for the scalar av = c / tau, the sample's row u
// and umax = max_{j >= 2} U_j of that row.  Uniform results.
__device__ __forceinline__ void se_pair(double av, const double* u, double umax, int M, int lane, double& post, int& miss) {
#pragma clang fp contract(off)
  const double l0 = av * av + av * u[0];  // the true column's logit
  const double mo = av * umax;            // the largest of the others
  const double mx = fmax(l0, mo);
  double sum = 0;
#pragma unroll 4
  for (int j = 1 + lane; j < M; j += 64) sum += exp(av * u[j] - mx);
  sum = wave_sum(sum);
  const double e0 = exp(l0 - mx);
  post = e0 / (e0 + sum);
  miss = l0 < mo ? 1 : 0;
}

// (No contraction in the kernels below: the operations are those of the
// NumPy statements the tests hold them to, tests/se_ref.py and
// tests/sc_se_ref.py, one rounding each; what differs is the device library's
// exp and the order of the sums.)
__global__ void __launch_bounds__(kSeThreads) k_se_expect(SeArgs a) {
#pragma clang fp contract(off)
  __shared__ double rows[kSeRow];
  __shared__ double umax[kSeSamples];
  __shared__ double post[kSeClasses * kSeSamples];
  __shared__ int missf[kSeClasses * kSeSamples];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ch = (int)(blockIdx.x % (unsigned)a.NCH), kc = (int)(blockIdx.x / (unsigned)a.NCH);
  const int M = a.M;
  const int s0 = ch * a.SC, ns = min(a.SC, a.S - s0);
  const int k0 = kc * kSeClasses, nk = min(kSeClasses, a.K - k0);
  // the chunk's rows (ns * M <= SC * M <= kSeRow)
  const double* src = a.U + (size_t)s0 * M;
  for (int i = tid; i < ns * M; i += kSeThreads) rows[i] = src[i];
  __syncthreads();
  // max_{j >= 2} U_j of each row (columns 1 .. M - 1 here; M >= 2)
  for (int s = wv; s < ns; s += kSeThreads / 64) {
    double m = -INFINITY;
    for (int j = 1 + lane; j < M; j += 64) m = fmax(m, rows[s * M + j]);
    m = wave_max(m);
    if (lane == 0) umax[s] = m;
  }
  __syncthreads();
  for (int item = wv; item < nk * ns; item += kSeThreads / 64) {
    const int kk = item / ns, s = item - kk * ns, k = k0 + kk;
    const double tau2 = a.tau2[(size_t)a.cls_b[k] * a.T1 + a.t];
    const double av = a.cls_c[k] / sqrt(tau2);
    double pv;
    int mv;
    se_pair(av, rows + s * M, umax[s], M, lane, pv, mv);
    if (lane == 0) {
      post[kk * kSeSamples + s] = pv;
      missf[kk * kSeSamples + s] = mv;
    }
  }
  __syncthreads();
  if (tid < nk) {  // the chunk's samples in order
    double p = 0;
    int mc = 0;
    for (int s = 0; s < ns; ++s) {
      p += post[tid * kSeSamples + s];
      mc += missf[tid * kSeSamples + s];
    }
    a.part_p[(size_t)(k0 + tid) * a.NCH + ch] = p;
    a.part_m[(size_t)(k0 + tid) * a.NCH + ch] = mc;
  }
}

struct SeRedArgs {
  const double* part_p;
  const int* part_m;
  const int* off;        // [B + 1] class range of each allocation
  const double* cls_w;   // [K] multiplicity * Pl / P
  const int* cls_mult;   // [K]
  const double* sig2;    // [B]
  const double* P;       // [B]
  double* tau2;          // [B][T + 1]
  double* x;             // [B][T]
  long long* miss;       // [B][T]
  double* ek;            // [K] E of the class (the last launch's stay)
  double* wx;            // [K] scratch: weight * E
  long long* mk;         // [K] scratch: multiplicity * misses
  int NCH, S, T, t;
};

__global__ void __launch_bounds__(kSeRedThreads) k_se_reduce(SeRedArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k0 = a.off[b], k1 = a.off[b + 1];
  for (int k = k0 + wv; k < k1; k += kSeRedThreads / 64) {
    const double* pp = a.part_p + (size_t)k * a.NCH;
    const int* pm = a.part_m + (size_t)k * a.NCH;
    double s = 0;
    int mc = 0;
    for (int c = lane; c < a.NCH; c += 64) {
      s += pp[c];
      mc += pm[c];
    }
    s = wave_sum(s);
    mc = se_wave_sum(mc);
    if (lane == 0) {
      const double E = s / (double)a.S;
      a.ek[k] = E;
      a.wx[k] = a.cls_w[k] * E;
      a.mk[k] = (long long)a.cls_mult[k] * mc;
    }
  }
  __syncthreads();
  if (wv == 0) {
    double s = 0;
    long long mm = 0;
    for (int k = k0 + lane; k < k1; k += 64) {
      s += a.wx[k];
      mm += a.mk[k];
    }
    s = wave_sum(s);
    mm = se_wave_sum(mm);
    if (lane == 0) {
      a.x[(size_t)b * a.T + a.t] = s;
      a.tau2[(size_t)b * (a.T + 1) + a.t + 1] = a.sig2[b] + a.P[b] * (1.0 - s);
      a.miss[(size_t)b * a.T + a.t] = mm;
    }
  }
}

// ---- coupled state evolution (sa_sc_se) ----------------------------------------
// k_scse_expect is k_se_expect with two differences: a class reads tau^2 from
// its tau slot (configuration, column block) of the iteration, and for t >= 1
// a class whose slot holds the bits it held at t - 1 is frozen: E is a
// deterministic function of (tau^2, U), so its [class][chunk] slots already
// hold what this launch would write, and its exponentials are skipped.  A
// workgroup whose classes are all frozen returns after the test.
struct ScSeArgs {
  const double* U;           // [S][M]
  const double* cls_c;       // [K] c = sqrt(n Pl) of the class
  const long long* cls_tau;  // [K] where its tau slot of t = 0 lies in tau2
  const double* tau2;        // [B][T + 1][Cmax]
  double* part_p;            // [K][NCH] posterior sums per sample chunk
  int* part_m;               // [K][NCH] miss counts
  int S, M, K, NCH, SC, Cmax, t, skip;
};

__global__ void __launch_bounds__(kSeThreads) k_scse_expect(ScSeArgs a) {
#pragma clang fp contract(off)
  __shared__ double rows[kSeRow];
  __shared__ double umax[kSeSamples];
  __shared__ double post[kSeClasses * kSeSamples];
  __shared__ int missf[kSeClasses * kSeSamples];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ch = (int)(blockIdx.x % (unsigned)a.NCH), kc = (int)(blockIdx.x / (unsigned)a.NCH);
  const int M = a.M;
  const int s0 = ch * a.SC, ns = min(a.SC, a.S - s0);
  const int k0 = kc * kSeClasses, nk = min(kSeClasses, a.K - k0);
  // the live classes of this workgroup (uniform: every thread tests all nk <= 8)
  const long long* tbits = (const long long*)a.tau2;
  const long long trow = (long long)a.t * a.Cmax;
  unsigned live = 0;
  for (int kk = 0; kk < nk; ++kk) {
    const long long at = a.cls_tau[k0 + kk] + trow;
    const bool frozen = a.skip && a.t > 0 && tbits[at] == tbits[at - a.Cmax];
    if (!frozen) live |= 1u << kk;
  }
  if (!live) return;
  const double* src = a.U + (size_t)s0 * M;
  for (int i = tid; i < ns * M; i += kSeThreads) rows[i] = src[i];
  __syncthreads();
  for (int s = wv; s < ns; s += kSeThreads / 64) {
    double m = -INFINITY;
    for (int j = 1 + lane; j < M; j += 64) m = fmax(m, rows[s * M + j]);
    m = wave_max(m);
    if (lane == 0) umax[s] = m;
  }
  __syncthreads();
  for (int item = wv; item < nk * ns; item += kSeThreads / 64) {
    const int kk = item / ns, s = item - kk * ns, k = k0 + kk;
    if (!((live >> kk) & 1u)) continue;
    const double tau2 = a.tau2[a.cls_tau[k] + trow];
    const double av = a.cls_c[k] / sqrt(tau2);
    double pv;
    int mv;
    se_pair(av, rows + s * M, umax[s], M, lane, pv, mv);
    if (lane == 0) {
      post[kk * kSeSamples + s] = pv;
      missf[kk * kSeSamples + s] = mv;
    }
  }
  __syncthreads();
  if (tid < nk && ((live >> tid) & 1u)) {  // the chunk's samples in order
    double p = 0;
    int mc = 0;
    for (int s = 0; s < ns; ++s) {
      p += post[tid * kSeSamples + s];
      mc += missf[tid * kSeSamples + s];
    }
    a.part_p[(size_t)(k0 + tid) * a.NCH + ch] = p;
    a.part_m[(size_t)(k0 + tid) * a.NCH + ch] = mc;
  }
}

// One workgroup per configuration.  A wave per class adds its slots as
// k_se_reduce does; then, in the first wave, lane c forms x_c, psi_c and the
// block's miss count over its classes in class order, lane r forms
// phi_r^{t+1} in c order, and lane c forms tau_c^2^{t+1} in r order: the slot
// the next launch reads (sa_scse.h: scse_phi_tau is the same on the host).
// The predicted stop index is written once: the first t + 1 at which every
// phi_r has the bits of the row before.
struct ScSeRedArgs {
  const double* part_p;
  const int* part_m;
  const int* cfg_off;      // [B + 1] class range of each configuration
  const int* slot_off;     // [B + 1] its tau slots
  const int* blk_off;      // [NS + 1] class range of each tau slot
  const long long* w_off;  // [B + 1] its base matrix in W
  const int* R;            // [B]
  const int* C;            // [B]
  const double* W;
  const double* cls_w;     // [K] multiplicity * Pl / P_c
  const int* cls_mult;     // [K]
  const double* sig2;      // [B]
  const double* Pc;        // [NS]
  double* phi;             // [B][T + 1][Rmax]
  double* tau2;            // [B][T + 1][Cmax]
  double* x;               // [B][T][Cmax]
  long long* miss;         // [B][T][Cmax]
  long long* stop;         // [B], T until written
  double* ek;              // [K] E of the class (the last launch's stay)
  double* wx;              // [K] scratch: weight * E
  long long* mk;           // [K] scratch: multiplicity * misses
  int NCH, S, T, t, Rmax, Cmax;
};

__global__ void __launch_bounds__(kSeRedThreads) k_scse_reduce(ScSeRedArgs a) {
#pragma clang fp contract(off)
  __shared__ double psi[kScSeMaxBlocks];
  __shared__ double phis[kScSeMaxBlocks];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k0 = a.cfg_off[b], k1 = a.cfg_off[b + 1];
  for (int k = k0 + wv; k < k1; k += kSeRedThreads / 64) {
    const double* pp = a.part_p + (size_t)k * a.NCH;
    const int* pm = a.part_m + (size_t)k * a.NCH;
    double s = 0;
    int mc = 0;
    for (int c = lane; c < a.NCH; c += 64) {
      s += pp[c];
      mc += pm[c];
    }
    s = wave_sum(s);
    mc = se_wave_sum(mc);
    if (lane == 0) {
      const double E = s / (double)a.S;
      a.ek[k] = E;
      a.wx[k] = a.cls_w[k] * E;
      a.mk[k] = (long long)a.cls_mult[k] * mc;
    }
  }
  __syncthreads();
  const int R = a.R[b], C = a.C[b], q0 = a.slot_off[b];  // R, C <= 64: one lane per block
  const double* W = a.W + a.w_off[b];
  if (wv == 0 && lane < C) {
    double x = 0;
    long long mm = 0;
    for (int k = a.blk_off[q0 + lane]; k < a.blk_off[q0 + lane + 1]; ++k) {
      x += a.wx[k];
      mm += a.mk[k];
    }
    psi[lane] = a.Pc[q0 + lane] * (1.0 - x);
    a.x[((size_t)b * a.T + a.t) * a.Cmax + lane] = x;
    a.miss[((size_t)b * a.T + a.t) * a.Cmax + lane] = mm;
  }
  __syncthreads();
  if (wv == 0) {
    bool same = true;
    if (lane < R) {
      double acc = 0;
      for (int c = 0; c < C; ++c) acc += W[(size_t)lane * C + c] * psi[c];
      const double ph = a.sig2[b] + acc;
      double* row = a.phi + ((size_t)b * (a.T + 1) + a.t + 1) * a.Rmax;
      same = __double_as_longlong(ph) == __double_as_longlong(row[lane - a.Rmax]);
      row[lane] = ph;
      phis[lane] = ph;
    }
    const bool all = __all(same ? 1 : 0);
    if (lane == 0 && all && a.stop[b] == a.T) a.stop[b] = a.t + 1;
  }
  __syncthreads();
  if (wv == 0 && lane < C) {
    double acc = 0;
    for (int r = 0; r < R; ++r) acc += W[(size_t)r * C + lane] / phis[r];
    a.tau2[((size_t)b * (a.T + 1) + a.t + 1) * a.Cmax + lane] = 1.0 / (acc / (double)R);
  }
}

// Row s = RandomState(seeds[s]).randn(M) (legacy_mt_dev.h).  A row whose randn
// runs into the chunk cap sets *err.
__global__ void __launch_bounds__(legacy_rng_dev::kThreads) k_se_draw(const uint32_t* __restrict__ seeds,
                                                                      double* __restrict__ U, int M, int max_chunks,
                                                                      long long* err) {
  __shared__ legacy_rng_dev::State st;
  const int s = blockIdx.x;
  legacy_rng_dev::seed_state(st, seeds[s]);
  int have = 0;
  const bool ok = legacy_rng_dev::draw_randn(st, have, 0, M, false, 1.0, U + (size_t)s * M, max_chunks);
  if (!ok && threadIdx.x == 0) *err = 1;
}

namespace {

// the device buffers, stream and events of one call
struct SeScope {
  std::vector<void*> bufs;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~SeScope() {
    for (void* p : bufs) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
  int open(const char* what, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SA_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(SA_ERR_ARG, std::string(what) + ": device index out of range");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    return SA_OK;
  }
  template <typename T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SA_ERR_NOMEM, "device allocation failed");
    }
    bufs.push_back(q);
    *p = (T*)q;
    return SA_OK;
  }
  template <typename T>
  int put(T** p, const T* h, size_t count) {
    if (int rc = alloc(p, count)) return rc;
    HIP_TRY(hipMemcpyAsync(*p, h, count * sizeof(T), hipMemcpyHostToDevice, st));
    return SA_OK;
  }
};

int se_draw(SeScope& sc, const uint32_t* seeds, int S, int M, double* d_U, long long* d_err) {
  uint32_t* d_seeds = nullptr;
  if (int rc = sc.put(&d_seeds, seeds, (size_t)S)) return rc;
  k_se_draw<<<S, legacy_rng_dev::kThreads, 0, sc.st>>>(d_seeds, d_U, M, legacy_rng_dev::randn_chunk_cap(M), d_err);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

}  // namespace
}  // namespace sa

using namespace sa;

extern "C" {

int sa_se_draws(int device, int S, int M, const uint32_t* seeds, double* U_out) {
  if (S < 1) return fail(SA_ERR_ARG, "sa_se_draws: S < 1");
  if (M < 1) return fail(SA_ERR_ARG, "sa_se_draws: M < 1");
  if (!seeds || !U_out) return fail(SA_ERR_ARG, "sa_se_draws: seeds and U_out must be given");
  if (M > (1 << 27)) return fail(SA_ERR_UNSUPPORTED, "sa_se_draws: M above 2^27");
  SeScope sc;
  if (int rc = sc.open("sa_se_draws", device)) return rc;
  double* d_U = nullptr;
  long long* d_err = nullptr;
  int rc;
  if ((rc = sc.alloc(&d_U, (size_t)S * M))) return rc;
  if ((rc = sc.alloc(&d_err, 1))) return rc;
  HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(long long), sc.st));
  if ((rc = se_draw(sc, seeds, S, M, d_U, d_err))) return rc;
  std::vector<double> h((size_t)S * M);
  long long err = 0;
  HIP_TRY(hipMemcpyAsync(h.data(), d_U, h.size() * sizeof(double), hipMemcpyDeviceToHost, sc.st));
  HIP_TRY(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, sc.st));
  HIP_TRY(hipStreamSynchronize(sc.st));
  if (err) return fail(SA_ERR_HIP, "sa_se_draws: a row's randn ran into the chunk cap");
  std::memcpy(U_out, h.data(), h.size() * sizeof(double));
  return SA_OK;
}

int sa_se(int device, int B, int L, int M, int n, const double* Pl, const double* sigma, int T, int S,
          const uint32_t* seeds, const double* U, double* tau2_out, double* x_out, int64_t* miss_out,
          double* sec_out, double* ms_out) {
  if (B < 1) return fail(SA_ERR_ARG, "sa_se: B < 1");
  if (L < 1) return fail(SA_ERR_ARG, "sa_se: L < 1");
  if (M < 2) return fail(SA_ERR_ARG, "sa_se: M < 2");
  if (n < 1) return fail(SA_ERR_ARG, "sa_se: n < 1");
  if (T < 1) return fail(SA_ERR_ARG, "sa_se: T < 1");
  if (S < 1) return fail(SA_ERR_ARG, "sa_se: S < 1");
  if (!Pl || !sigma || !tau2_out || !x_out || !miss_out)
    return fail(SA_ERR_ARG, "sa_se: Pl, sigma, tau2_out, x_out and miss_out must be given");
  if ((seeds != nullptr) == (U != nullptr)) return fail(SA_ERR_ARG, "sa_se: exactly one of seeds and U must be given");
  for (int b = 0; b < B; ++b)
    if (!(sigma[b] > 0) || !std::isfinite(sigma[b]))
      return fail(SA_ERR_ARG, "sa_se: sigma[" + std::to_string(b) + "] must be finite and > 0");
  // the classes: per allocation the distinct powers in order of first appearance
  std::vector<double> cls_c, cls_w, sig2(B), Pb(B), tau2_0((size_t)B);
  std::vector<int> cls_b, cls_mult, off(B + 1, 0), sec_cls((size_t)B * L);
  for (int b = 0; b < B; ++b) {
    const double* pl = Pl + (size_t)b * L;
    long double acc = 0;
    for (int l = 0; l < L; ++l) {
      if (!(pl[l] >= 0) || !std::isfinite(pl[l]))
        return fail(SA_ERR_ARG, "sa_se: Pl[" + std::to_string(b) + "][" + std::to_string(l) + "] must be finite and >= 0");
      acc += pl[l];
    }
    const double P = (double)acc;
    if (!(P > 0)) return fail(SA_ERR_ARG, "sa_se: P = sum(Pl) is 0 for allocation " + std::to_string(b));
    if (!std::isfinite(P)) return fail(SA_ERR_ARG, "sa_se: P = sum(Pl) overflows for allocation " + std::to_string(b));
    std::unordered_map<uint64_t, int> seen;
    const int k0 = (int)cls_c.size();
    std::vector<double> cls_pl;
    for (int l = 0; l < L; ++l) {
      uint64_t bits;
      std::memcpy(&bits, &pl[l], sizeof(bits));
      auto it = seen.find(bits);
      if (it == seen.end()) {
        it = seen.emplace(bits, (int)cls_c.size()).first;
        cls_c.push_back(std::sqrt((double)n * pl[l]));
        cls_pl.push_back(pl[l]);
        cls_mult.push_back(0);
        cls_b.push_back(b);
      }
      ++cls_mult[it->second];
      sec_cls[(size_t)b * L + l] = it->second;
    }
    for (size_t k = k0; k < cls_c.size(); ++k) cls_w.push_back((double)cls_mult[k] * cls_pl[k - k0] / P);
    off[b + 1] = (int)cls_c.size();
    Pb[b] = P;
    sig2[b] = sigma[b] * sigma[b];
    tau2_0[b] = sig2[b] + P;
  }
  if (M > kSeMaxM) return fail(SA_ERR_UNSUPPORTED, "sa_se: M above SA_SE_MAX_M = " + std::to_string(kSeMaxM));
  if (S > (1 << 24)) return fail(SA_ERR_UNSUPPORTED, "sa_se: S above 2^24");
  const int K = (int)cls_c.size();
  const int SC = std::max(1, std::min(kSeSamples, kSeRow / M));
  const int NCH = (S + SC - 1) / SC;
  const long long grid = (long long)NCH * ((K + kSeClasses - 1) / kSeClasses);
  if (grid >= (1LL << 31)) return fail(SA_ERR_UNSUPPORTED, "sa_se: classes x sample chunks above 2^31 workgroups");

  SeScope sc;
  int rc;
  if ((rc = sc.open("sa_se", device))) return rc;
  // one block of results: tau2 [B][T + 1] | x [B][T] | E [K] | misses [B][T] | the draw's error flag
  const size_t n_tau = (size_t)B * (T + 1), n_x = (size_t)B * T, n_res = n_tau + n_x + K + n_x + 1;
  std::vector<double> res(n_res, 0.0);
  for (int b = 0; b < B; ++b) res[(size_t)b * (T + 1)] = tau2_0[b];
  double* d_res = nullptr;
  if ((rc = sc.put(&d_res, res.data(), n_res))) return rc;
  double* d_tau2 = d_res;
  double* d_x = d_res + n_tau;
  double* d_ek = d_x + n_x;
  long long* d_miss = (long long*)(d_ek + K);
  long long* d_err = d_miss + n_x;
  double *d_U = nullptr, *d_c = nullptr, *d_w = nullptr, *d_sig2 = nullptr, *d_P = nullptr, *d_pp = nullptr, *d_wx = nullptr;
  int *d_b = nullptr, *d_mult = nullptr, *d_off = nullptr, *d_pm = nullptr;
  long long* d_mk = nullptr;
  if ((rc = sc.put(&d_c, cls_c.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_w, cls_w.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_b, cls_b.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_mult, cls_mult.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_off, off.data(), (size_t)B + 1))) return rc;
  if ((rc = sc.put(&d_sig2, sig2.data(), (size_t)B))) return rc;
  if ((rc = sc.put(&d_P, Pb.data(), (size_t)B))) return rc;
  if ((rc = sc.alloc(&d_pp, (size_t)K * NCH))) return rc;
  if ((rc = sc.alloc(&d_pm, (size_t)K * NCH))) return rc;
  if ((rc = sc.alloc(&d_wx, (size_t)K))) return rc;
  if ((rc = sc.alloc(&d_mk, (size_t)K))) return rc;
  if (U) {
    if ((rc = sc.put(&d_U, U, (size_t)S * M))) return rc;
  } else {
    if ((rc = sc.alloc(&d_U, (size_t)S * M))) return rc;
  }
  HIP_TRY(hipEventRecord(sc.e0, sc.st));
  if (seeds && (rc = se_draw(sc, seeds, S, M, d_U, d_err))) return rc;
  SeArgs ea;
  ea.U = d_U; ea.cls_c = d_c; ea.cls_b = d_b; ea.tau2 = d_tau2; ea.part_p = d_pp; ea.part_m = d_pm;
  ea.S = S; ea.M = M; ea.K = K; ea.NCH = NCH; ea.SC = SC; ea.T1 = T + 1; ea.t = 0;
  SeRedArgs ra;
  ra.part_p = d_pp; ra.part_m = d_pm; ra.off = d_off; ra.cls_w = d_w; ra.cls_mult = d_mult; ra.sig2 = d_sig2;
  ra.P = d_P; ra.tau2 = d_tau2; ra.x = d_x; ra.miss = d_miss; ra.ek = d_ek; ra.wx = d_wx; ra.mk = d_mk;
  ra.NCH = NCH; ra.S = S; ra.T = T; ra.t = 0;
  // every iteration queued on the one stream; the host waits once, below
  for (int t = 0; t < T; ++t) {
    ea.t = ra.t = t;
    k_se_expect<<<(unsigned)grid, kSeThreads, 0, sc.st>>>(ea);
    k_se_reduce<<<B, kSeRedThreads, 0, sc.st>>>(ra);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sc.e1, sc.st));
  HIP_TRY(hipMemcpyAsync(res.data(), d_res, n_res * sizeof(double), hipMemcpyDeviceToHost, sc.st));
  HIP_TRY(hipStreamSynchronize(sc.st));
  long long err = 0;
  std::memcpy(&err, res.data() + n_tau + n_x + K + n_x, sizeof(err));
  if (err) return fail(SA_ERR_HIP, "sa_se: a row's randn ran into the chunk cap");
  std::memcpy(tau2_out, res.data(), n_tau * sizeof(double));
  std::memcpy(x_out, res.data() + n_tau, n_x * sizeof(double));
  std::memcpy(miss_out, res.data() + n_tau + n_x + K, n_x * sizeof(int64_t));
  if (sec_out) {
    const double* ek = res.data() + n_tau + n_x;
    for (size_t i = 0; i < (size_t)B * L; ++i) sec_out[i] = ek[sec_cls[i]];
  }
  if (ms_out) {
    float ms = -1.f;
    HIP_TRY(hipEventElapsedTime(&ms, sc.e0, sc.e1));
    *ms_out = ms;
  }
  return SA_OK;
}

int sa_sc_se(int device, int B, int L, int M, const int* n, const int* R, const int* C, const double* W,
             const double* Pl, const double* sigma, int T, int S, const uint32_t* seeds, const double* U, int Rmax,
             int Cmax, int flags, double* phi_out, double* tau2_out, double* x_out, int64_t* miss_out, int* stop_out,
             double* sec_out, double* ms_out) {
  if (!phi_out || !tau2_out || !x_out || !miss_out || !stop_out)
    return fail(SA_ERR_ARG, "sa_sc_se: phi_out, tau2_out, x_out, miss_out and stop_out must be given");
  if ((seeds != nullptr) == (U != nullptr)) return fail(SA_ERR_ARG, "sa_sc_se: exactly one of seeds and U must be given");
  if (flags & ~SA_SCSE_NO_SKIP) return fail(SA_ERR_ARG, "sa_sc_se: unknown flags");
  ScSePlan p;
  std::string err;
  if (int rc = scse_plan(p, B, L, M, n, R, C, W, Pl, sigma, T, S, err)) return fail(rc, "sa_sc_se: " + err);
  if (Rmax < p.Rmax) return fail(SA_ERR_ARG, "sa_sc_se: Rmax below the largest R of the batch");
  if (Cmax < p.Cmax) return fail(SA_ERR_ARG, "sa_sc_se: Cmax below the largest C of the batch");
  const int K = p.K, NCH = p.NCH;
  std::vector<long long> cls_tau((size_t)K);
  for (int b = 0; b < B; ++b)
    for (int k = p.cfg_off[b]; k < p.cfg_off[b + 1]; ++k)
      cls_tau[k] = (long long)b * (T + 1) * Cmax + (p.cls_slot[k] - p.slot_off[b]);

  SeScope sc;
  int rc;
  if ((rc = sc.open("sa_sc_se", device))) return rc;
  // one block of results: phi [B][T + 1][Rmax] | tau2 [B][T + 1][Cmax] | x [B][T][Cmax] | E [K] |
  // misses [B][T][Cmax] | stop [B] | the draw's error flag; zero where a configuration has no block
  const size_t n_phi = (size_t)B * (T + 1) * Rmax, n_tau = (size_t)B * (T + 1) * Cmax, n_x = (size_t)B * T * Cmax;
  const size_t o_tau = n_phi, o_x = o_tau + n_tau, o_ek = o_x + n_x, o_miss = o_ek + K, o_stop = o_miss + n_x,
               o_err = o_stop + B, n_res = o_err + 1;
  std::vector<double> res(n_res, 0.0);
  const long long stop0 = T;
  for (int b = 0; b < B; ++b) {
    std::memcpy(&res[(size_t)b * (T + 1) * Rmax], &p.phi0[p.row_off[b]], (size_t)p.R[b] * sizeof(double));
    std::memcpy(&res[o_tau + (size_t)b * (T + 1) * Cmax], &p.tau20[p.slot_off[b]], (size_t)p.C[b] * sizeof(double));
    std::memcpy(&res[o_stop + b], &stop0, sizeof(stop0));
  }
  double* d_res = nullptr;
  if ((rc = sc.put(&d_res, res.data(), n_res))) return rc;
  double *d_U = nullptr, *d_c = nullptr, *d_w = nullptr, *d_sig2 = nullptr, *d_Pc = nullptr, *d_W = nullptr, *d_pp = nullptr,
         *d_wx = nullptr;
  int *d_mult = nullptr, *d_cfg = nullptr, *d_slot = nullptr, *d_blk = nullptr, *d_R = nullptr, *d_C = nullptr, *d_pm = nullptr;
  long long *d_mk = nullptr, *d_ctau = nullptr, *d_woff = nullptr;
  if ((rc = sc.put(&d_c, p.cls_c.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_w, p.cls_w.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_mult, p.cls_mult.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_ctau, cls_tau.data(), (size_t)K))) return rc;
  if ((rc = sc.put(&d_cfg, p.cfg_off.data(), (size_t)B + 1))) return rc;
  if ((rc = sc.put(&d_slot, p.slot_off.data(), (size_t)B + 1))) return rc;
  if ((rc = sc.put(&d_blk, p.blk_off.data(), (size_t)p.NS + 1))) return rc;
  if ((rc = sc.put(&d_woff, p.w_off.data(), (size_t)B + 1))) return rc;
  if ((rc = sc.put(&d_R, p.R.data(), (size_t)B))) return rc;
  if ((rc = sc.put(&d_C, p.C.data(), (size_t)B))) return rc;
  if ((rc = sc.put(&d_W, W, (size_t)p.w_off[B]))) return rc;
  if ((rc = sc.put(&d_sig2, p.sig2.data(), (size_t)B))) return rc;
  if ((rc = sc.put(&d_Pc, p.Pc.data(), (size_t)p.NS))) return rc;
  if ((rc = sc.alloc(&d_pp, (size_t)K * NCH))) return rc;
  if ((rc = sc.alloc(&d_pm, (size_t)K * NCH))) return rc;
  if ((rc = sc.alloc(&d_wx, (size_t)K))) return rc;
  if ((rc = sc.alloc(&d_mk, (size_t)K))) return rc;
  if (U) {
    if ((rc = sc.put(&d_U, U, (size_t)S * M))) return rc;
  } else {
    if ((rc = sc.alloc(&d_U, (size_t)S * M))) return rc;
  }
  long long* d_err = (long long*)(d_res + o_err);
  HIP_TRY(hipEventRecord(sc.e0, sc.st));
  if (seeds && (rc = se_draw(sc, seeds, S, M, d_U, d_err))) return rc;
  ScSeArgs ea;
  ea.U = d_U; ea.cls_c = d_c; ea.cls_tau = d_ctau; ea.tau2 = d_res + o_tau; ea.part_p = d_pp; ea.part_m = d_pm;
  ea.S = S; ea.M = M; ea.K = K; ea.NCH = NCH; ea.SC = p.SC; ea.Cmax = Cmax; ea.t = 0;
  ea.skip = (flags & SA_SCSE_NO_SKIP) ? 0 : 1;
  ScSeRedArgs ra;
  ra.part_p = d_pp; ra.part_m = d_pm; ra.cfg_off = d_cfg; ra.slot_off = d_slot; ra.blk_off = d_blk; ra.w_off = d_woff;
  ra.R = d_R; ra.C = d_C; ra.W = d_W; ra.cls_w = d_w; ra.cls_mult = d_mult; ra.sig2 = d_sig2; ra.Pc = d_Pc;
  ra.phi = d_res; ra.tau2 = d_res + o_tau; ra.x = d_res + o_x; ra.miss = (long long*)(d_res + o_miss);
  ra.stop = (long long*)(d_res + o_stop); ra.ek = d_res + o_ek; ra.wx = d_wx; ra.mk = d_mk;
  ra.NCH = NCH; ra.S = S; ra.T = T; ra.t = 0; ra.Rmax = Rmax; ra.Cmax = Cmax;
  // every iteration queued on the one stream; the host waits once, below
  for (int t = 0; t < T; ++t) {
    ea.t = ra.t = t;
    k_scse_expect<<<(unsigned)p.grid, kSeThreads, 0, sc.st>>>(ea);
    k_scse_reduce<<<B, kSeRedThreads, 0, sc.st>>>(ra);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sc.e1, sc.st));
  HIP_TRY(hipMemcpyAsync(res.data(), d_res, n_res * sizeof(double), hipMemcpyDeviceToHost, sc.st));
  HIP_TRY(hipStreamSynchronize(sc.st));
  long long derr = 0;
  std::memcpy(&derr, res.data() + o_err, sizeof(derr));
  if (derr) return fail(SA_ERR_HIP, "sa_sc_se: a row's randn ran into the chunk cap");
  std::memcpy(phi_out, res.data(), n_phi * sizeof(double));
  for (int b = 0; b < B; ++b)  // the T rows the iterations read (row T is formed, never read)
    std::memcpy(tau2_out + (size_t)b * T * Cmax, res.data() + o_tau + (size_t)b * (T + 1) * Cmax, (size_t)T * Cmax * sizeof(double));
  std::memcpy(x_out, res.data() + o_x, n_x * sizeof(double));
  std::memcpy(miss_out, res.data() + o_miss, n_x * sizeof(int64_t));
  for (int b = 0; b < B; ++b) {
    long long s = 0;
    std::memcpy(&s, res.data() + o_stop + b, sizeof(s));
    stop_out[b] = (int)s;
  }
  if (sec_out) {
    const double* ek = res.data() + o_ek;
    for (size_t i = 0; i < (size_t)B * L; ++i) sec_out[i] = ek[p.sec_cls[i]];
  }
  if (ms_out) {
    float ms = -1.f;
    HIP_TRY(hipEventElapsedTime(&ms, sc.e0, sc.e1));
    *ms_out = ms;
  }
  return SA_OK;
}

}  // extern "C"
