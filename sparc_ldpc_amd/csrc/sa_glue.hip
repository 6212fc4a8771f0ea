// sa_glue.hip — SPARC <-> LDPC glue of the joint decoder on the device
// (encoding, LLRs, bp2sp, hard / threshold decisions, cancellation).
#include "sa_host.h"
#include "sa_sc_ctx.h"

// ---------------------------------------------------------------------------
// SPARC <-> LDPC glue of the joint decoder (sparc_ldpc.py:257-314, 359-712)
// ---------------------------------------------------------------------------
// All of it runs on the device in binary64 on the B codewords of the batch;
// the LLR / app arrays are handed to and from the LDPC decoder
// (libldpc_bp.so) as device pointers, so a joint round never leaves HBM.
namespace sa {

// Columns of one-hot beta summed per row: for row r of codeword b,
//   acc = sum_{l in [l0, l0+ns)} c_l * sgn(o_lr) * H_M[k_lr, idx[b][l-l0]]
// (A[r, l*M + i] = sgn(o_lr) (-1)^popcount(k_lr & i) / sqrt(n), the same
// factorisation as the section kernels).  out = base - acc/sqrt(n) (hard
// cancellation, sparc_ldpc.py:508-518) or acc/sqrt(n) + add (encoding,
// sparc_ldpc.py:436-446).  One thread per row, idx staged in LDS.
template <typename real>
__global__ void __launch_bounds__(256) k_colsum(const ushort4* __restrict__ fwd, const double* __restrict__ cd,
                                                const int32_t* __restrict__ idx, int ldi, int l0, int ns,
                                                const real* __restrict__ base, const double* __restrict__ add,
                                                real* __restrict__ out, int n, double sqrt_n, double amp) {
  extern __shared__ int32_t sidx[];
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  for (int i = threadIdx.x; i < ns; i += 256) sidx[i] = idx[(size_t)b * ldi + i];
  __syncthreads();
  if (r >= n) return;
  double acc = 0.0;
  const int g0 = l0 / kSpw, g1 = (l0 + ns + kSpw - 1) / kSpw;
  for (int g = g0; g < g1; ++g) {
    const ushort4 f = fwd[(size_t)g * n + r];
    const unsigned short fq[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int l = g * kSpw + q;
      if (l < l0 || l >= l0 + ns || sidx[l - l0] < 0) continue;  // idx < 0: section not decided
      const unsigned k = fq[q] & 0x7fffu;
      const unsigned neg = (fq[q] >> 15) ^ (__popc(k & (unsigned)sidx[l - l0]) & 1u);
      acc += neg ? -cd[l] : cd[l];
    }
  }
  const double x = (amp == 1.0 ? acc : acc * amp) / sqrt_n;
  const size_t o = (size_t)b * n + r;
  out[o] = base ? (real)((double)base[o] - x) : (real)(x + (add ? add[o] : 0.0));
}

// Sequential ascending sum of cnt LDS values v[idx(i)], i = 0..cnt-1, with
// the loads issued 16 ahead of the dependent additions (the reference's
// order; a one-lane chain otherwise waits on every LDS read).
template <typename F>
__device__ __forceinline__ double lds_seq_sum(const double* v, int cnt, F idx) {
  double s = 0.0;
  int i = 0;
  for (; i + 16 <= cnt; i += 16) {
    double r[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) r[u] = v[idx(i + u)];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += r[u];
  }
  for (; i < cnt; ++i) s += v[idx(i)];
  return s;
}

// sp2bp + LLR (sparc_ldpc.py:470-479 -> :257-281): one wavefront per
// (codeword, LDPC section).  The section's posterior beta_j / c_l is read once
// (coalesced) into LDS; lane t < log2 M then forms p_t, the sum over the
// entries j whose bit (logM-1-t) is set, in ascending j (the reference's
// order); llr = nan_to_num(log(1 - p) - log(p)).
template <typename real>
__global__ void __launch_bounds__(64) k_llr(const real* __restrict__ beta, const double* __restrict__ cd, int L,
                                            int M, int lgM, int l0, int ns, double* __restrict__ llr) {
  extern __shared__ double post[];
  const size_t bl = blockIdx.x;  // b * ns + lp
  const int l = l0 + (int)(bl % ns);
  const real* bs = beta + ((bl / ns) * L + l) * M;
  const double c = cd[l];
  // An entry holding the whole section amplitude in the working type is a
  // decided section: posterior 1, as c_l / c_l in binary64.  (In binary32
  // (float)c_l / c_l is 1 -+ 6e-8: the bits of a decided section would get
  // |LLR| near 16.6 or, with p above 1, NaN -> 0 instead of the saturated -+max.)
  const real cr = (real)c;
  for (int j = threadIdx.x; j < M; j += 64) post[j] = bs[j] == cr ? 1.0 : (double)bs[j] / c;
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= lgM) return;
  const int sh = lgM - 1 - t, lo = (1 << sh) - 1;
  // i-th entry (ascending) whose bit sh is set
  const double p = lds_seq_sum(post, M >> 1, [=](int i) { return ((i >> sh) << (sh + 1)) | (lo + 1) | (i & lo); });
  double v = log(1.0 - p) - log(p);
  if (v != v) v = 0.0;                                 // nan_to_num: NaN -> 0
  else if (isinf(v)) v = v > 0 ? DBL_MAX : -DBL_MAX;  // +-inf -> +-max
  llr[bl * lgM + t] = v;
}

// nan_to_num and the magnitude clip of an LLR: NaN -> 0; lim > 0 bounds the
// value to [-lim, lim] (+-inf included); lim == 0 (no clip) sends +-inf to +-max.
__device__ __forceinline__ double llr_finish(double v, double lim) {
  if (v != v) return 0.0;
  if (lim > 0.0) return fmin(fmax(v, -lim), lim);
  if (isinf(v)) return v > 0 ? DBL_MAX : -DBL_MAX;
  return v;
}

// The two-sided LLR (SA_LLR_TWO_SIDED), staged like k_llr: lane t < log2 M
// forms p1_t as k_llr forms p, lane log2 M + t forms p0_t, the sum over the
// entries whose bit (logM-1-t) is clear, also in ascending j;
// llr = log(p0) - log(p1).  Neither sum is formed as 1 - (the other), so a beta
// held in binary32, whose sums carry 6e-8 of rounding, keeps its LLR beyond
// |LLR| = 16 and a sum that lands above 1 gives no NaN.
template <typename real>
__global__ void __launch_bounds__(64) k_llr2(const real* __restrict__ beta, const double* __restrict__ cd, int L,
                                             int M, int lgM, int l0, int ns, double lim, double* __restrict__ llr) {
  extern __shared__ double post[];
  const size_t bl = blockIdx.x;  // b * ns + lp
  const int l = l0 + (int)(bl % ns);
  const real* bs = beta + ((bl / ns) * L + l) * M;
  const double c = cd[l];
  const real cr = (real)c;  // a decided section: posterior 1 (see k_llr)
  for (int j = threadIdx.x; j < M; j += 64) post[j] = bs[j] == cr ? 1.0 : (double)bs[j] / c;
  __syncthreads();
  const int t = threadIdx.x;  // 2 log2 M <= 26 lanes sum (check_glue: M <= 8192)
  double p = 0.0;
  if (t < 2 * lgM) {
    const int one = t < lgM, sh = lgM - 1 - (one ? t : t - lgM), lo = (1 << sh) - 1;
    const int set = one ? lo + 1 : 0;
    // i-th entry (ascending) whose bit sh is set / clear
    p = lds_seq_sum(post, M >> 1, [=](int i) { return ((i >> sh) << (sh + 1)) | set | (i & lo); });
  }
  const double p0 = __shfl(p, (t + lgM) & 63);  // every lane of the wavefront takes part
  if (t >= lgM) return;
  llr[bl * lgM + t] = llr_finish(log(p0) - log(p), lim);
}

// The clip of SA_LLR_REFERENCE's output, in place: k_llr has already sent NaN
// to 0 and +-inf to +-max.
__global__ void k_llr_clip(double* __restrict__ llr, size_t cnt, double lim) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x)
    llr[i] = fmin(fmax(llr[i], -lim), lim);
}

// bp2sp of the LDPC a-posteriori LLRs into beta0 (sparc_ldpc.py:683-696 ->
// :283-314), one wavefront per (codeword, LDPC section): bp_t = 1/(1+exp(app_t));
// sp_m = prod_t (bit_t(m) ? bp_t : 1 - bp_t), MSB first, in LDS; the
// reference's sequential normaliser S (builtin sum, :313); beta0_m = (sp_m / S) c_l.
template <typename real>
__global__ void __launch_bounds__(64) k_soft_sec(const double* __restrict__ app, const double* __restrict__ cd,
                                                 int L, int M, int lgM, int l0, int ns, real* __restrict__ beta) {
  extern __shared__ double sp[];
  __shared__ double bpv[32];
  __shared__ double S;
  const size_t bl = blockIdx.x;  // b * ns + lp
  const int l = l0 + (int)(bl % ns);
  if (threadIdx.x < lgM) bpv[threadIdx.x] = 1.0 / (1.0 + exp(app[bl * lgM + threadIdx.x]));
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += 64) {
    double prod = 1.0;
    for (int t = 0; t < lgM; ++t) {
      const double bp = bpv[t];
      prod *= ((m >> (lgM - 1 - t)) & 1) ? bp : 1.0 - bp;
    }
    sp[m] = prod;
  }
  __syncthreads();
  if (threadIdx.x == 0) S = lds_seq_sum(sp, M, [](int i) { return i; });
  __syncthreads();
  const double c = cd[l], tot = S;
  real* o = beta + ((bl / ns) * L + l) * M;
  for (int m = threadIdx.x; m < M; m += 64) o[m] = (real)((sp[m] / tot) * c);
}

// beta0 of the sections AMP keeps (:657, :691, :696): (beta / c) * c.
template <typename real>
__global__ void k_rescale(real* __restrict__ beta, const double* __restrict__ cd, int L, int M, int l0, int ns,
                          int B) {
  const size_t tot = (size_t)B * L * M;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)((i / M) % L);
    if (l >= l0 && l < l0 + ns) continue;
    const double c = cd[l];
    beta[i] = (real)(((double)beta[i] / c) * c);
  }
}

// Hard decisions of the LDPC output (:486-490): bits = app < 0, MSB first.
__global__ void k_app_idx(const double* __restrict__ app, int lgM, int ns, int B, int32_t* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * ns) return;
  const double* a = app + (size_t)i * lgM;
  int32_t v = 0;
  for (int t = 0; t < lgM; ++t) v = (v << 1) | (a[t] < 0.0 ? 1 : 0);
  idx[i] = v;
}

// Message bits to section indices (bits2indices, sparc_ldpc.py:317): section l of codeword b takes bits
// [l lgM, (l + 1) lgM) of the codeword's L lgM bytes, MSB first; a byte counts as 1 unless it is 0.
__global__ void k_bits_idx(const uint8_t* __restrict__ bits, int lgM, int L, int B, int32_t* __restrict__ idx) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)B * L) return;
  const uint8_t* a = bits + i * lgM;
  int32_t v = 0;
  for (int t = 0; t < lgM; ++t) v = (v << 1) | (a[t] != 0 ? 1 : 0);
  idx[i] = v;
}

// One-hot beta0 (sparc_ldpc.py:832-835): beta[b][l*M + idx[b][l]] = c_l, 0 elsewhere.
template <typename real>
__global__ void k_onehot(const int32_t* __restrict__ idx, const double* __restrict__ cd, int L, int M, int B,
                         double scale, real* __restrict__ beta) {
  const size_t tot = (size_t)B * L * M;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
    const size_t bl = i / M;
    const int m = (int)(i % M), l = (int)(bl % L);
    beta[i] = m == idx[bl] ? (real)(scale == 1.0 ? cd[l] : cd[l] * scale) : (real)0;  // idx < 0: all zero
  }
}

// Threshold decisions of the LDPC soft output (amp_exit.py:56-105 on the
// bp2sp of sparc_ldpc.py:987-994): per (codeword, section) the normalised
// product of bit marginals sp_m / S; the section is decided (index m) iff
// exactly one entry exceeds the threshold, else -1.  One workgroup per
// section: products in LDS, the reference's sequential normaliser, counts.
__global__ void __launch_bounds__(256) k_threshold(const double* __restrict__ app, int M, int lgM, int ns,
                                                   double thr, int32_t* __restrict__ idx) {
  extern __shared__ double sp[];
  __shared__ int cnt, pick;
  __shared__ double S, bpv[32];
  const size_t bl = blockIdx.x;  // b * ns + section
  if (threadIdx.x < lgM) bpv[threadIdx.x] = 1.0 / (1.0 + exp(app[bl * lgM + threadIdx.x]));
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += 256) {
    double prod = 1.0;
    for (int t = 0; t < lgM; ++t) {
      const double bp = bpv[t];
      prod *= ((m >> (lgM - 1 - t)) & 1) ? bp : 1.0 - bp;
    }
    sp[m] = prod;
  }
  __syncthreads();
  if (threadIdx.x == 0) S = lds_seq_sum(sp, M, [](int i) { return i; });
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += 256)
    if (sp[m] / S > thr) {
      atomicAdd(&cnt, 1);
      pick = m;  // only read when cnt == 1
    }
  __syncthreads();
  if (threadIdx.x == 0) idx[bl] = cnt == 1 ? pick : -1;
}

int grid_of(size_t tot) {
  const size_t g = (tot + 255) / 256;
  return (int)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

constexpr int kGlueMaxM = 8192;  // a section of fp64 in the 64 KiB of dynamic LDS

int check_glue(sa_ctx* c, int B, int l0, int ns) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || B > c->Bcap) return fail(SA_ERR_ARG, "batch larger than the context's workspace");
  if (l0 < 0 || ns <= 0 || l0 + ns > c->L) return fail(SA_ERR_ARG, "section range outside [0, L)");
  if (!c->power_set) return fail(SA_ERR_ARG, "power allocation not staged");
  if (c->M < 2) return fail(SA_ERR_UNSUPPORTED, "M < 2 carries no bits");
  if (!c->pow2) return fail(SA_ERR_UNSUPPORTED, "bit-level glue needs M a power of two (bits2indices, sparc_ldpc.py:317)");
  if (c->M > kGlueMaxM) return fail(SA_ERR_UNSUPPORTED, "SPARC<->LDPC glue stages a section in LDS: M <= 8192");
  return SA_OK;
}

// Host-or-device fp64 array of `count` values on the context's device:
// returns a device pointer (copying host data into the staging buffer).
int dev_in(sa_ctx* c, const double* p, size_t count, int flags, const double** out) {
  if (flags & SA_PTR_DEVICE) {
    *out = p;
    return SA_OK;
  }
  int rc = ensure_stage(c, count);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->at().d_stage, p, count * 8, hipMemcpyHostToDevice, c->at().stream));
  *out = c->at().d_stage;
  return SA_OK;
}

template <typename real>
int launch_colsum(sa_ctx* c, const int32_t* d_idx, int ldi, int l0, int ns, const real* base, const double* add,
                  real* out, int B, double amp = 1.0) {
  dim3 grid((c->n + 255) / 256, B);
  k_colsum<real><<<grid, 256, (size_t)ns * sizeof(int32_t), c->at().stream>>>(
      (const ushort4*)c->tab.fwd, c->d_cd, d_idx, ldi, l0, ns, base, add, out, c->n, std::sqrt((double)c->n), amp);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

// What sa_encode and sa_encode_bits check before anything else (`who`), and the workspace for B codewords.
int encode_begin(sa_ctx* c, int B, bool args_ok, const std::string& who) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || !args_ok) return fail(SA_ERR_ARG, who + ": bad arguments");
  if (!c->power_set) return fail(SA_ERR_ARG, who + ": power allocation not staged");
  if (int rc0 = check_tables(c, who.c_str())) return rc0;
  if (!c->pow2) return fail(SA_ERR_UNSUPPORTED, who + ": the row-parallel encoder needs M a power of two");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_workspace(c, B, c->Tcap > 0 ? c->Tcap : 1);
}

// The encoder on the device: y = A beta(d_idx) + d_noise (NULL: none) of B codewords becomes the current lane's
// staged y, from the section indices queued into c->d_idx on that lane's stream; idx_out (host, or NULL) receives
// them.  Blocking.
int encode_staged(sa_ctx* c, int B, const double* d_noise, int32_t* idx_out) {
  sa_lane& ln = c->at();
  int rc;
  if ((rc = y_begin_write(c, ln.stream, B))) return rc;  // the current lane's y becomes the staged one
  rc = c->prec == SA_PREC_F64
           ? launch_colsum<double>(c, c->d_idx, c->L, 0, c->L, nullptr, d_noise, (double*)ln.d_y, B)
           : launch_colsum<float>(c, c->d_idx, c->L, 0, c->L, nullptr, d_noise, (float*)ln.d_y, B);
  if (rc) return rc;
  if (idx_out)
    HIP_TRY(hipMemcpyAsync(idx_out, c->d_idx, (size_t)B * c->L * sizeof(int32_t), hipMemcpyDeviceToHost, ln.stream));
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return y_mark(c);
}

int launch_bits_idx(hipStream_t stream, const uint8_t* d_bits, int lgM, int L, int B, int32_t* d_idx) {
  const size_t tot = (size_t)B * L;
  k_bits_idx<<<(unsigned)((tot + 255) / 256), 256, 0, stream>>>(d_bits, lgM, L, B, d_idx);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

// ---- the same glue on a coupled context's d_beta ----
// What every coupled glue call checks first: the section range (sa_sc.h:
// sc_glue_check), then the batch and the staged state (sc_stage_rule).
int sc_glue_begin(sa_sc* s, int call, int B, int l0, int ns, const char* who) {
  if (!s) return fail(SA_ERR_ARG, std::string(who) + ": null context");
  std::string err;
  if (int rc = sc_glue_check(s->lay, l0, ns, err)) return fail(rc, std::string(who) + ": " + err);
  if (int rc = sc_stage_rule(s->st, call, B, s->Bcap, err)) return fail(rc, std::string(who) + ": " + err);
  HIP_TRY(hipSetDevice(s->parent->device));
  return SA_OK;
}

// dev_in for a coupled context: the device pointer itself, or the host values copied into the staging buffer
int sc_dev_in(sa_sc* s, const double* p, size_t count, int flags, const double** out) {
  if (flags & SA_PTR_DEVICE) {
    *out = p;
    return SA_OK;
  }
  if (int rc = sc_stage(s, count)) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_stage, p, count * 8, hipMemcpyHostToDevice, s->stream));
  *out = s->d_stage;
  return SA_OK;
}

}  // namespace sa

using namespace sa;

extern "C" {

int sa_encode(sa_ctx* c, int B, const int32_t* idx, const double* noise) {
  int rc = encode_begin(c, B, idx != nullptr, "sa_encode");
  if (rc) return rc;
  sa_lane& ln = c->at();
  for (size_t i = 0; i < (size_t)B * c->L; ++i)
    if (idx[i] < 0 || idx[i] >= c->M) return fail(SA_ERR_ARG, "sa_encode: index outside [0, M)");
  HIP_TRY(hipMemcpyAsync(c->d_idx, idx, (size_t)B * c->L * sizeof(int32_t), hipMemcpyHostToDevice, ln.stream));
  const double* d_noise = nullptr;
  if (noise && (rc = dev_in(c, noise, (size_t)B * c->n, 0, &d_noise))) return rc;
  return encode_staged(c, B, d_noise, nullptr);
}

int sa_encode_bits(sa_ctx* c, int B, const uint8_t* d_bits, const double* d_noise, int32_t* idx_out) {
  int rc = encode_begin(c, B, d_bits != nullptr, "sa_encode_bits");
  if (rc) return rc;
  if (c->M < 2) return fail(SA_ERR_UNSUPPORTED, "sa_encode_bits: M < 2 carries no bits");
  const size_t tot = (size_t)B * c->L;
  k_bits_idx<<<(unsigned)((tot + 255) / 256), 256, 0, c->at().stream>>>(d_bits, ilog2(c->M), c->L, B, c->d_idx);
  HIP_TRY(hipGetLastError());
  return encode_staged(c, B, d_noise, idx_out);
}

namespace {
int stage_onehot_impl(sa_ctx* c, int B, const int32_t* idx, double scale, bool allow_empty) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || B > c->Bcap || !idx) return fail(SA_ERR_ARG, "sa_stage_onehot: bad arguments");
  if (!c->power_set) return fail(SA_ERR_ARG, "sa_stage_onehot: power allocation not staged");
  if (!std::isfinite(scale)) return fail(SA_ERR_ARG, "sa_stage_onehot: scale must be finite");
  if (c->dead) return fail(SA_ERR_UNSUPPORTED, "sa_stage_onehot: M must be a power of two (bits2indices)");
  for (size_t i = 0; i < (size_t)B * c->L; ++i)
    if (idx[i] >= c->M || (idx[i] < 0 && !(allow_empty && idx[i] == -1)))
      return fail(SA_ERR_ARG, "sa_stage_onehot: index outside [0, M)");
  HIP_TRY(hipSetDevice(c->device));
  sa_lane& ln = c->at();
  tail_beta_rewritten(ln);
  HIP_TRY(hipMemcpyAsync(c->d_idx, idx, (size_t)B * c->L * sizeof(int32_t), hipMemcpyHostToDevice, ln.stream));
  const size_t tot = (size_t)B * c->L * c->M;
  if (c->prec == SA_PREC_F64)
    k_onehot<double><<<grid_of(tot), 256, 0, ln.stream>>>(c->d_idx, c->d_cd, c->L, c->M, B, scale, (double*)ln.d_beta);
  else
    k_onehot<float><<<grid_of(tot), 256, 0, ln.stream>>>(c->d_idx, c->d_cd, c->L, c->M, B, scale, (float*)ln.d_beta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return SA_OK;
}
}  // namespace

int sa_stage_onehot(sa_ctx* c, int B, const int32_t* idx) { return stage_onehot_impl(c, B, idx, 1.0, false); }

int sa_stage_onehot_scaled(sa_ctx* c, int B, const int32_t* idx, double scale) {
  return stage_onehot_impl(c, B, idx, scale, true);
}

int sa_llr(sa_ctx* c, int B, int l0, int ns, double* llr, int flags) {
  return sa_llr_ex(c, B, l0, ns, llr, flags, SA_LLR_REFERENCE, INFINITY);
}

int sa_llr_ex(sa_ctx* c, int B, int l0, int ns, double* llr, int flags, int mode, double clip) {
  int rc = check_glue(c, B, l0, ns);
  if (rc) return rc;
  if (!llr) return fail(SA_ERR_ARG, "sa_llr: llr is NULL");
  if (mode != SA_LLR_REFERENCE && mode != SA_LLR_TWO_SIDED) return fail(SA_ERR_ARG, "sa_llr_ex: unknown mode");
  if (!(clip >= 0.0)) return fail(SA_ERR_ARG, "sa_llr_ex: clip must be positive, or 0 / +inf for none");
  const double lim = std::isinf(clip) ? 0.0 : clip;  // 0: no clip
  HIP_TRY(hipSetDevice(c->device));
  sa_lane& ln = c->at();
  const int lgM = ilog2(c->M);
  const size_t cnt = (size_t)B * ns * lgM;
  double* d_out = llr;
  if (!(flags & SA_PTR_DEVICE)) {
    if ((rc = ensure_stage(c, cnt))) return rc;
    d_out = ln.d_stage;
  }
  const size_t lds = (size_t)c->M * sizeof(double);
  if (mode == SA_LLR_TWO_SIDED) {
    if (c->prec == SA_PREC_F64)
      k_llr2<double><<<B * ns, 64, lds, ln.stream>>>((const double*)ln.d_beta, c->d_cd, c->L, c->M, lgM, l0, ns, lim,
                                                     d_out);
    else
      k_llr2<float><<<B * ns, 64, lds, ln.stream>>>((const float*)ln.d_beta, c->d_cd, c->L, c->M, lgM, l0, ns, lim,
                                                    d_out);
  } else {
    if (c->prec == SA_PREC_F64)
      k_llr<double><<<B * ns, 64, lds, ln.stream>>>((const double*)ln.d_beta, c->d_cd, c->L, c->M, lgM, l0, ns, d_out);
    else
      k_llr<float><<<B * ns, 64, lds, ln.stream>>>((const float*)ln.d_beta, c->d_cd, c->L, c->M, lgM, l0, ns, d_out);
    if (lim > 0.0) k_llr_clip<<<grid_of(cnt), 256, 0, ln.stream>>>(d_out, cnt, lim);
  }
  HIP_TRY(hipGetLastError());
  if (!(flags & SA_PTR_DEVICE)) HIP_TRY(hipMemcpyAsync(llr, d_out, cnt * 8, hipMemcpyDeviceToHost, ln.stream));
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return SA_OK;
}

int sa_soft_beta0(sa_ctx* c, int B, int l0, int ns, const double* app, int flags) {
  int rc = check_glue(c, B, l0, ns);
  if (rc) return rc;
  if (!app) return fail(SA_ERR_ARG, "sa_soft_beta0: app is NULL");
  HIP_TRY(hipSetDevice(c->device));
  sa_lane& ln = c->at();
  tail_beta_rewritten(ln);
  const int lgM = ilog2(c->M);
  const size_t na = (size_t)B * ns * lgM;
  const double* d_app = app;
  if (!(flags & SA_PTR_DEVICE)) {
    if ((rc = ensure_stage(c, na))) return rc;
    HIP_TRY(hipMemcpyAsync(ln.d_stage, app, na * 8, hipMemcpyHostToDevice, ln.stream));
    d_app = ln.d_stage;
  }
  const size_t tot = (size_t)B * c->L * c->M, lds = (size_t)c->M * sizeof(double);
  if (c->prec == SA_PREC_F64) {
    if (ns < c->L) k_rescale<double><<<grid_of(tot), 256, 0, ln.stream>>>((double*)ln.d_beta, c->d_cd, c->L, c->M, l0, ns, B);
    k_soft_sec<double><<<B * ns, 64, lds, ln.stream>>>(d_app, c->d_cd, c->L, c->M, lgM, l0, ns, (double*)ln.d_beta);
  } else {
    if (ns < c->L) k_rescale<float><<<grid_of(tot), 256, 0, ln.stream>>>((float*)ln.d_beta, c->d_cd, c->L, c->M, l0, ns, B);
    k_soft_sec<float><<<B * ns, 64, lds, ln.stream>>>(d_app, c->d_cd, c->L, c->M, lgM, l0, ns, (float*)ln.d_beta);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return SA_OK;
}

int sa_hard_cancel(sa_ctx* c, int B, int l0, int ns, const double* app, int flags, sa_ctx* dst, int32_t* idx_out) {
  if (dst && check_tables(c, "sa_hard_cancel")) return SA_ERR_UNSUPPORTED;
  int rc = check_glue(c, B, l0, ns);
  if (rc) return rc;
  if (!app) return fail(SA_ERR_ARG, "sa_hard_cancel: app is NULL");
  if (dst && (dst->n != c->n || dst->prec != c->prec || dst->device != c->device))
    return fail(SA_ERR_ARG, "sa_hard_cancel: dst must share n, precision and device");
  HIP_TRY(hipSetDevice(c->device));
  if (dst && (rc = ensure_workspace(dst, B, dst->Tcap > 0 ? dst->Tcap : 1))) return rc;
  sa_lane& ln = c->at();  // (dst may be c: after its workspace)
  const int lgM = ilog2(c->M);
  const double* d_app = nullptr;
  if ((rc = dev_in(c, app, (size_t)B * ns * lgM, flags, &d_app))) return rc;
  k_app_idx<<<(B * ns + 255) / 256, 256, 0, ln.stream>>>(d_app, lgM, ns, B, c->d_idx);
  HIP_TRY(hipGetLastError());
  if (dst) {
    // reads the staged y (wherever it was staged), writes dst's
    if ((rc = y_sync(c)) || (rc = y_begin_write(dst, ln.stream, B))) return rc;
    rc = c->prec == SA_PREC_F64
             ? launch_colsum<double>(c, c->d_idx, ns, l0, ns, (const double*)ln.d_y, nullptr, (double*)dst->at().d_y, B)
             : launch_colsum<float>(c, c->d_idx, ns, l0, ns, (const float*)ln.d_y, nullptr, (float*)dst->at().d_y, B);
    if (rc) return rc;
  }
  if (idx_out)
    HIP_TRY(hipMemcpyAsync(idx_out, c->d_idx, (size_t)B * ns * sizeof(int32_t), hipMemcpyDeviceToHost, ln.stream));
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return dst ? y_mark(dst) : SA_OK;
}

int sa_threshold(sa_ctx* c, int B, int l0, int ns, const double* app, int flags, double threshold,
                 int32_t* idx_out) {
  int rc = check_glue(c, B, l0, ns);
  if (rc) return rc;
  if (!app || !idx_out) return fail(SA_ERR_ARG, "sa_threshold: null argument");
  HIP_TRY(hipSetDevice(c->device));
  sa_lane& ln = c->at();
  const int lgM = ilog2(c->M);
  const double* d_app = nullptr;
  if ((rc = dev_in(c, app, (size_t)B * ns * lgM, flags, &d_app))) return rc;
  k_threshold<<<B * ns, 256, (size_t)c->M * sizeof(double), ln.stream>>>(d_app, c->M, lgM, ns, threshold, c->d_idx);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(idx_out, c->d_idx, (size_t)B * ns * sizeof(int32_t), hipMemcpyDeviceToHost, ln.stream));
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return SA_OK;
}

int sa_cancel_scaled(sa_ctx* c, int B, const int32_t* idx, double scale, sa_ctx* dst) {
  if (check_ctx(c) || check_ctx(dst)) return SA_ERR_ARG;
  if (int rc0 = check_tables(c, "sa_cancel")) return rc0;
  if (!c->pow2) return fail(SA_ERR_UNSUPPORTED, "sa_cancel: needs M a power of two");
  if (B <= 0 || B > c->Bcap || !idx) return fail(SA_ERR_ARG, "sa_cancel: bad arguments");
  if (!c->power_set) return fail(SA_ERR_ARG, "sa_cancel: power allocation not staged");
  if (dst->n != c->n || dst->prec != c->prec || dst->device != c->device)
    return fail(SA_ERR_ARG, "sa_cancel: dst must share n, precision and device");
  for (size_t i = 0; i < (size_t)B * c->L; ++i)
    if (idx[i] >= c->M) return fail(SA_ERR_ARG, "sa_cancel: index >= M");
  if (!std::isfinite(scale)) return fail(SA_ERR_ARG, "sa_cancel: scale must be finite");
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_workspace(dst, B, dst->Tcap > 0 ? dst->Tcap : 1))) return rc;
  sa_lane& ln = c->at();  // (dst may be c: after its workspace)
  HIP_TRY(hipMemcpyAsync(c->d_idx, idx, (size_t)B * c->L * sizeof(int32_t), hipMemcpyHostToDevice, ln.stream));
  if ((rc = y_sync(c)) || (rc = y_begin_write(dst, ln.stream, B))) return rc;  // as sa_hard_cancel
  rc = c->prec == SA_PREC_F64
           ? launch_colsum<double>(c, c->d_idx, c->L, 0, c->L, (const double*)ln.d_y, nullptr, (double*)dst->at().d_y, B, scale)
           : launch_colsum<float>(c, c->d_idx, c->L, 0, c->L, (const float*)ln.d_y, nullptr, (float*)dst->at().d_y, B, scale);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return y_mark(dst);
}

int sa_cancel(sa_ctx* c, int B, const int32_t* idx, sa_ctx* dst) { return sa_cancel_scaled(c, B, idx, 1.0, dst); }

int sa_sc_llr(sa_sc* s, int B, int l0, int ns, double* llr, int flags, int mode, double clip) {
  if (s && !llr) return fail(SA_ERR_ARG, "sa_sc_llr: llr is NULL");
  if (mode != SA_LLR_REFERENCE && mode != SA_LLR_TWO_SIDED) return fail(SA_ERR_ARG, "sa_sc_llr: unknown mode");
  if (!(clip >= 0.0)) return fail(SA_ERR_ARG, "sa_sc_llr: clip must be positive, or 0 / +inf for none");
  int rc = sc_glue_begin(s, SC_CALL_LLR, B, l0, ns, "sa_sc_llr");
  if (rc) return rc;
  const double lim = std::isinf(clip) ? 0.0 : clip;  // 0: no clip
  const ScLayout& y = s->lay;
  const int lgM = ilog2(y.M);
  const size_t cnt = (size_t)B * ns * lgM;
  double* d_out = llr;
  if (!(flags & SA_PTR_DEVICE)) {
    if ((rc = sc_stage(s, cnt))) return rc;
    d_out = s->d_stage;
  }
  const size_t lds = (size_t)y.M * sizeof(double);
  if (mode == SA_LLR_TWO_SIDED) {
    if (y.prec == SA_PREC_F64)
      k_llr2<double><<<B * ns, 64, lds, s->stream>>>((const double*)s->d_beta, s->d_cd, y.L, y.M, lgM, l0, ns, lim, d_out);
    else
      k_llr2<float><<<B * ns, 64, lds, s->stream>>>((const float*)s->d_beta, s->d_cd, y.L, y.M, lgM, l0, ns, lim, d_out);
  } else {
    if (y.prec == SA_PREC_F64)
      k_llr<double><<<B * ns, 64, lds, s->stream>>>((const double*)s->d_beta, s->d_cd, y.L, y.M, lgM, l0, ns, d_out);
    else
      k_llr<float><<<B * ns, 64, lds, s->stream>>>((const float*)s->d_beta, s->d_cd, y.L, y.M, lgM, l0, ns, d_out);
    if (lim > 0.0) k_llr_clip<<<grid_of(cnt), 256, 0, s->stream>>>(d_out, cnt, lim);
  }
  HIP_TRY(hipGetLastError());
  if (!(flags & SA_PTR_DEVICE)) HIP_TRY(hipMemcpyAsync(llr, d_out, cnt * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

int sa_sc_soft_beta0(sa_sc* s, int B, int l0, int ns, const double* app, int flags) {
  if (s && !app) return fail(SA_ERR_ARG, "sa_sc_soft_beta0: app is NULL");
  int rc = sc_glue_begin(s, SC_CALL_SOFT_BETA0, B, l0, ns, "sa_sc_soft_beta0");
  if (rc) return rc;
  const ScLayout& y = s->lay;
  const int lgM = ilog2(y.M);
  const double* d_app = nullptr;
  if ((rc = sc_dev_in(s, app, (size_t)B * ns * lgM, flags, &d_app))) return rc;
  const size_t tot = (size_t)B * y.L * y.M, lds = (size_t)y.M * sizeof(double);
  if (y.prec == SA_PREC_F64) {
    if (ns < y.L) k_rescale<double><<<grid_of(tot), 256, 0, s->stream>>>((double*)s->d_beta, s->d_cd, y.L, y.M, l0, ns, B);
    k_soft_sec<double><<<B * ns, 64, lds, s->stream>>>(d_app, s->d_cd, y.L, y.M, lgM, l0, ns, (double*)s->d_beta);
  } else {
    if (ns < y.L) k_rescale<float><<<grid_of(tot), 256, 0, s->stream>>>((float*)s->d_beta, s->d_cd, y.L, y.M, l0, ns, B);
    k_soft_sec<float><<<B * ns, 64, lds, s->stream>>>(d_app, s->d_cd, y.L, y.M, lgM, l0, ns, (float*)s->d_beta);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

int sa_sc_hard_indices(sa_sc* s, int B, int l0, int ns, const double* app, int flags, int32_t* idx_out) {
  if (s && (!app || !idx_out)) return fail(SA_ERR_ARG, "sa_sc_hard_indices: null argument");
  int rc = sc_glue_begin(s, SC_CALL_HARD, B, l0, ns, "sa_sc_hard_indices");
  if (rc) return rc;
  const int lgM = ilog2(s->lay.M);
  const double* d_app = nullptr;
  if ((rc = sc_dev_in(s, app, (size_t)B * ns * lgM, flags, &d_app))) return rc;
  k_app_idx<<<(B * ns + 255) / 256, 256, 0, s->stream>>>(d_app, lgM, ns, B, s->d_idx);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(idx_out, s->d_idx, (size_t)B * ns * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

int sa_sc_stage_onehot(sa_sc* s, int B, const int32_t* idx) {
  if (s && !idx) return fail(SA_ERR_ARG, "sa_sc_stage_onehot: idx is NULL");
  if (s && B >= 1 && B <= s->Bcap)
    for (size_t i = 0; i < (size_t)B * s->lay.L; ++i)
      if (idx[i] < 0 || idx[i] >= s->lay.M) return fail(SA_ERR_ARG, "sa_sc_stage_onehot: index outside [0, M)");
  int rc = sc_glue_begin(s, SC_CALL_ONEHOT, B, 0, s ? s->lay.L : 1, "sa_sc_stage_onehot");
  if (rc) return rc;
  const ScLayout& y = s->lay;
  HIP_TRY(hipMemcpyAsync(s->d_idx, idx, (size_t)B * y.L * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  const size_t tot = (size_t)B * y.L * y.M;
  if (y.prec == SA_PREC_F64)
    k_onehot<double><<<grid_of(tot), 256, 0, s->stream>>>(s->d_idx, s->d_cd, y.L, y.M, B, 1.0, (double*)s->d_beta);
  else
    k_onehot<float><<<grid_of(tot), 256, 0, s->stream>>>(s->d_idx, s->d_cd, y.L, y.M, B, 1.0, (float*)s->d_beta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

}  // extern "C"
