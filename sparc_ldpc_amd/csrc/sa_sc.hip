// sa_sc.hip — AMP for spatially coupled SPARCs on the sub-sampled Hadamard
// operator: the block-aware section kernel k_scsec, the row kernel k_scrow and
// the sa_sc_* C ABI (include/sparc_amp.h).  The host rules (validation, block
// maps, group layout, limits, LDS bytes) are sa_sc.h; the equations and the
// launch sequence are DESIGN.md section 13.
//
// The coupled design is A[i, j] = sqrt(W[r(i), c(j)]) At[i, j] over the parent
// context's +-1/sqrt(n) operator At, so the factorisation of the uncoupled
// kernels carries over: per section one bucket gather of a scaled z, one
// M-point FWHT, the section denoiser, a second FWHT and a signed row gather
// (k_sec is the model), with the block weights applied to z in front of the
// gather (A^T) and to the groups' partials in the row kernel (A).  A coupled
// context borrows the parent's bucket table (and its Ab table where the column
// blocks are whole groups of four sections) and has its own stream and buffers.
#include "sa_sc_ctx.h"

namespace sa {

enum { SC_AMP = 0, SC_AB = 1, SC_AZ = 2 };
enum { SCR_INIT = 0, SCR_AMP = 1, SCR_ABOUT = 2 };

template <typename real>
struct ScSecArgs {
  const uint16_t* __restrict__ inv;  // [L][w] the parent's bucket table
  const ushort4* __restrict__ fwd;   // [G][n] Ab table of the section groups
  const real* __restrict__ c;        // [L] sqrt(n Pl)
  const real* __restrict__ W;        // [R][C]
  const real* __restrict__ sqW;      // [R][C] sqrt(W)
  const real* __restrict__ z;        // [B][n]
  real* __restrict__ beta;           // [B][L*M] read and written in place (each section by its own wave)
  real* __restrict__ out;            // [B][L*M] (SC_AZ)
  real* __restrict__ abp;            // [B][G][n] unweighted Ab partials of the groups
  real* __restrict__ bbp;            // [B][G] beta^2 partials
  const real* __restrict__ zzp;      // [B][NZ] z^2 partials, zpb per row block
  real* __restrict__ phi;            // [B][T][R] the trace
  int* __restrict__ iters;           // [B] stop index, -1 while running
  const int* __restrict__ done;      // [B] set by k_scrow in the launch after the stop
  int L, M, n, w, nhi, G, gpc, Lc, R, C, nr, zpb, NZ, T, t, mode, early_stop;
  real sqrt_n;
  static constexpr bool wave = false;
};

// The wave form's arguments: the tolerance stop and the
// frozen column blocks.  SC_AMP only.
template <typename real>
struct ScWaveArgs : ScSecArgs<real> {
  real stop_tol, freeze_tol;       // in the working precision; freeze_tol == 0: every block live
  real* __restrict__ taul;         // [B][2][C] tau_c^2 of block c's last live iteration, by the parity of t
  unsigned char* __restrict__ live;  // [B][T][C] the live bits, or null
  static constexpr bool wave = true;
};

template <typename real>
struct ScRowArgs {
  const real* __restrict__ y;     // [B][n]
  real* __restrict__ z;           // [B][n]
  const real* __restrict__ abp;   // [B][G][n]
  const real* __restrict__ bbp;   // [B][G]
  const real* __restrict__ W;     // [R][C]
  const real* __restrict__ sqW;   // [R][C]
  const real* __restrict__ Pc;    // [C] sum of Pl over a column block
  const real* __restrict__ phi;   // [B][T][R]
  real* __restrict__ zzp;         // [B][NZ]
  real* __restrict__ out;         // [B][n] (SCR_ABOUT)
  const double* __restrict__ noise;  // [B][n] added in binary64 (SCR_ABOUT: the encoder), or null
  int* __restrict__ iters;
  int* __restrict__ done;
  int n, G, gpc, R, C, nr, zpb, NZ, T, t, mode;
  real sqrt_n;
};

// Section kernel: one workgroup = one section group (4 waves, one section each,
// all of column block cb) of one codeword (blockIdx.y).
//  - phi_r = sum of row block r's z^2 partials / n_r, wave wv taking r = wv,
//    wv + 4, ... (a fixed order: the same bits in every workgroup); the stop
//    (every phi_r equal to the previous iteration's, bit for bit) from the trace;
//  - 1 / tau_c^2 = (1 / R) sum_r W[r, cb] / phi_r, summed in r order;
//  - z staged into LDS as v_i = z_i sqrt(W[r(i), cb]) tau_c^2 / phi_r(i), so the
//    bucket gather, the FWHT and denoise_section(cl, tau_c^2) give
//    u = (beta + At^T v) c_l / tau_c^2 as in the uncoupled kernels;
//  - T_l = H_M beta_l staged, the group's unweighted Ab partial of every row.
// SC_AB: the partials of the beta given.  SC_AZ: out = At^T (z sqrt(W[r, cb])) / sqrt(n).
//
// The wave form (Args = ScWaveArgs, SC_AMP; section 13b) stops on
// |phi_r - last| <= stop_tol * last for every r and, with freeze_tol > 0 at
// t > 0, leaves a block whose tau_c^2 is within freeze_tol of taul_c (that of
// its last live iteration) alone: its workgroups return behind the phi / tau
// prologue, in front of the z staging, and beta, abp and bbp of the block stay
// as its last live iteration wrote them (k_scrow re-reads them).  taul is read
// at parity t - 1 by every group and written at parity t by the block's first
// group, frozen or live, so no workgroup reads a word another one of the same
// launch writes.  Where a block may be frozen the table loads (bucket table,
// beta, c_l, the first Ab rows) are issued behind the test, not at entry.  The
// test is uniform over the workgroup: every thread forms the same tau_c^2 bits.
template <typename real, int E, typename Args = ScSecArgs<real>>
__global__ void __launch_bounds__(256) k_scsec(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KH = E >= 16 ? 2 : 16;
  constexpr int NQ = (E + 3) / 4;
  const int g = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = a.M, n = a.n;
  const size_t LM = (size_t)a.L * M;
  const int mlanes = M < 64 ? M : 64;
  const int cb = g / a.gpc, ls = (g % a.gpc) * kSpw + wv;
  const bool have = ls < a.Lc;                       // absent: padding of the block's last group
  const int l = cb * a.Lc + (have ? ls : a.Lc - 1);  // clamped section for unconditional loads

  real* zs = reinterpret_cast<real*>(smem);
  const int zslots = ((n + 1) * (int)sizeof(real) + 15) / 16 * 16 / (int)sizeof(real);
  real* ts = zs + zslots;            // [kSpw][M]
  real* bbw = ts + kSpw * M;         // [kSpw]
  real* phis = bbw + kSpw;           // [kScMaxBlocks] phi_r
  real* trm = phis + kScMaxBlocks;   // [kScMaxBlocks] W[r, cb] / phi_r
  real* scl = trm + kScMaxBlocks;    // [kScMaxBlocks] the z scale of row block r
  int* neqw = reinterpret_cast<int*>(scl + kScMaxBlocks);  // [kSpw] a phi_r of the wave differs from the last

  real v[E];
  real bprev[E];
  real* bl = a.beta + (size_t)b * LM + (size_t)l * M;
  const uint16_t* il = a.inv + (size_t)l * a.w;
  const ushort4* fw = a.fwd + (size_t)g * n;
  constexpr int KR = 8;  // rows per thread whose Ab-table loads are in flight together
  ushort4 f[KR];
  bool late = false;  // wave form: the block may be frozen, so the table loads wait for the test
  real tlp = 0;       // taul_c as the previous iteration left it
  if constexpr (Args::wave) {
    late = a.mode == SC_AMP && a.t > 0 && a.freeze_tol > (real)0;
    if (late) tlp = a.taul[((size_t)b * 2 + ((a.t - 1) & 1)) * a.C + cb];
  }
  if (a.mode != SC_AZ && !(Args::wave && late)) {  // the first rows' entries with the kernel's first loads (as k_sec)
#pragma unroll
    for (int u = 0; u < KR; ++u) {
      const int r = u * 256 + tid;
      f[u] = fw[r < n ? r : 0];
    }
  }

  if (a.mode == SC_AB) {
    load_section<real, E>(bl, v, lane, M);
  } else {
    // a codeword that stopped in an earlier launch (uniform over the grid row:
    // k_scrow wrote done[b] in a launch of its own)
    if (a.mode == SC_AMP && a.done[b]) return;
    ushort4 tb[KH][NQ];
    real cl;
    if constexpr (!Args::wave) {
      load_buckets<E, KH>(il, 0, a.nhi, M, lane, tb);
      if (a.mode == SC_AMP) load_section<real, E>(bl, bprev, lane, M);
      cl = ld_vmem(a.c + l);
    } else {
      cl = 0;
      if (!late) {
        load_buckets<E, KH>(il, 0, a.nhi, M, lane, tb);
        load_section<real, E>(bl, bprev, lane, M);
        cl = ld_vmem(a.c + l);
      }
    }
    real tau2 = 1;
    if (a.mode == SC_AMP) {
      // every z^2 partial and the previous phi in one memory round trip, through
      // LDS: the z slots are free until the staging (NZ <= n: sc_check_layout)
      const real* zzb = a.zzp + (size_t)b * a.NZ;
      for (int i = tid; i < a.NZ; i += 256) zs[i] = zzb[i];
      if (a.t > 0 && tid < a.R) trm[tid] = a.phi[((size_t)b * a.T + a.t - 1) * a.R + tid];
      __syncthreads();
      bool neq = a.t == 0;
      for (int r = wv; r < a.R; r += kSpw) {  // lane i adds partials i, i + 64, ... in order, then the fixed butterfly
        real s = 0;
        for (int i = lane; i < a.zpb; i += 64) s += zs[r * a.zpb + i];
        const real ph = wave_sum(s) / (real)a.nr;
        if constexpr (Args::wave) {
          if (a.t > 0) neq = neq || !(fabs(ph - trm[r]) <= a.stop_tol * trm[r]);  // stop_tol = 0: bit equality
        } else {
          if (a.t > 0) neq = neq || !(ph == trm[r]);
        }
        if (lane == 0) phis[r] = ph;
      }
      if (lane == 0) neqw[wv] = neq ? 1 : 0;
      __syncthreads();
      const bool stop = a.early_stop && a.t > 0 && !(neqw[0] | neqw[1] | neqw[2] | neqw[3]);
      if (stop) {  // uniform over the grid row: beta, z stay as they are; the trace row stays zero
        if (g == 0 && tid == 0 && a.iters[b] < 0) a.iters[b] = a.t;
        return;
      }
      if (g == 0 && tid < a.R) a.phi[((size_t)b * a.T + a.t) * a.R + tid] = phis[tid];
      if (tid < a.R) trm[tid] = a.W[tid * a.C + cb] / phis[tid];
      __syncthreads();
      real acc = 0;
      for (int r = 0; r < a.R; ++r) acc += trm[r];
      tau2 = (real)a.R / acc;
      if constexpr (Args::wave) {
        const bool live = !late || fabs(tau2 - tlp) > a.freeze_tol * tlp;
        if (g % a.gpc == 0 && tid == 0) {
          a.taul[((size_t)b * 2 + (a.t & 1)) * a.C + cb] = live ? tau2 : tlp;
          if (a.live) a.live[((size_t)b * a.T + a.t) * a.C + cb] = live ? 1 : 0;
        }
        if (!live) return;  // frozen: uniform over the workgroup, no barrier waits on it
        if (late) {
#pragma unroll
          for (int u = 0; u < KR; ++u) {
            const int r = u * 256 + tid;
            f[u] = fw[r < n ? r : 0];
          }
          load_buckets<E, KH>(il, 0, a.nhi, M, lane, tb);
          load_section<real, E>(bl, bprev, lane, M);
          cl = ld_vmem(a.c + l);
        }
      }
      if (tid < a.R) scl[tid] = a.sqW[tid * a.C + cb] * tau2 / phis[tid];
    } else {
      if (tid < a.R) scl[tid] = a.sqW[tid * a.C + cb];
    }
    __syncthreads();
    const real* zb = a.z + (size_t)b * n;
    for (int i = tid; i < n; i += 256) zs[i] = zb[i] * scl[i / a.nr];
    if (tid == 0) zs[n] = 0;  // the zero slot of empty buckets
    __syncthreads();

#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = 0;
    for (int h0 = 0; h0 < a.nhi; h0 += KH) {
      ushort4 tn[KH][NQ];
      const bool more = h0 + KH < a.nhi;
      if (more) load_buckets<E, KH>(il, h0 + KH, a.nhi, M, lane, tn);
      gather_buckets<real, E, KH>(zs, h0, a.nhi, tb, v);
      if (more) {
#pragma unroll
        for (int hh = 0; hh < KH; ++hh)
#pragma unroll
          for (int j = 0; j < NQ; ++j) tb[hh][j] = tn[hh][j];
      }
    }
    fwht_wave<real, E>(v, lane, E >= 2 ? 64 : mlanes);
    if (a.mode == SC_AZ) {
      if (have) {
        real* ol = a.out + (size_t)b * LM + (size_t)l * M;
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = v[i] / a.sqrt_n;
        store_section<real, E>(ol, v, lane, M);
      }
      return;  // uniform: no barrier follows in this mode
    }
    if (have) {
      const real bb = denoise_section<real, E>(v, bprev, bl, lane, M, cl, tau2, a.sqrt_n, true, 0);
      if (lane == 0) bbw[wv] = bb;
    }
  }
  if (have) {
    fwht_wave<real, E>(v, lane, E >= 2 ? 64 : mlanes);  // T_l = H_M beta_l
  } else {
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = 0;  // absent section
    if (lane == 0) bbw[wv] = 0;
  }
  {
    real* tl = ts + wv * M;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int e = elem_index<E>(lane, i);
      if (e < M) tl[e] = v[i];
    }
  }
  __syncthreads();
  if (a.mode == SC_AMP && tid == 0) a.bbp[(size_t)b * a.G + g] = ((bbw[0] + bbw[1]) + bbw[2]) + bbw[3];
  real* abp = a.abp + ((size_t)b * a.G + g) * n;
  for (int r0 = 0; r0 < n; r0 += 256 * KR) {
    ushort4 fn[KR];
    const bool more = r0 + 256 * KR < n;
    if (more) {  // the next pass's entries in flight under this pass's LDS reads
#pragma unroll
      for (int u = 0; u < KR; ++u) {
        const int r = r0 + 256 * KR + u * 256 + tid;
        fn[u] = fw[r < n ? r : 0];
      }
    }
    real acc[KR];
#pragma unroll
    for (int u = 0; u < KR; ++u) {
      const real v0 = ts[0 * M + (f[u].x & 0x7fffu)];
      const real v1 = ts[1 * M + (f[u].y & 0x7fffu)];
      const real v2 = ts[2 * M + (f[u].z & 0x7fffu)];
      const real v3 = ts[3 * M + (f[u].w & 0x7fffu)];
      real t = (f[u].x & 0x8000u) ? -v0 : v0;
      t += (f[u].y & 0x8000u) ? -v1 : v1;
      t += (f[u].z & 0x8000u) ? -v2 : v2;
      t += (f[u].w & 0x8000u) ? -v3 : v3;
      acc[u] = t;
    }
#pragma unroll
    for (int u = 0; u < KR; ++u) {
      const int r = r0 + u * 256 + tid;
      if (r < n) st_part(&abp[r], acc[u]);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < KR; ++u) f[u] = fn[u];
    }
  }
}

// Row kernel: one wavefront = up to 64 rows of one row block r (z^2 partial
// q = blockIdx.x, lane = row) of one codeword (blockIdx.y).
//   (A beta)_i = sum_g sqrt(W[r, c(g)]) partial[g][i] / sqrt(n), in group order
//   (the groups of a column block with W[r, c] = 0 are skipped: they add 0);
//   psi_c = P_c - sum_{g in c} beta^2 partial[g] / n (lane c, in group order),
//   gamma_r = sum_c W[r, c] psi_c (in c order);
//   z_i <- y_i - (A beta)_i + (z_i / phi_r) gamma_r, phi_r the trace's row t.
// SCR_INIT: z = y and its z^2 partials, iters = -1.  SCR_ABOUT: out = A beta
// (+ noise, added in binary64: the encoder).
template <typename real>
__global__ void __launch_bounds__(64) k_scrow(ScRowArgs<real> a) {
  const int q = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int r = q / a.zpb, li = (q % a.zpb) * kScRowsPerBlk + lane;
  const bool valid = li < a.nr;
  const int i = r * a.nr + (valid ? li : 0);
  const size_t o = (size_t)b * a.n + i;
  real zn = 0;
  if (a.mode == SCR_INIT) {
    zn = valid ? a.y[o] : (real)0;
    if (valid) a.z[o] = zn;
    if (q == 0 && lane == 0) {
      a.iters[b] = -1;
      a.done[b] = 0;
    }
  } else {
    if (a.mode == SCR_AMP && a.iters[b] >= 0) {  // stopped (k_scsec of this or an earlier iteration): uniform
      if (q == 0 && lane == 0) a.done[b] = 1;
      return;
    }
    real acc = 0;
    const real* p = a.abp + (size_t)b * a.G * a.n + i;
    for (int c = 0; c < a.C; ++c) {
      const real wq = a.sqW[r * a.C + c];
      if (wq == (real)0) continue;  // uniform
      for (int j0 = 0; j0 < a.gpc; j0 += 4) {
        real t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u < a.gpc ? j0 + u : a.gpc - 1;
          t[u] = p[(size_t)(c * a.gpc + j) * a.n];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < a.gpc) acc += wq * t[u];
      }
    }
    const real ab = acc / a.sqrt_n;
    if (a.mode == SCR_ABOUT) {
      real x = ab;
      if (a.noise) x = (real)((double)ab + a.noise[o]);
      if (valid) a.out[o] = x;
      return;
    }
    real psi = 0;
    if (lane < a.C) {
      const real* bp = a.bbp + (size_t)b * a.G + (size_t)lane * a.gpc;
      real s = 0;
      for (int j = 0; j < a.gpc; ++j) s += bp[j];
      psi = a.Pc[lane] - s / (real)a.n;
    }
    real gam = 0;
    for (int c = 0; c < a.C; ++c) gam += a.W[r * a.C + c] * __shfl(psi, c);
    const real ph = a.phi[((size_t)b * a.T + a.t) * a.R + r];
    if (valid) {
      zn = a.y[o] - ab;
      zn += (a.z[o] / ph) * gam;
      a.z[o] = zn;
    }
  }
  const real s = wave_sum(zn * zn);
  if (lane == 0) a.zzp[(size_t)b * a.NZ + q] = s;
}

// The beta_0 start: z = y - A beta_0 with A beta_0 as
// sc_ab left it in ab [B][n], the z^2 partials, iters = -1 and done = 0.  The
// grid and indexing of k_scrow (one wavefront per z^2 partial and codeword) and
// its wave_sum, so the partials are formed in SCR_INIT's order; a kernel of its
// own, so that k_scrow compiles to what it compiled to.
template <typename real>
__global__ void __launch_bounds__(64) k_scstart(const real* __restrict__ y, const real* __restrict__ ab,
                                                real* __restrict__ z, real* __restrict__ zzp, int* __restrict__ iters,
                                                int* __restrict__ done, int n, int nr, int zpb, int NZ) {
  const int q = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int r = q / zpb, li = (q % zpb) * kScRowsPerBlk + lane;
  const bool valid = li < nr;
  const size_t o = (size_t)b * n + r * nr + (valid ? li : 0);
  real zn = 0;
  if (valid) {
    zn = y[o] - ab[o];
    z[o] = zn;
  }
  if (q == 0 && lane == 0) {
    iters[b] = -1;
    done[b] = 0;
  }
  const real s = wave_sum(zn * zn);
  if (lane == 0) zzp[(size_t)b * NZ + q] = s;
}

// Section decisions of the staged context (sa_sc_decide): argmax, first index on ties
template <typename real, int E>
__global__ void __launch_bounds__(256) k_sc_argmax(const real* beta, int32_t* dec, int L, int M) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (l >= L) return;
  const int bi = section_argmax<real, E>(beta + ((size_t)b * L + l) * M, lane, M, 0);
  if (lane == 0) dec[(size_t)b * L + l] = bi;
}

// one-hot beta(idx) with c_l at column idx[b][l] (beta zeroed in front)
template <typename real>
__global__ void k_sc_onehot(real* beta, const int32_t* idx, const real* c, int L, int M, int B) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B * L) return;
  const int l = k % L;
  beta[(size_t)k * M + idx[k]] = c[l];
}

// Section decisions (argmax, first index on ties), bit errors against idx
// (popcount of decision ^ index, summed per codeword: integer atomics), and
// iters = T for a codeword that never stopped.
template <typename real, int E>
__global__ void __launch_bounds__(256) k_sc_decide(const real* beta, const int32_t* idx, int32_t* dec, int32_t* errs,
                                                   int* iters, int L, int M, int T) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0 && iters[b] < 0) iters[b] = T;
  if (l >= L) return;
  const int bi = section_argmax<real, E>(beta + ((size_t)b * L + l) * M, lane, M, 0);
  if (lane == 0) {
    dec[(size_t)b * L + l] = bi;
    atomicAdd(&errs[b], __popc((unsigned)(bi ^ idx[(size_t)b * L + l])));
  }
}

template <typename S, typename D>
__global__ void k_sc_cvt(const S* s, D* d, size_t N) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x)
    d[i] = (D)s[i];
}

// ---- host side -----------------------------------------------------------------
static size_t sc_rsz(const sa_sc* s) { return s->lay.prec == SA_PREC_F64 ? 8 : 4; }

static int sc_alloc(void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(SA_ERR_NOMEM, "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
  }
  return SA_OK;
}

static int sc_blocks(size_t count) { return (int)std::min<size_t>(std::max<size_t>((count + 255) / 256, 1), 4096); }

int sc_stage(sa_sc* s, size_t count) {
  if (count <= s->stage_cap) return SA_OK;
  HIP_TRY(hipStreamSynchronize(s->stream));
  dev_free(s->d_stage);
  s->d_stage = nullptr;
  s->stage_cap = 0;
  if (int rc = sc_alloc((void**)&s->d_stage, count * sizeof(double))) return rc;
  s->stage_cap = count;
  return SA_OK;
}

// host binary64 -> a device buffer of the context precision, and back, on the context's stream
static int sc_upload(sa_sc* s, void* dst, const double* src, size_t count) {
  if (s->lay.prec == SA_PREC_F64) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * 8, hipMemcpyHostToDevice, s->stream));
    return SA_OK;
  }
  if (int rc = sc_stage(s, count)) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_stage, src, count * 8, hipMemcpyHostToDevice, s->stream));
  k_sc_cvt<double, float><<<sc_blocks(count), 256, 0, s->stream>>>(s->d_stage, (float*)dst, count);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

static int sc_download(sa_sc* s, double* dst, const void* src, size_t count) {
  if (s->lay.prec == SA_PREC_F64) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * 8, hipMemcpyDeviceToHost, s->stream));
    return SA_OK;
  }
  if (int rc = sc_stage(s, count)) return rc;
  k_sc_cvt<float, double><<<sc_blocks(count), 256, 0, s->stream>>>((const float*)src, s->d_stage, count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, s->d_stage, count * 8, hipMemcpyDeviceToHost, s->stream));
  return SA_OK;
}

static void sc_free_workspace(sa_sc* s) {
  dev_free(s->d_y); dev_free(s->d_z); dev_free(s->d_beta); dev_free(s->d_out);
  dev_free(s->d_abp); dev_free(s->d_bbp); dev_free(s->d_zzp); dev_free(s->d_phi);
  dev_free(s->d_iters); dev_free(s->d_done); dev_free(s->d_idx); dev_free(s->d_dec); dev_free(s->d_errs);
  dev_free(s->d_noise);
  s->d_y = s->d_z = s->d_beta = s->d_out = s->d_abp = s->d_bbp = s->d_zzp = s->d_phi = nullptr;
  s->d_iters = s->d_done = nullptr;
  s->d_idx = s->d_dec = s->d_errs = nullptr;
  s->d_noise = nullptr;
  s->Bcap = s->Tcap = 0;
  std::string none;
  sc_stage_rule(s->st, SC_CALL_RESIZE, 0, 0, none);  // nothing staged survives
  s->Trun = -1;
}

// buffers for B codewords and T iterations (grown, never shrunk)
static int sc_workspace(sa_sc* s, int B, int T) {
  if (B <= s->Bcap && T <= s->Tcap) return SA_OK;
  HIP_TRY(hipStreamSynchronize(s->stream));
  const int nB = std::max(B, s->Bcap), nT = std::max(std::max(T, s->Tcap), 1);
  sc_free_workspace(s);
  const ScLayout& y = s->lay;
  const size_t z = sc_rsz(s), LM = (size_t)y.L * y.M, n = (size_t)y.n;
  int rc = sc_alloc(&s->d_y, nB * n * z);
  if (!rc) rc = sc_alloc(&s->d_z, nB * n * z);
  if (!rc) rc = sc_alloc(&s->d_beta, nB * LM * z);
  if (!rc) rc = sc_alloc(&s->d_out, nB * std::max(LM, n) * z);
  if (!rc) rc = sc_alloc(&s->d_abp, (size_t)nB * y.G * n * z);
  if (!rc) rc = sc_alloc(&s->d_bbp, (size_t)nB * y.G * z);
  if (!rc) rc = sc_alloc(&s->d_zzp, (size_t)nB * y.NZ * z);
  if (!rc) rc = sc_alloc(&s->d_phi, (size_t)nB * nT * y.R * z);
  if (!rc) rc = sc_alloc((void**)&s->d_iters, (size_t)nB * sizeof(int));
  if (!rc) rc = sc_alloc((void**)&s->d_done, (size_t)nB * sizeof(int));
  if (!rc) rc = sc_alloc((void**)&s->d_idx, (size_t)nB * y.L * sizeof(int32_t));
  if (!rc) rc = sc_alloc((void**)&s->d_dec, (size_t)nB * y.L * sizeof(int32_t));
  if (!rc) rc = sc_alloc((void**)&s->d_errs, (size_t)nB * sizeof(int32_t));
  if (!rc) rc = sc_alloc((void**)&s->d_noise, nB * n * sizeof(double));
  if (rc) {
    sc_free_workspace(s);
    return rc;
  }
  s->Bcap = nB;
  s->Tcap = nT;
  return SA_OK;
}

static void sc_free_wave(sa_sc* s) {
  dev_free(s->d_taul); dev_free(s->d_live);
  s->d_taul = nullptr;
  s->d_live = nullptr;
  s->wBcap = s->wTcap = 0;
}

// the wave form's buffers for B codewords and T iterations (sa_sc.h: sc_wave_plan's bytes; grown, never shrunk)
static int sc_wave_workspace(sa_sc* s, int B, int T) {
  if (B <= s->wBcap && T <= s->wTcap) return SA_OK;
  HIP_TRY(hipStreamSynchronize(s->stream));
  const int nB = std::max(B, s->wBcap), nT = std::max(std::max(T, s->wTcap), 1);
  sc_free_wave(s);
  int rc = sc_alloc(&s->d_taul, sc_taul_bytes(s->lay, nB));
  if (!rc) rc = sc_alloc((void**)&s->d_live, sc_live_bytes(s->lay, nB, nT));
  if (rc) {
    sc_free_wave(s);
    return rc;
  }
  s->wBcap = nB;
  s->wTcap = nT;
  return SA_OK;
}

template <typename real>
static ScSecArgs<real> sc_sec_args(sa_sc* s, int mode, int T, int t, int es) {
  const ScLayout& y = s->lay;
  ScSecArgs<real> a;
  a.inv = s->parent->tab.inv;
  a.fwd = (const ushort4*)(y.own_fwd ? s->d_fwd : s->parent->tab.fwd);
  a.c = (const real*)s->d_c; a.W = (const real*)s->d_W; a.sqW = (const real*)s->d_sqW;
  a.z = (const real*)s->d_z; a.beta = (real*)s->d_beta; a.out = (real*)s->d_out;
  a.abp = (real*)s->d_abp; a.bbp = (real*)s->d_bbp; a.zzp = (const real*)s->d_zzp;
  a.phi = (real*)s->d_phi; a.iters = s->d_iters; a.done = s->d_done;
  a.L = y.L; a.M = y.M; a.n = y.n; a.w = y.w; a.nhi = y.nhi; a.G = y.G; a.gpc = y.gpc; a.Lc = y.L_c;
  a.R = y.R; a.C = y.C; a.nr = y.n_r; a.zpb = y.zpb; a.NZ = y.NZ; a.T = T; a.t = t; a.mode = mode;
  a.early_stop = es;
  a.sqrt_n = (real)std::sqrt((double)y.n);
  return a;
}

template <typename real>
static ScRowArgs<real> sc_row_args(sa_sc* s, int mode, int T, int t) {
  const ScLayout& y = s->lay;
  ScRowArgs<real> a;
  a.y = (const real*)s->d_y; a.z = (real*)s->d_z; a.abp = (const real*)s->d_abp; a.bbp = (const real*)s->d_bbp;
  a.W = (const real*)s->d_W; a.sqW = (const real*)s->d_sqW; a.Pc = (const real*)s->d_Pc;
  a.phi = (const real*)s->d_phi; a.zzp = (real*)s->d_zzp; a.out = (real*)s->d_out; a.noise = nullptr;
  a.iters = s->d_iters; a.done = s->d_done;
  a.n = y.n; a.G = y.G; a.gpc = y.gpc; a.R = y.R; a.C = y.C; a.nr = y.n_r; a.zpb = y.zpb; a.NZ = y.NZ;
  a.T = T; a.t = t; a.mode = mode;
  a.sqrt_n = (real)std::sqrt((double)y.n);
  return a;
}

template <typename real>
static int sc_launch_sec(sa_sc* s, int B, const ScSecArgs<real>& a) {
  const dim3 grid(s->lay.G, B);
  const size_t lds = s->lay.sec_lds;
  switch (s->lay.E) {
#define SA_SC_SEC(EE) case EE: k_scsec<real, EE><<<grid, 256, lds, s->stream>>>(a); break;
    SA_SC_SEC(1) SA_SC_SEC(2) SA_SC_SEC(4) SA_SC_SEC(8) SA_SC_SEC(16) SA_SC_SEC(32) SA_SC_SEC(64)
#undef SA_SC_SEC
    default: return fail(SA_ERR_UNSUPPORTED, "k_scsec: M");
  }
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

// the wave form's instances: the same grid, block and LDS image
template <typename real>
static int sc_launch_wave(sa_sc* s, int B, const ScWaveArgs<real>& a) {
  const dim3 grid(s->lay.G, B);
  const size_t lds = s->lay.sec_lds;
  switch (s->lay.E) {
#define SA_SC_SEC(EE) case EE: k_scsec<real, EE, ScWaveArgs<real>><<<grid, 256, lds, s->stream>>>(a); break;
    SA_SC_SEC(1) SA_SC_SEC(2) SA_SC_SEC(4) SA_SC_SEC(8) SA_SC_SEC(16) SA_SC_SEC(32) SA_SC_SEC(64)
#undef SA_SC_SEC
    default: return fail(SA_ERR_UNSUPPORTED, "k_scsec: M");
  }
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

template <typename real>
static int sc_launch_row(sa_sc* s, int B, const ScRowArgs<real>& a) {
  k_scrow<real><<<dim3(s->lay.NZ, B), 64, 0, s->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

// The decode of the y staged in d_y: z = y, then T times (k_scsec, k_scrow),
// launched eagerly on the context's stream with no host synchronisation
// between them (why no graph).  The launches are
// sc_decode_launches' (sa_sc.h), in its order: with beta0 the staged d_beta is
// the start and z = y - A beta_0 (section 13c).
// wv.wave (sc_wave_plan): k_scsec's wave form with the plan's tolerances, the
// live trace into d_live where wv.live_bytes asks for one (zeroed in front, as
// the phi trace); else exactly the launches of a decode without tolerances.
template <typename real>
static int sc_ab(sa_sc* s, int B, const double* d_noise, void* d_out);

template <typename real>
static int sc_launch_start(sa_sc* s, int B) {
  const ScLayout& y = s->lay;
  k_scstart<real><<<dim3(y.NZ, B), 64, 0, s->stream>>>((const real*)s->d_y, (const real*)s->d_out, (real*)s->d_z,
                                                       (real*)s->d_zzp, s->d_iters, s->d_done, y.n, y.n_r, y.zpb, y.NZ);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

template <typename real>
static int sc_decode(sa_sc* s, int B, int T, int es, const ScWavePlan& wv, bool beta0 = false) {
  const ScLayout& y = s->lay;
  for (const ScLaunch& l : sc_decode_launches(T, beta0, wv)) {
    int rc = SA_OK;
    switch (l.step) {
      case SCS_MEMSET_BETA:
        HIP_TRY(hipMemsetAsync(s->d_beta, 0, (size_t)B * y.L * y.M * sizeof(real), s->stream));
        break;
      case SCS_MEMSET_PHI:
        HIP_TRY(hipMemsetAsync(s->d_phi, 0, (size_t)B * std::max(T, 1) * y.R * sizeof(real), s->stream));
        break;
      case SCS_MEMSET_LIVE:
        HIP_TRY(hipMemsetAsync(s->d_live, 0, wv.live_bytes, s->stream));
        break;
      case SCS_ROW_INIT:
        rc = sc_launch_row<real>(s, B, sc_row_args<real>(s, SCR_INIT, T, 0));
        break;
      case SCS_SEC_AB:  // with SCS_ROW_ABOUT: A beta_0 into d_out
        rc = sc_launch_sec<real>(s, B, sc_sec_args<real>(s, SC_AB, 1, 0, 0));
        break;
      case SCS_ROW_ABOUT:
        rc = sc_launch_row<real>(s, B, sc_row_args<real>(s, SCR_ABOUT, 1, 0));
        break;
      case SCS_START:
        rc = sc_launch_start<real>(s, B);
        break;
      case SCS_SEC_AMP:
        rc = sc_launch_sec<real>(s, B, sc_sec_args<real>(s, SC_AMP, T, l.t, es));
        break;
      case SCS_SEC_WAVE: {
        ScWaveArgs<real> a;
        static_cast<ScSecArgs<real>&>(a) = sc_sec_args<real>(s, SC_AMP, T, l.t, es);
        a.stop_tol = (real)wv.stop_tol;
        a.freeze_tol = (real)wv.freeze_tol;
        a.taul = (real*)s->d_taul;
        a.live = wv.live_bytes ? s->d_live : nullptr;
        rc = sc_launch_wave<real>(s, B, a);
        break;
      }
      case SCS_ROW_AMP:
        rc = sc_launch_row<real>(s, B, sc_row_args<real>(s, SCR_AMP, T, l.t));
        break;
    }
    if (rc) return rc;
  }
  return SA_OK;
}

// A beta of d_beta -> d_out [B][n] (+ noise in binary64 where given: the encoder)
template <typename real>
static int sc_ab(sa_sc* s, int B, const double* d_noise, void* d_out) {
  if (int rc = sc_launch_sec<real>(s, B, sc_sec_args<real>(s, SC_AB, 1, 0, 0))) return rc;
  ScRowArgs<real> a = sc_row_args<real>(s, SCR_ABOUT, 1, 0);
  a.noise = d_noise;
  a.out = (real*)d_out;
  return sc_launch_row<real>(s, B, a);
}

template <typename real>
static hipError_t sc_lds_attrs_t() {
  const int mx = (int)kLdsBytes;
  hipError_t e = hipSuccess;
#define SA_A(F) if (e == hipSuccess) e = hipFuncSetAttribute((const void*)F, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
  SA_A((k_scsec<real, 1>)) SA_A((k_scsec<real, 2>)) SA_A((k_scsec<real, 4>)) SA_A((k_scsec<real, 8>))
  SA_A((k_scsec<real, 16>)) SA_A((k_scsec<real, 32>)) SA_A((k_scsec<real, 64>))
  SA_A((k_scsec<real, 1, ScWaveArgs<real>>)) SA_A((k_scsec<real, 2, ScWaveArgs<real>>))
  SA_A((k_scsec<real, 4, ScWaveArgs<real>>)) SA_A((k_scsec<real, 8, ScWaveArgs<real>>))
  SA_A((k_scsec<real, 16, ScWaveArgs<real>>)) SA_A((k_scsec<real, 32, ScWaveArgs<real>>))
  SA_A((k_scsec<real, 64, ScWaveArgs<real>>))
#undef SA_A
  return e;
}

// c_l = sqrt(n Pl_l) and P_c = sum of Pl over column block c, in binary64 on the host, then the context precision
// (and c_l once more as binary64, d_cd)
static int sc_set_power(sa_sc* s, const double* Pl) {
  const ScLayout& y = s->lay;
  std::vector<double> v((size_t)y.L + y.C, 0.0);
  for (int l = 0; l < y.L; ++l) {
    if (!(Pl[l] >= 0) || !std::isfinite(Pl[l])) return fail(SA_ERR_ARG, "Pl must be non-negative and finite");
    v[l] = std::sqrt((double)y.n * Pl[l]);
    v[(size_t)y.L + l / y.L_c] += Pl[l];
  }
  if (int rc = sc_upload(s, s->d_c, v.data(), y.L)) return rc;
  if (int rc = sc_upload(s, s->d_Pc, v.data() + y.L, y.C)) return rc;
  // the glue kernels of sa_glue.hip read c_l as binary64
  HIP_TRY(hipMemcpyAsync(s->d_cd, v.data(), (size_t)y.L * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));  // v is a host temporary
  std::string none;
  return sc_stage_rule(s->st, SC_CALL_STAGE_POWER, 0, 0, none);
}

// a one-call entry point overwrites the workspace: nothing staged survives it
static void sc_one_call(sa_sc* s) {
  std::string none;
  sc_stage_rule(s->st, SC_CALL_ONE_CALL, 0, 0, none);
}

static int sc_check(const sa_sc* s, int B, const char* what) {
  if (!s) return fail(SA_ERR_ARG, std::string(what) + ": null context");
  if (B < 1 || B > 65535) return fail(SA_ERR_ARG, std::string(what) + ": B must be in [1, 65535]");
  return SA_OK;
}

}  // namespace sa

using namespace sa;

extern "C" {

int sa_sc_create(sa_ctx* parent, int R, int C, const double* W, sa_sc** out) {
  if (!out) return fail(SA_ERR_ARG, "sa_sc_create: out is NULL");
  if (!parent) return fail(SA_ERR_ARG, "sa_sc_create: parent is NULL");
  if (parent->backend != SA_BACKEND_HADAMARD)
    return fail(SA_ERR_UNSUPPORTED, "sa_sc_create: parent must be a Hadamard-backend context");
  if (!parent->pow2 || parent->dead != 0)
    return fail(SA_ERR_UNSUPPORTED, "sa_sc_create: M must be a power of two for a coupled design");
  ScLayout lay;
  std::string err;
  if (int rc = sc_layout(lay, parent->L, parent->M, parent->n, parent->prec, R, C, W, err))
    return fail(rc, "sa_sc_create: " + err);
  if (parent->big || !parent->tab.inv || !parent->tab.fwd || parent->w != lay.w || parent->nhi != lay.nhi ||
      parent->E != lay.E)
    return fail(SA_ERR_UNSUPPORTED, "sa_sc_create: n too large: the parent operator keeps z out of the LDS");
  HIP_TRY(hipSetDevice(parent->device));
  {
    static int done = 0;
    if (!done) {
      hipError_t e = sc_lds_attrs_t<float>();
      if (e == hipSuccess) e = sc_lds_attrs_t<double>();
      if (e != hipSuccess) return fail(SA_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
      done = 1;
    }
  }
  sa_sc* s = new sa_sc();
  s->parent = parent;
  s->lay = lay;
  s->W.assign(W, W + (size_t)R * C);
  int rc = SA_OK;
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess)
    rc = fail(SA_ERR_HIP, "sa_sc_create: stream / event creation failed");
  const size_t z = sc_rsz(s), RC = (size_t)R * C;
  if (!rc) rc = sc_alloc(&s->d_W, RC * z);
  if (!rc) rc = sc_alloc(&s->d_sqW, RC * z);
  if (!rc) rc = sc_alloc(&s->d_c, (size_t)lay.L * z);
  if (!rc) rc = sc_alloc(&s->d_Pc, (size_t)C * z);
  if (!rc) rc = sc_alloc((void**)&s->d_cd, sc_cd_bytes(lay));
  std::vector<double> sq(RC);
  for (size_t k = 0; k < RC; ++k) sq[k] = std::sqrt(W[k]);
  if (!rc) rc = sc_upload(s, s->d_W, W, RC);
  if (!rc) rc = sc_upload(s, s->d_sqW, sq.data(), RC);
  std::vector<uint16_t> fwd;
  if (!rc && lay.own_fwd) {
    if (parent->ordering.size() != (size_t)lay.L * lay.n) {
      rc = fail(SA_ERR_UNSUPPORTED, "sa_sc_create: the parent holds no ordering");
    } else {
      fwd.resize((size_t)lay.G * lay.n * kSpw);
      sc_fwd_table(lay, parent->ordering.data(), fwd.data());
      rc = sc_alloc((void**)&s->d_fwd, fwd.size() * sizeof(uint16_t));
      if (!rc && hipMemcpyAsync(s->d_fwd, fwd.data(), fwd.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s->stream) !=
                     hipSuccess)
        rc = fail(SA_ERR_HIP, "sa_sc_create: table upload failed");
    }
  }
  if (!rc && hipStreamSynchronize(s->stream) != hipSuccess) rc = fail(SA_ERR_HIP, "sa_sc_create: upload failed");
  if (rc) {
    sa_sc_destroy(s);
    return rc;
  }
  *out = s;
  return SA_OK;
}

void sa_sc_destroy(sa_sc* s) {
  if (!s) return;
  (void)hipSetDevice(s->parent->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  sc_free_workspace(s);
  sc_free_wave(s);
  dev_free(s->d_W); dev_free(s->d_sqW); dev_free(s->d_fwd); dev_free(s->d_c); dev_free(s->d_Pc); dev_free(s->d_cd);
  dev_free(s->d_stage);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

int sa_sc_Ab(sa_sc* s, int B, const double* beta, double* out) {
  if (int rc = sc_check(s, B, "sa_sc_Ab")) return rc;
  if (!beta || !out) return fail(SA_ERR_ARG, "sa_sc_Ab: beta or out is NULL");
  HIP_TRY(hipSetDevice(s->parent->device));
  int rc = sc_workspace(s, B, 1);
  if (rc) return rc;
  sc_one_call(s);
  const ScLayout& y = s->lay;
  if ((rc = sc_upload(s, s->d_beta, beta, (size_t)B * y.L * y.M))) return rc;
  rc = y.prec == SA_PREC_F64 ? sc_ab<double>(s, B, nullptr, s->d_out) : sc_ab<float>(s, B, nullptr, s->d_out);
  if (rc) return rc;
  if ((rc = sc_download(s, out, s->d_out, (size_t)B * y.n))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

int sa_sc_Az(sa_sc* s, int B, const double* z, double* out) {
  if (int rc = sc_check(s, B, "sa_sc_Az")) return rc;
  if (!z || !out) return fail(SA_ERR_ARG, "sa_sc_Az: z or out is NULL");
  HIP_TRY(hipSetDevice(s->parent->device));
  int rc = sc_workspace(s, B, 1);
  if (rc) return rc;
  sc_one_call(s);
  const ScLayout& y = s->lay;
  if ((rc = sc_upload(s, s->d_z, z, (size_t)B * y.n))) return rc;
  rc = y.prec == SA_PREC_F64 ? sc_launch_sec<double>(s, B, sc_sec_args<double>(s, SC_AZ, 1, 0, 0))
                             : sc_launch_sec<float>(s, B, sc_sec_args<float>(s, SC_AZ, 1, 0, 0));
  if (rc) return rc;
  if ((rc = sc_download(s, out, s->d_out, (size_t)B * y.L * y.M))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

// The live trace of a decode without tolerances: every block of every iteration in front of the stop index
static void sc_live_all(const ScLayout& y, int B, int T, const int* iters, unsigned char* live_out) {
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      std::memset(live_out + sc_live_index(y, T, b, t, 0), t < iters[b] ? 1 : 0, (size_t)y.C);
}

static int sc_amp_impl(const char* what, sa_sc* s, int B, const double* yv, const double* Pl, int T, double stop_tol,
                       double freeze_tol, double* beta_out, int* iters_out, double* phi_out, unsigned char* live_out,
                       int flags, const double* beta0 = nullptr) {
  const std::string w = std::string(what) + ": ";
  if (int rc = sc_check(s, B, what)) return rc;
  if (!yv) return fail(SA_ERR_ARG, w + "y is NULL");
  if (!Pl) return fail(SA_ERR_ARG, w + "Pl is NULL");
  if (!beta_out) return fail(SA_ERR_ARG, w + "beta_out is NULL");
  if (T < 0) return fail(SA_ERR_ARG, w + "T must be non-negative");
  if (flags & ~SA_FLAG_NO_EARLY_STOP) return fail(SA_ERR_ARG, w + "unknown flags");
  const ScLayout& y = s->lay;
  ScWavePlan wv;
  std::string err;
  if (int rc = sc_wave_plan(wv, y, B, T, stop_tol, freeze_tol, live_out != nullptr, err)) return fail(rc, w + err);
  HIP_TRY(hipSetDevice(s->parent->device));
  for (int l = 0; l < y.L; ++l)
    if (!(Pl[l] >= 0) || !std::isfinite(Pl[l])) return fail(SA_ERR_ARG, w + "Pl must be non-negative and finite");
  int rc = sc_workspace(s, B, T);
  if (rc) return rc;
  sc_one_call(s);
  if (wv.wave && (rc = sc_wave_workspace(s, B, T))) return rc;
  if ((rc = sc_set_power(s, Pl))) return rc;
  if ((rc = sc_upload(s, s->d_y, yv, (size_t)B * y.n))) return rc;
  if (beta0 && (rc = sc_upload(s, s->d_beta, beta0, (size_t)B * y.L * y.M))) return rc;
  const int es = (flags & SA_FLAG_NO_EARLY_STOP) ? 0 : 1;
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  rc = y.prec == SA_PREC_F64 ? sc_decode<double>(s, B, T, es, wv, beta0 != nullptr)
                             : sc_decode<float>(s, B, T, es, wv, beta0 != nullptr);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  s->timed = true;
  if ((rc = sc_download(s, beta_out, s->d_beta, (size_t)B * y.L * y.M))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (phi_out && T > 0) {
    if ((rc = sc_download(s, phi_out, s->d_phi, (size_t)B * T * y.R))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  std::vector<int> own;
  int* iters = iters_out;
  if (!iters && live_out && !wv.wave) {
    own.resize(B);
    iters = own.data();
  }
  if (iters) {
    HIP_TRY(hipMemcpyAsync(iters, s->d_iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int b = 0; b < B; ++b)
      if (iters[b] < 0) iters[b] = T;
  }
  if (live_out && T > 0) {
    if (wv.wave) {
      HIP_TRY(hipMemcpyAsync(live_out, s->d_live, (size_t)B * T * y.C, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
    } else {
      sc_live_all(y, B, T, iters, live_out);
    }
  }
  return SA_OK;
}

int sa_sc_amp(sa_sc* s, int B, const double* yv, const double* Pl, int T, double* beta_out, int* iters_out,
              double* phi_out, int flags) {
  return sc_amp_impl("sa_sc_amp", s, B, yv, Pl, T, 0.0, 0.0, beta_out, iters_out, phi_out, nullptr, flags);
}

int sa_sc_amp_ex(sa_sc* s, int B, const double* yv, const double* Pl, int T, double stop_tol, double freeze_tol,
                 double* beta_out, int* iters_out, double* phi_out, unsigned char* live_out, int flags) {
  return sc_amp_impl("sa_sc_amp_ex", s, B, yv, Pl, T, stop_tol, freeze_tol, beta_out, iters_out, phi_out, live_out, flags);
}

int sa_sc_amp_start(sa_sc* s, int B, const double* yv, const double* Pl, int T, const double* beta0, double stop_tol,
                    double freeze_tol, double* beta_out, int* iters_out, double* phi_out, unsigned char* live_out,
                    int flags) {
  return sc_amp_impl("sa_sc_amp_start", s, B, yv, Pl, T, stop_tol, freeze_tol, beta_out, iters_out, phi_out, live_out,
                     flags, beta0);
}

double sa_sc_event_ms(sa_sc* s) {
  if (!s || !s->timed) return -1.0;
  float ms = 0;
  if (hipEventSynchronize(s->ev1) != hipSuccess || hipEventElapsedTime(&ms, s->ev0, s->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

static int sc_mc_impl(const char* what, sa_sc* s, int B, const int32_t* idx, const double* noise, const double* Pl, int T,
                      double stop_tol, double freeze_tol, int flags, int32_t* dec_out, int32_t* iters_out,
                      int32_t* errs_out, unsigned char* live_out, double* ms_out) {
  const std::string w = std::string(what) + ": ";
  if (int rc = sc_check(s, B, what)) return rc;
  if (!idx) return fail(SA_ERR_ARG, w + "idx is NULL");
  if (!Pl) return fail(SA_ERR_ARG, w + "Pl is NULL");
  if (T < 0) return fail(SA_ERR_ARG, w + "T must be non-negative");
  if (flags & ~SA_FLAG_NO_EARLY_STOP) return fail(SA_ERR_ARG, w + "unknown flags");
  const ScLayout& y = s->lay;
  ScWavePlan wv;
  std::string err;
  if (int rc = sc_wave_plan(wv, y, B, T, stop_tol, freeze_tol, live_out != nullptr, err)) return fail(rc, w + err);
  for (size_t k = 0; k < (size_t)B * y.L; ++k)
    if (idx[k] < 0 || idx[k] >= y.M) return fail(SA_ERR_ARG, w + "idx outside [0, M)");
  for (int l = 0; l < y.L; ++l)
    if (!(Pl[l] >= 0) || !std::isfinite(Pl[l])) return fail(SA_ERR_ARG, w + "Pl must be non-negative and finite");
  HIP_TRY(hipSetDevice(s->parent->device));
  int rc = sc_workspace(s, B, T);
  if (rc) return rc;
  sc_one_call(s);
  if (wv.wave && (rc = sc_wave_workspace(s, B, T))) return rc;
  if ((rc = sc_set_power(s, Pl))) return rc;
  const size_t z = sc_rsz(s), LM = (size_t)y.L * y.M;
  HIP_TRY(hipMemcpyAsync(s->d_idx, idx, (size_t)B * y.L * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  if (noise) HIP_TRY(hipMemcpyAsync(s->d_noise, noise, (size_t)B * y.n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  s->timed = false;
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  // encoder: y = A beta(idx) + noise, by the kernels of sa_sc_Ab
  HIP_TRY(hipMemsetAsync(s->d_beta, 0, (size_t)B * LM * z, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_errs, 0, (size_t)B * sizeof(int32_t), s->stream));
  const int es = (flags & SA_FLAG_NO_EARLY_STOP) ? 0 : 1;
  const int nb = (B * y.L + 255) / 256;
  const dim3 dgrid((y.L + 3) / 4, B);
  if (y.prec == SA_PREC_F64) {
    k_sc_onehot<double><<<nb, 256, 0, s->stream>>>((double*)s->d_beta, s->d_idx, (const double*)s->d_c, y.L, y.M, B);
    rc = sc_ab<double>(s, B, noise ? s->d_noise : nullptr, s->d_y);
    if (!rc) rc = sc_decode<double>(s, B, T, es, wv);
  } else {
    k_sc_onehot<float><<<nb, 256, 0, s->stream>>>((float*)s->d_beta, s->d_idx, (const float*)s->d_c, y.L, y.M, B);
    rc = sc_ab<float>(s, B, noise ? s->d_noise : nullptr, s->d_y);
    if (!rc) rc = sc_decode<float>(s, B, T, es, wv);
  }
  if (rc) return rc;
#define SA_SC_DEC(EE)                                                                                                  \
  case EE:                                                                                                             \
    if (y.prec == SA_PREC_F64)                                                                                         \
      k_sc_decide<double, EE><<<dgrid, 256, 0, s->stream>>>((const double*)s->d_beta, s->d_idx, s->d_dec, s->d_errs,   \
                                                             s->d_iters, y.L, y.M, T);                                 \
    else                                                                                                               \
      k_sc_decide<float, EE><<<dgrid, 256, 0, s->stream>>>((const float*)s->d_beta, s->d_idx, s->d_dec, s->d_errs,     \
                                                            s->d_iters, y.L, y.M, T);                                  \
    break;
  switch (y.E) { SA_SC_DEC(1) SA_SC_DEC(2) SA_SC_DEC(4) SA_SC_DEC(8) SA_SC_DEC(16) SA_SC_DEC(32) SA_SC_DEC(64) }
#undef SA_SC_DEC
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  if (dec_out) HIP_TRY(hipMemcpyAsync(dec_out, s->d_dec, (size_t)B * y.L * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  if (iters_out) HIP_TRY(hipMemcpyAsync(iters_out, s->d_iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  if (errs_out) HIP_TRY(hipMemcpyAsync(errs_out, s->d_errs, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  std::vector<int32_t> own;
  if (live_out && T > 0) {
    if (wv.wave) {
      HIP_TRY(hipMemcpyAsync(live_out, s->d_live, (size_t)B * T * y.C, hipMemcpyDeviceToHost, s->stream));
    } else if (!iters_out) {
      own.resize(B);
      HIP_TRY(hipMemcpyAsync(own.data(), s->d_iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (live_out && T > 0 && !wv.wave) sc_live_all(y, B, T, iters_out ? iters_out : own.data(), live_out);
  if (ms_out) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    *ms_out = (double)ms;
  }
  return SA_OK;
}

int sa_sc_mc(sa_sc* s, int B, const int32_t* idx, const double* noise, const double* Pl, int T, int flags,
             int32_t* dec_out, int32_t* iters_out, int32_t* errs_out, double* ms_out) {
  return sc_mc_impl("sa_sc_mc", s, B, idx, noise, Pl, T, 0.0, 0.0, flags, dec_out, iters_out, errs_out, nullptr, ms_out);
}

int sa_sc_mc_ex(sa_sc* s, int B, const int32_t* idx, const double* noise, const double* Pl, int T, double stop_tol,
                double freeze_tol, int flags, int32_t* dec_out, int32_t* iters_out, int32_t* errs_out,
                unsigned char* live_out, double* ms_out) {
  return sc_mc_impl("sa_sc_mc_ex", s, B, idx, noise, Pl, T, stop_tol, freeze_tol, flags, dec_out, iters_out, errs_out,
                    live_out, ms_out);
}

// ---- the staged, device-resident life cycle ----
// sc_stage_rule on the context: the checks alone (commit = false, in front of the work) or with the state it leaves
static int sc_rule(sa_sc* s, int call, int B, const char* what, bool commit = true) {
  if (!s) return fail(SA_ERR_ARG, std::string(what) + ": null context");
  std::string err;
  ScStageState probe = s->st;
  if (int rc = sc_stage_rule(commit ? s->st : probe, call, B, s->Bcap, err)) return fail(rc, std::string(what) + ": " + err);
  return SA_OK;
}

int sa_sc_reserve(sa_sc* s, int B, int T) {
  if (int rc = sc_check(s, B, "sa_sc_reserve")) return rc;
  if (T < 0) return fail(SA_ERR_ARG, "sa_sc_reserve: T must be non-negative");
  HIP_TRY(hipSetDevice(s->parent->device));
  return sc_workspace(s, B, T);
}

int sa_sc_stage_power(sa_sc* s, const double* Pl) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_stage_power: null context");
  if (!Pl) return fail(SA_ERR_ARG, "sa_sc_stage_power: Pl is NULL");
  HIP_TRY(hipSetDevice(s->parent->device));
  return sc_set_power(s, Pl);
}

int sa_sc_stage(sa_sc* s, int B, const double* yv, const double* beta0) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_stage: null context");
  if (!yv) return fail(SA_ERR_ARG, "sa_sc_stage: y is NULL");
  if (int rc = sc_rule(s, beta0 ? SC_CALL_STAGE_BETA0 : SC_CALL_STAGE, B, "sa_sc_stage", false)) return rc;
  HIP_TRY(hipSetDevice(s->parent->device));
  const ScLayout& y = s->lay;
  int rc = sc_upload(s, s->d_y, yv, (size_t)B * y.n);
  if (rc) return rc;
  if (beta0 && (rc = sc_upload(s, s->d_beta, beta0, (size_t)B * y.L * y.M))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return sc_rule(s, beta0 ? SC_CALL_STAGE_BETA0 : SC_CALL_STAGE, B, "sa_sc_stage");
}

// y = A beta(d_idx) + d_noise (NULL: none) of B codewords into d_y, by the kernels of sa_sc_Ab (as sa_sc_mc encodes)
static int sc_encode_staged(sa_sc* s, int B, const double* d_noise, int32_t* idx_out) {
  const ScLayout& y = s->lay;
  const int nb = (B * y.L + 255) / 256;
  HIP_TRY(hipMemsetAsync(s->d_beta, 0, (size_t)B * y.L * y.M * sc_rsz(s), s->stream));
  int rc;
  if (y.prec == SA_PREC_F64) {
    k_sc_onehot<double><<<nb, 256, 0, s->stream>>>((double*)s->d_beta, s->d_idx, (const double*)s->d_c, y.L, y.M, B);
    rc = sc_ab<double>(s, B, d_noise, s->d_y);
  } else {
    k_sc_onehot<float><<<nb, 256, 0, s->stream>>>((float*)s->d_beta, s->d_idx, (const float*)s->d_c, y.L, y.M, B);
    rc = sc_ab<float>(s, B, d_noise, s->d_y);
  }
  if (rc) return rc;
  if (idx_out)
    HIP_TRY(hipMemcpyAsync(idx_out, s->d_idx, (size_t)B * y.L * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return sc_rule(s, SC_CALL_ENCODE, B, "sa_sc_encode");
}

int sa_sc_encode(sa_sc* s, int B, const int32_t* idx, const double* noise) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_encode: null context");
  if (!idx) return fail(SA_ERR_ARG, "sa_sc_encode: idx is NULL");
  if (int rc = sc_rule(s, SC_CALL_ENCODE, B, "sa_sc_encode", false)) return rc;
  const ScLayout& y = s->lay;
  for (size_t k = 0; k < (size_t)B * y.L; ++k)
    if (idx[k] < 0 || idx[k] >= y.M) return fail(SA_ERR_ARG, "sa_sc_encode: idx outside [0, M)");
  HIP_TRY(hipSetDevice(s->parent->device));
  s->st.y = s->st.beta = false;  // d_y and d_beta are being rewritten
  HIP_TRY(hipMemcpyAsync(s->d_idx, idx, (size_t)B * y.L * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  if (noise) HIP_TRY(hipMemcpyAsync(s->d_noise, noise, (size_t)B * y.n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return sc_encode_staged(s, B, noise ? s->d_noise : nullptr, nullptr);
}

int sa_sc_encode_bits(sa_sc* s, int B, const uint8_t* d_bits, const double* d_noise, int32_t* idx_out) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_encode_bits: null context");
  if (!d_bits) return fail(SA_ERR_ARG, "sa_sc_encode_bits: bits is NULL");
  if (int rc = sc_rule(s, SC_CALL_ENCODE, B, "sa_sc_encode_bits", false)) return rc;
  const ScLayout& y = s->lay;
  if (y.M < 2) return fail(SA_ERR_UNSUPPORTED, "sa_sc_encode_bits: M < 2 carries no bits");
  HIP_TRY(hipSetDevice(s->parent->device));
  s->st.y = s->st.beta = false;
  if (int rc = launch_bits_idx(s->stream, d_bits, ilog2(y.M), y.L, B, s->d_idx)) return rc;
  return sc_encode_staged(s, B, d_noise, idx_out);
}

int sa_sc_run(sa_sc* s, int B, int T, double stop_tol, double freeze_tol, int flags) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_run: null context");
  if (flags & ~(SA_FLAG_NO_EARLY_STOP | SA_FLAG_BETA0)) return fail(SA_ERR_ARG, "sa_sc_run: unknown flags");
  if (T < 0 || T > std::max(s->Tcap, 0)) return fail(SA_ERR_ARG, "sa_sc_run: T outside the reserved workspace (sa_sc_reserve)");
  const bool b0 = (flags & SA_FLAG_BETA0) != 0;
  if (int rc = sc_rule(s, b0 ? SC_CALL_RUN_BETA0 : SC_CALL_RUN, B, "sa_sc_run", false)) return rc;
  const ScLayout& y = s->lay;
  ScWavePlan wv;
  std::string err;
  int rc = sc_wave_plan(wv, y, B, T, stop_tol, freeze_tol, false, err);
  if (rc) return fail(rc, "sa_sc_run: " + err);
  sc_rule(s, b0 ? SC_CALL_RUN_BETA0 : SC_CALL_RUN, B, "sa_sc_run");
  HIP_TRY(hipSetDevice(s->parent->device));
  if (wv.wave && (rc = sc_wave_workspace(s, B, T))) return rc;
  const int es = (flags & SA_FLAG_NO_EARLY_STOP) ? 0 : 1;
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  rc = y.prec == SA_PREC_F64 ? sc_decode<double>(s, B, T, es, wv, b0) : sc_decode<float>(s, B, T, es, wv, b0);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  s->timed = true;
  s->Trun = T;
  return SA_OK;
}

int sa_sc_wait(sa_sc* s) {
  if (!s) return fail(SA_ERR_ARG, "sa_sc_wait: null context");
  HIP_TRY(hipSetDevice(s->parent->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

int sa_sc_fetch(sa_sc* s, int B, double* beta_out, int* iters_out, double* phi_out) {
  if (int rc = sc_rule(s, SC_CALL_FETCH, B, "sa_sc_fetch")) return rc;
  if ((iters_out || phi_out) && s->Trun < 0) return fail(SA_ERR_ARG, "sa_sc_fetch: no run to read the stop indices of");
  HIP_TRY(hipSetDevice(s->parent->device));
  const ScLayout& y = s->lay;
  int rc;
  if (beta_out) {
    if ((rc = sc_download(s, beta_out, s->d_beta, (size_t)B * y.L * y.M))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  if (phi_out && s->Trun > 0) {
    if ((rc = sc_download(s, phi_out, s->d_phi, (size_t)B * s->Trun * y.R))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  if (iters_out) {
    HIP_TRY(hipMemcpyAsync(iters_out, s->d_iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int b = 0; b < B; ++b)
      if (iters_out[b] < 0) iters_out[b] = s->Trun;
  }
  return SA_OK;
}

int sa_sc_decide(sa_sc* s, int B, int32_t* idx_out) {
  if (int rc = sc_rule(s, SC_CALL_FETCH, B, "sa_sc_decide")) return rc;
  if (!idx_out) return fail(SA_ERR_ARG, "sa_sc_decide: idx_out is NULL");
  HIP_TRY(hipSetDevice(s->parent->device));
  const ScLayout& y = s->lay;
  const dim3 dgrid((y.L + 3) / 4, B);
#define SA_SC_ARG(EE)                                                                                              \
  case EE:                                                                                                         \
    if (y.prec == SA_PREC_F64)                                                                                     \
      k_sc_argmax<double, EE><<<dgrid, 256, 0, s->stream>>>((const double*)s->d_beta, s->d_dec, y.L, y.M);         \
    else                                                                                                           \
      k_sc_argmax<float, EE><<<dgrid, 256, 0, s->stream>>>((const float*)s->d_beta, s->d_dec, y.L, y.M);           \
    break;
  switch (y.E) { SA_SC_ARG(1) SA_SC_ARG(2) SA_SC_ARG(4) SA_SC_ARG(8) SA_SC_ARG(16) SA_SC_ARG(32) SA_SC_ARG(64) }
#undef SA_SC_ARG
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(idx_out, s->d_dec, (size_t)B * y.L * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SA_OK;
}

}  // extern "C"
