// sa_row2.hip — the small-batch row kernel k_row2 and its launcher, in a
// translation unit of their own: the unit csrc/Makefile builds with kernarg
// preload, which every kernel with plain leading parameters in a unit gets.
#include "sa_host.h"

namespace sa {

// Row kernel for small batches: 32 rows per 512-thread workgroup, so the
// ceil(n/32) workgroups of a codeword spread over twice as many CUs as
// k_row's 64-row workgroups.  Thread (row rl, group pg) sums the Ab
// partials g = pg, pg+16, ... of its row in order
// (all loads of a thread in flight together); the 16 group sums are added in
// group order; wave 0 finishes the rows (Onsager residual, z^2 partial).
// R = 16 (row-block-major partials only, where the line holds two partials of
// the same block): twice the workgroups, NG = 32 partial groups of G / 32.
//
// One vector memory trip per launch and no scalar one in front of it: the
// arguments are a head of 14 dwords of plain parameters, which arrive in
// SGPRs with the wave (kernarg preload, csrc/Makefile), and a tail struct.
// Every load of the first trip (tau_t, tau_{t-1}, y, z, the codeword's power,
// the beta^2 partials, the Ab partials) forms its address from the head and
// the block / thread indices alone; the tail (what wave 0 needs behind the
// barrier) is loaded while that trip is in flight.  What makes 14 dwords do:
//   taut   tau + t, folded on the host (tpos: t > 0, tau_{t-1} exists)
//   z      the residual, read (the previous one) and written in place
//   gg     G | Gb << 16
//   flt    T1 | flags << 24 (kRow2Mode ..., sa_common.h)
//   bbo    byte offset of the beta^2 partials from taut (one allocation, lane_alloc)
// and the row-block count is ceil(n / R) (launch_row2 checks the plan's), no
// argument and no hidden grid size.  Everything wave 0 needs behind the
// barrier (y, z, the beta^2 partials, the codeword's power) is loaded with
// the Ab partials in front of it.
template <typename real, int R = kRow2Rows, int NT = 512>
__global__ void __launch_bounds__(NT) k_row2(const real* __restrict__ abp_p, const real* __restrict__ y_p,
                                             real* z_p, const real* __restrict__ taut_p,
                                             const real* __restrict__ Pb_p, int n, unsigned gg, unsigned flt,
                                             unsigned bbo, Row2Tail<real> tl) {
  constexpr int NG = NT / R;  // partial groups
  __shared__ real red[NG][R + 1];
  const real* zin_p = z_p;
  const real* bbp_p = reinterpret_cast<const real*>(reinterpret_cast<const char*>(taut_p) + bbo);
  const int G = (int)(gg & 0xffffu), Gb = (int)(gg >> 16), NZ = (n + R - 1) / R;
  const int T1 = (int)(flt & 0xffffffu);
  const unsigned fl = flt >> 24;
  const int mode = (int)(fl & kRow2Mode), pt = (int)(fl & kRow2Pt), es = (int)(fl & kRow2Es);
  const int Pbst = (fl & kRow2Pbst) ? 1 : 0;
  const bool tpos = (fl & kRow2Tpos) != 0;
  // the tail, wanted in SGPRs behind the issue of the first trip's loads
  // (tail_now there): its one batch of scalar loads rides under that trip,
  // and nothing in front of a vector load waits for it
  real* zzp_p = tl.zzp;
  real* out_p = tl.out;
  int* iters_p = tl.iters;
  const real sqrt_n = tl.sqrt_n;
  const int itset = tl.itset;
  auto tail_now = [&] { sgpr_now(zzp_p, out_p, iters_p, sqrt_n, itset); };
  const int b = blockIdx.y, tid = threadIdx.x;
  const int rl = tid & (R - 1), pg = tid / R;
  const int r = blockIdx.x * R + rl;
  // tau_t and tau_{t-1} are loaded with everything else; the early-stop
  // test waits for them only after the Ab-partial loads are in flight
  // (testing first cost a whole memory round trip per launch)
  real tau = 1, last = 0;
  if (mode == ROW_AMP) {
    tau = ld_vmem(taut_p + (size_t)b * T1);
    last = tpos ? ld_vmem(taut_p + (size_t)b * T1 - 1) : (real)0;
  }
  const size_t o = (size_t)b * n + (r < n ? r : 0);
  real yv = 0, zv = 0, Pv = 0, bbv[4] = {0, 0, 0, 0};
  if (tid < 64) {
    yv = y_p[o];
    if (mode == ROW_AMP) {
      zv = zin_p[o];
      // the codeword's power: constant over the decode, but behind the barrier
      // its load was a second memory round trip of every launch
      Pv = ld_vmem(Pb_p + (size_t)b * Pbst);
      const real* bp = bbp_p + (size_t)b * Gb;
#pragma unroll
      for (int q = 0; q < 4; ++q) bbv[q] = tid + 64 * q < Gb ? bp[tid + 64 * q] : (real)0;
    }
  }
  if (mode != ROW_INIT0) {
    // pt: partial g of row r at [b][r / R][g][r % R] (n padded to R rows)
    const size_t gs = pt ? (size_t)R : (size_t)n;
    const real* p = pt ? abp_p + (size_t)b * G * ((size_t)NZ * R) + (size_t)blockIdx.x * G * R + rl
                       : abp_p + (size_t)b * G * n + (r < n ? r : 0);
    real acc = 0;
    constexpr int U = 256 / NG;  // G = 256 (C2, C4): every load of a thread in one pass
    if (pt && (R == 16 || sizeof(real) == 4) && G == NG * U) {
      // row-block-major partials with exactly NG x U partials (32-row blocks:
      // binary32 only, C4 single codeword +1 %; the binary64 32-row blocks
      // measured 1.4 % slower in this form).  The [G][n] partials of k_sec
      // (sa_Ab, the beta0 start) take the general loop even in 16-row blocks:
      // constant strides from the block base, no bounds, 32-bit offsets (the
      // general form spent ~40 VALU ops of 64-bit address math before the
      // first load); the same loads and sums in the same order
      const real* pb = abp_p + (size_t)b * G * ((size_t)NZ * R) + (size_t)blockIdx.x * G * R;
      real tt[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        tt[u] = ld_off(pb, (unsigned)(((pg + NG * u) * R + rl) * (int)sizeof(real)));
      tail_now();
#pragma unroll
      for (int u = 0; u < U; ++u) acc += tt[u];
    } else if (pt && (R == 16 || sizeof(real) == 4) && G == NG * (U / 2)) {
      // the same with G = 128 (c2 on k_sec44): half the loads per thread
      constexpr int UH = U / 2;
      const real* pb = abp_p + (size_t)b * G * ((size_t)NZ * R) + (size_t)blockIdx.x * G * R;
      real tt[UH];
#pragma unroll
      for (int u = 0; u < UH; ++u)
        tt[u] = ld_off(pb, (unsigned)(((pg + NG * u) * R + rl) * (int)sizeof(real)));
      tail_now();
#pragma unroll
      for (int u = 0; u < UH; ++u) acc += tt[u];
    } else
    for (int g0 = pg; g0 < G; g0 += NG * U) {
      real tt[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + NG * u;
        tt[u] = p[(size_t)(g < G ? g : pg) * gs];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (g0 + NG * u < G) acc += tt[u];
    }
    red[pg][rl] = acc;
  }
  tail_now();
  if (mode == ROW_AMP && es && tau == last) return;  // uniform over the workgroup
  const real tau2 = tau * tau;
  __syncthreads();
  if (tid >= 64) return;
  // the decode's iters[b]: -1 with the residual's initialisation; T with the
  // last iteration, which runs to here only when no stop has fired (a stopped
  // codeword stops every later launch too, and keeps the index it stopped at)
  if (itset != 0 && blockIdx.x == 0 && tid == 0) iters_p[b] = itset;
  real ons = 0;
  if (mode == ROW_AMP) {
    real bb;
    if (Gb <= 256) {
      real sacc = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) sacc += bbv[q];
      bb = wave_sum(sacc);
    } else {
      bb = wave_sum_parts(bbp_p + (size_t)b * Gb, Gb);
    }
    ons = Pv - bb / (real)n;
  }
  real zn = 0;
  if (tid < R && r < n) {
    if (mode == ROW_INIT0) {
      zn = yv;
    } else {
      real acc = 0;
#pragma unroll
      for (int q = 0; q < NG; ++q) acc += red[q][rl];
      const real ab = acc / sqrt_n;
      if (mode == ROW_ABOUT) {
        out_p[o] = ab;
        return;
      }
      zn = yv - ab;
      if (mode == ROW_AMP) zn += (zv / tau2) * ons;
    }
    z_p[o] = zn;
  }
  if (mode == ROW_ABOUT) return;
  const real sz = wave_sum(zn * zn);
  if (tid == 0) zzp_p[(size_t)b * NZ + blockIdx.x] = sz;
}

// k_row2's head and tail out of the host-side description (RowArgs)
template <typename real, int R>
int launch_row2(sa_ctx* c, const Plan& p, int B, const RowArgs<real>& a) {
  if (p.nz != (a.n + R - 1) / R) return fail(SA_ERR_UNSUPPORTED, "k_row2: row blocks of the plan");
  if (a.z_in != a.z) return fail(SA_ERR_UNSUPPORTED, "k_row2: the residual is updated in place");
  if (a.G > 0xffff || a.Gb > 0xffff || a.T1 >= (1 << 24)) return fail(SA_ERR_UNSUPPORTED, "k_row2: G, Gb, T1");
  const real* taut = a.tau + a.t;
  const std::ptrdiff_t bbo = reinterpret_cast<const char*>(a.bbp) - reinterpret_cast<const char*>(taut);
  if (bbo < 0 || bbo > (std::ptrdiff_t)0xffffffffu) return fail(SA_ERR_UNSUPPORTED, "k_row2: beta^2 partials not behind tau");
  const unsigned fl = (unsigned)(a.mode & kRow2Mode) | (a.pt ? kRow2Pt : 0u) | (a.early_stop ? kRow2Es : 0u) |
                      (a.t > 0 ? kRow2Tpos : 0u) | (a.Pbst ? kRow2Pbst : 0u);
  Row2Tail<real> tl;
  tl.zzp = a.zzp; tl.out = a.out; tl.iters = a.iters; tl.sqrt_n = a.sqrt_n; tl.itset = a.itset;
  plaunch(c, k_row2<real, R>, dim3(p.nz, B), 512, 0, a.abp, a.y, a.z, taut, a.Pb, a.n,
          (unsigned)a.G | (unsigned)a.Gb << 16, (unsigned)a.T1 | fl << 24, (unsigned)bbo, tl);
  return SA_OK;
}

template int launch_row2<float, kRow2Rows>(sa_ctx*, const Plan&, int, const RowArgs<float>&);
template int launch_row2<float, 16>(sa_ctx*, const Plan&, int, const RowArgs<float>&);
template int launch_row2<double, kRow2Rows>(sa_ctx*, const Plan&, int, const RowArgs<double>&);
template int launch_row2<double, 16>(sa_ctx*, const Plan&, int, const RowArgs<double>&);

}  // namespace sa
