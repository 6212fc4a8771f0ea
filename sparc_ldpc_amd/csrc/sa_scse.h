// sa_scse.h — the host rules of coupled state evolution (sa_sc_se, the
// k_scse_* kernels of sa_se.hip) as pure host code: which batches of coupled
// configurations (n, R, C, W, Pl, sigma over a shared L, M) are accepted, how
// their sections form classes, which tau slot a class reads, the offsets of
// the batch's one class list, and the iteration-0 values phi^0 and tau^2^0.
// No HIP include: csrc/sa_host_check.cpp (`scse`) prints the plan and runs its
// invariants on a machine without a GPU.
//
// Notation (DESIGN.md sections 13, 13a): c_l = sqrt(n Pl_l), P_c = sum of the
// Pl_l of column block c (l in order), column block c(l) = l / (L / C).
//   psi_c^0 = P_c
//   phi_r^t = sigma^2 + sum_c W[r, c] psi_c^t                (c in order)
//   1 / tau_c^2^t = (sum_r W[r, c] / phi_r^t) / R             (r in order)
// A class is the set of sections of one configuration and one column block
// whose powers are equal bit for bit, in order of first appearance; its tau
// slot is (configuration, column block), numbered slot_off[b] + c.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "sparc_amp.h"

namespace sa {

constexpr int kScSeMaxBlocks = SA_SC_MAX_BLOCKS;  // one lane of k_scse_reduce's first wave per block
constexpr int kSeMaxM = SA_SE_MAX_M;              // the largest row of U a workgroup holds
constexpr int kSeRow = 4096;                      // binary64 values of U in a workgroup's LDS (32 KB)
constexpr int kSeSamples = 16;                    // samples per chunk, at most (SC = min(16, kSeRow / M))
constexpr int kSeClasses = 8;                     // classes per workgroup
static_assert(kSeMaxM <= kSeRow, "one row must fit");

struct ScSePlan {
  int B = 0, L = 0, M = 0, T = 0, S = 0;
  std::vector<int> n, R, C;      // [B]
  std::vector<int> slot_off;     // [B + 1] tau slots of configuration b: slot_off[b] + c
  std::vector<int> row_off;      // [B + 1] row blocks of configuration b: row_off[b] + r
  std::vector<long long> w_off;  // [B + 1] first entry of configuration b's W
  std::vector<int> blk_off;      // [NS + 1] class range of each tau slot
  std::vector<int> cfg_off;      // [B + 1] class range of each configuration (= blk_off[slot_off[b]])
  std::vector<double> cls_c;     // [K] c = sqrt(n Pl) of the class
  std::vector<double> cls_w;     // [K] multiplicity * Pl / P_c
  std::vector<int> cls_mult;     // [K]
  std::vector<int> cls_slot;     // [K] its tau slot
  std::vector<int> sec_cls;      // [B][L] the class of each section
  std::vector<double> Pc;        // [NS]
  std::vector<double> sig2;      // [B]
  std::vector<double> phi0;      // [NR] phi_r^0
  std::vector<double> tau20;     // [NS] tau_c^2^0
  int K = 0, NS = 0, NR = 0, Rmax = 0, Cmax = 0;
  int SC = 0, NCH = 0;           // samples per chunk, chunks
  long long grid = 0;            // k_scse_expect's workgroups
};

// phi_r = sig2 + sum_c W[r, c] psi_c and tau_c^2 = 1 / ((sum_r W[r, c] / phi_r) / R),
// each sum in index order from 0: the host's statement of what k_scse_reduce
// does every iteration (one rounding per operation, no contraction).
inline void scse_phi_tau(int R, int C, const double* W, double sig2, const double* psi, double* phi, double* tau2) {
#pragma clang fp contract(off)
  for (int r = 0; r < R; ++r) {
    double acc = 0;
    for (int c = 0; c < C; ++c) acc += W[(size_t)r * C + c] * psi[c];
    phi[r] = sig2 + acc;
  }
  for (int c = 0; c < C; ++c) {
    double acc = 0;
    for (int r = 0; r < R; ++r) acc += W[(size_t)r * C + c] / phi[r];
    tau2[c] = 1.0 / (acc / (double)R);
  }
}

// The plan of a batch, or why there is none: SA_ERR_ARG for an argument fault,
// SA_ERR_UNSUPPORTED for a valid batch outside the kernels' range; err names
// the argument and the configuration.
inline int scse_plan(ScSePlan& p, int B, int L, int M, const int* n, const int* R, const int* C, const double* W,
                     const double* Pl, const double* sigma, int T, int S, std::string& err) {
  p = ScSePlan();
  if (B < 1) { err = "B < 1"; return SA_ERR_ARG; }
  if (L < 1) { err = "L < 1"; return SA_ERR_ARG; }
  if (M < 2) { err = "M < 2"; return SA_ERR_ARG; }
  if (T < 1) { err = "T < 1"; return SA_ERR_ARG; }
  if (S < 1) { err = "S < 1"; return SA_ERR_ARG; }
  if (!n || !R || !C || !W || !Pl || !sigma) { err = "n, R, C, W, Pl and sigma must be given"; return SA_ERR_ARG; }
  p.B = B; p.L = L; p.M = M; p.T = T; p.S = S;
  p.n.assign(n, n + B); p.R.assign(R, R + B); p.C.assign(C, C + B);
  p.slot_off.assign(B + 1, 0); p.row_off.assign(B + 1, 0); p.w_off.assign(B + 1, 0); p.cfg_off.assign(B + 1, 0);
  p.sec_cls.assign((size_t)B * L, 0);
  p.sig2.assign(B, 0.0);
  p.blk_off.push_back(0);
  for (int b = 0; b < B; ++b) {
    const std::string cfg = "configuration " + std::to_string(b) + ": ";
    const int Rb = R[b], Cb = C[b], nb = n[b];
    if (nb < 1) { err = cfg + "n < 1"; return SA_ERR_ARG; }
    if (Rb < 1) { err = cfg + "R must be at least 1"; return SA_ERR_ARG; }
    if (Cb < 1) { err = cfg + "C must be at least 1"; return SA_ERR_ARG; }
    if (Rb > kScSeMaxBlocks) { err = cfg + "R above SA_SC_MAX_BLOCKS = " + std::to_string(kScSeMaxBlocks); return SA_ERR_UNSUPPORTED; }
    if (Cb > kScSeMaxBlocks) { err = cfg + "C above SA_SC_MAX_BLOCKS = " + std::to_string(kScSeMaxBlocks); return SA_ERR_UNSUPPORTED; }
    if (nb % Rb != 0) { err = cfg + "R = " + std::to_string(Rb) + " does not divide n = " + std::to_string(nb); return SA_ERR_ARG; }
    if (L % Cb != 0) { err = cfg + "C = " + std::to_string(Cb) + " does not divide L = " + std::to_string(L); return SA_ERR_ARG; }
    const double* Wb = W + p.w_off[b];
    for (int r = 0; r < Rb; ++r)
      for (int c = 0; c < Cb; ++c) {
        const double v = Wb[(size_t)r * Cb + c];
        const std::string at = cfg + "W[" + std::to_string(r) + "," + std::to_string(c) + "]";
        if (!std::isfinite(v)) { err = at + " is not finite"; return SA_ERR_ARG; }
        if (v < 0) { err = at + " is negative"; return SA_ERR_ARG; }
      }
    for (int r = 0; r < Rb; ++r) {
      bool any = false;
      for (int c = 0; c < Cb; ++c) any = any || Wb[(size_t)r * Cb + c] > 0;
      if (!any) { err = cfg + "W row " + std::to_string(r) + " has no positive entry"; return SA_ERR_ARG; }
    }
    for (int c = 0; c < Cb; ++c) {
      bool any = false;
      for (int r = 0; r < Rb; ++r) any = any || Wb[(size_t)r * Cb + c] > 0;
      if (!any) { err = cfg + "W column " + std::to_string(c) + " has no positive entry"; return SA_ERR_ARG; }
    }
    if (!(sigma[b] > 0) || !std::isfinite(sigma[b])) {
      err = "sigma[" + std::to_string(b) + "] must be finite and > 0";
      return SA_ERR_ARG;
    }
    const double* pl = Pl + (size_t)b * L;
    for (int l = 0; l < L; ++l)
      if (!(pl[l] >= 0) || !std::isfinite(pl[l])) {
        err = "Pl[" + std::to_string(b) + "][" + std::to_string(l) + "] must be finite and >= 0";
        return SA_ERR_ARG;
      }
    // the classes of each column block: its distinct powers in order of first appearance
    const int Lc = L / Cb;
    for (int c = 0; c < Cb; ++c) {
      double P = 0;
      for (int l = c * Lc; l < (c + 1) * Lc; ++l) P += pl[l];
      if (!(P > 0)) { err = cfg + "P_c = 0 for column block " + std::to_string(c); return SA_ERR_ARG; }
      if (!std::isfinite(P)) { err = cfg + "P_c overflows for column block " + std::to_string(c); return SA_ERR_ARG; }
      const int slot = p.slot_off[b] + c;
      const int k0 = (int)p.cls_c.size();
      std::unordered_map<uint64_t, int> seen;
      std::vector<double> cls_pl;
      for (int l = c * Lc; l < (c + 1) * Lc; ++l) {
        uint64_t bits;
        std::memcpy(&bits, &pl[l], sizeof(bits));
        auto it = seen.find(bits);
        if (it == seen.end()) {
          it = seen.emplace(bits, (int)p.cls_c.size()).first;
          p.cls_c.push_back(std::sqrt((double)nb * pl[l]));
          cls_pl.push_back(pl[l]);
          p.cls_mult.push_back(0);
          p.cls_slot.push_back(slot);
        }
        ++p.cls_mult[it->second];
        p.sec_cls[(size_t)b * L + l] = it->second;
      }
      for (size_t k = k0; k < p.cls_c.size(); ++k) p.cls_w.push_back((double)p.cls_mult[k] * cls_pl[k - k0] / P);
      p.blk_off.push_back((int)p.cls_c.size());
      p.Pc.push_back(P);
    }
    p.sig2[b] = sigma[b] * sigma[b];
    p.slot_off[b + 1] = p.slot_off[b] + Cb;
    p.row_off[b + 1] = p.row_off[b] + Rb;
    p.w_off[b + 1] = p.w_off[b] + (long long)Rb * Cb;
    p.cfg_off[b + 1] = (int)p.cls_c.size();
    p.Rmax = Rb > p.Rmax ? Rb : p.Rmax;
    p.Cmax = Cb > p.Cmax ? Cb : p.Cmax;
  }
  if (M > kSeMaxM) { err = "M above SA_SE_MAX_M = " + std::to_string(kSeMaxM); return SA_ERR_UNSUPPORTED; }
  if (S > (1 << 24)) { err = "S above 2^24"; return SA_ERR_UNSUPPORTED; }
  p.K = (int)p.cls_c.size();
  p.NS = p.slot_off[B];
  p.NR = p.row_off[B];
  p.SC = kSeRow / M < kSeSamples ? kSeRow / M : kSeSamples;
  p.NCH = (S + p.SC - 1) / p.SC;
  p.grid = (long long)p.NCH * ((p.K + kSeClasses - 1) / kSeClasses);
  if (p.grid >= (1LL << 31)) { err = "classes x sample chunks above 2^31 workgroups"; return SA_ERR_UNSUPPORTED; }
  p.phi0.assign(p.NR, 0.0);
  p.tau20.assign(p.NS, 0.0);
  for (int b = 0; b < B; ++b)
    scse_phi_tau(R[b], C[b], W + p.w_off[b], p.sig2[b], p.Pc.data() + p.slot_off[b], p.phi0.data() + p.row_off[b],
                 p.tau20.data() + p.slot_off[b]);
  return SA_OK;
}

// What the kernels rely on, checked on a plan: every class in exactly one tau
// slot's range and that slot its own, the ranges of a configuration's slots
// back to back, every section in a class of its own column block with its
// power's c, the multiplicities adding up to L / C per block and the weights
// to 1 (to rounding), a chunk within the LDS row buffer.  Empty: holds.
inline std::string scse_check_plan(const ScSePlan& p, const double* Pl) {
  if ((int)p.blk_off.size() != p.NS + 1 || p.blk_off[0] != 0 || p.blk_off[p.NS] != p.K) return "blk_off does not span the classes";
  for (int q = 0; q < p.NS; ++q) {
    if (p.blk_off[q + 1] <= p.blk_off[q]) return "tau slot " + std::to_string(q) + " has no class";
    for (int k = p.blk_off[q]; k < p.blk_off[q + 1]; ++k)
      if (p.cls_slot[k] != q) return "class " + std::to_string(k) + " lies outside its tau slot's range";
  }
  for (int b = 0; b < p.B; ++b) {
    if (p.cfg_off[b] != p.blk_off[p.slot_off[b]] || p.cfg_off[b + 1] != p.blk_off[p.slot_off[b + 1]])
      return "configuration " + std::to_string(b) + ": class range is not its slots' ranges";
    if (p.R[b] > kScSeMaxBlocks || p.C[b] > kScSeMaxBlocks) return "more blocks than lanes";
    const int Lc = p.L / p.C[b];
    std::vector<int> cnt(p.K, 0);
    for (int l = 0; l < p.L; ++l) {
      const int k = p.sec_cls[(size_t)b * p.L + l];
      if (k < p.cfg_off[b] || k >= p.cfg_off[b + 1]) return "a section's class lies outside its configuration";
      if (p.cls_slot[k] != p.slot_off[b] + l / Lc) return "a section's class reads another block's tau";
      if (p.cls_c[k] != std::sqrt((double)p.n[b] * Pl[(size_t)b * p.L + l])) return "a section's class has another c";
      ++cnt[k];
    }
    for (int c = 0; c < p.C[b]; ++c) {
      const int q = p.slot_off[b] + c;
      int m = 0;
      double w = 0;
      for (int k = p.blk_off[q]; k < p.blk_off[q + 1]; ++k) {
        if (cnt[k] != p.cls_mult[k]) return "class " + std::to_string(k) + ": multiplicity is not its section count";
        m += p.cls_mult[k];
        w += p.cls_w[k];
      }
      if (m != Lc) return "tau slot " + std::to_string(q) + ": multiplicities do not add up to L / C";
      if (!(std::fabs(w - 1.0) <= 1e-12 * (1 + p.blk_off[q + 1] - p.blk_off[q]))) return "tau slot " + std::to_string(q) + ": weights do not add up to 1";
    }
  }
  if (p.SC < 1 || (long long)p.SC * p.M > kSeRow) return "a chunk's rows past the LDS buffer";
  if ((long long)p.NCH * p.SC < p.S) return "the chunks do not cover the samples";
  return "";
}

}  // namespace sa
