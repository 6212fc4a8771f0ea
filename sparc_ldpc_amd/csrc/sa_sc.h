// sa_sc.h — the host rules of the spatially coupled decoder (sa_sc.hip) as
// pure host code: what (R, C, W) a coupled design over an operator of L
// sections of M columns and n rows may have, which row block a row and which
// column block a section lies in, how the sections form the workgroups of
// k_scsec and the rows the z^2 partials of k_scrow, the limits, and each
// kernel's LDS bytes.  No HIP include: csrc/sa_host_check.cpp (`sc`) prints
// the layout and runs its invariants on a machine without a GPU.
//
// The coupled design is A[i, j] = sqrt(W[r(i), c(j)]) * At[i, j], At the
// +-1/sqrt(n) operator of the parent context, W an R x C base matrix, row
// block r(i) = i / (n / R), column block c(l) = l / (L / C) (DESIGN.md
// section 13).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sa_shape.h"
#include "sa_tables.h"

namespace sa {

// Row blocks R and column blocks C of a base matrix: at most one wavefront's
// lanes, so that k_scrow holds the C values psi_c one per lane and k_scsec
// writes the R values phi_r of an iteration with one store instruction.  The
// LDS they cost k_scsec (three arrays of kScMaxBlocks reals, 1.5 KB in
// binary64) is under 1 % of the image.
constexpr int kScMaxBlocks = 64;  // SA_SC_MAX_BLOCKS
static_assert(kScMaxBlocks == SA_SC_MAX_BLOCKS, "sparc_amp.h states the limit");
constexpr int kScRowsPerBlk = 64; // rows of one z^2 partial (one k_scrow workgroup, one per lane)

struct ScLayout {
  int R = 0, C = 0;          // the base matrix is R x C
  int L = 0, M = 0, n = 0, prec = 0;
  int n_r = 0, L_c = 0;      // rows per row block, sections per column block
  // section groups (k_scsec workgroups of kSpw sections, one wave each): gpc per
  // column block, the last of a block padded with absent sections where
  // L_c % kSpw != 0, so no group straddles a column block
  int gpc = 0, G = 0;
  // z^2 partials (k_scrow workgroups of kScRowsPerBlk rows): zpb per row block,
  // the last of a block short where n_r % kScRowsPerBlk != 0
  int zpb = 0, NZ = 0;
  // the groups are the parent's groups of 4 consecutive sections (L_c % kSpw
  // == 0: its Ab table fwd is borrowed), else the coupled context builds its own
  bool own_fwd = false;
  int w = 0, nhi = 0, E = 1;  // the parent operator's transform (Shape)
  size_t sec_lds = 0;         // k_scsec's LDS bytes (k_scrow: none)
};

inline int sc_row_block(const ScLayout& s, int i) { return i / s.n_r; }
inline int sc_col_block(const ScLayout& s, int l) { return l / s.L_c; }
// column block of section group g, and its section of wave wv (-1: absent)
inline int sc_group_block(const ScLayout& s, int g) { return g / s.gpc; }
inline int sc_group_section(const ScLayout& s, int g, int wv) {
  const int ls = (g % s.gpc) * kSpw + wv;
  return ls < s.L_c ? sc_group_block(s, g) * s.L_c + ls : -1;
}
// row block of z^2 partial q, its first row and its number of rows
inline int sc_zpart_block(const ScLayout& s, int q) { return q / s.zpb; }
inline int sc_zpart_row0(const ScLayout& s, int q) { return (q / s.zpb) * s.n_r + (q % s.zpb) * kScRowsPerBlk; }
inline int sc_zpart_rows(const ScLayout& s, int q) {
  const int left = s.n_r - (q % s.zpb) * kScRowsPerBlk;
  return left < kScRowsPerBlk ? left : kScRowsPerBlk;
}

// k_scsec's LDS image: k_sec's (z slots, 4 sections' T, 4 beta^2 partials),
// then phi_r, W[r, c] / phi_r and the z scale of each row block, then the
// four waves' stop flags
inline size_t sc_sec_lds_need(int M, int n, size_t s) {
  return sec_lds_need(M, n, s, true) + 3 * (size_t)kScMaxBlocks * s + 16;
}

// The layout of a coupled design, or why there is none: SA_ERR_ARG for a
// (R, C, W) that is no base matrix of this (L, n), SA_ERR_UNSUPPORTED for a
// valid one outside the kernels' range; err names the argument.
inline int sc_layout(ScLayout& s, int L, int M, int n, int prec, int R, int C, const double* W, std::string& err) {
  s = ScLayout();
  if (L <= 0 || M <= 0 || n <= 0) { err = "L, M, n must be positive"; return SA_ERR_ARG; }
  if (prec != SA_PREC_F32 && prec != SA_PREC_F64) { err = "unknown precision"; return SA_ERR_ARG; }
  if (R < 1) { err = "R must be at least 1"; return SA_ERR_ARG; }
  if (C < 1) { err = "C must be at least 1"; return SA_ERR_ARG; }
  if (!W) { err = "W is NULL"; return SA_ERR_ARG; }
  if (R > kScMaxBlocks) { err = "R above SA_SC_MAX_BLOCKS = " + std::to_string(kScMaxBlocks); return SA_ERR_UNSUPPORTED; }
  if (C > kScMaxBlocks) { err = "C above SA_SC_MAX_BLOCKS = " + std::to_string(kScMaxBlocks); return SA_ERR_UNSUPPORTED; }
  if ((M & (M - 1)) != 0) { err = "M must be a power of two for a coupled design"; return SA_ERR_UNSUPPORTED; }
  if (M > 4096) { err = "M must be <= 4096"; return SA_ERR_UNSUPPORTED; }
  if (n % R != 0) { err = "R = " + std::to_string(R) + " does not divide n = " + std::to_string(n); return SA_ERR_ARG; }
  if (L % C != 0) { err = "C = " + std::to_string(C) + " does not divide L = " + std::to_string(L); return SA_ERR_ARG; }
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) {
      const double v = W[(size_t)r * C + c];
      if (!std::isfinite(v)) { err = "W[" + std::to_string(r) + "," + std::to_string(c) + "] is not finite"; return SA_ERR_ARG; }
      if (v < 0) { err = "W[" + std::to_string(r) + "," + std::to_string(c) + "] is negative"; return SA_ERR_ARG; }
    }
  for (int r = 0; r < R; ++r) {
    bool any = false;
    for (int c = 0; c < C; ++c) any = any || W[(size_t)r * C + c] > 0;
    if (!any) { err = "W row " + std::to_string(r) + " has no positive entry"; return SA_ERR_ARG; }
  }
  for (int c = 0; c < C; ++c) {
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || W[(size_t)r * C + c] > 0;
    if (!any) { err = "W column " + std::to_string(c) + " has no positive entry"; return SA_ERR_ARG; }
  }
  const size_t sz = prec == SA_PREC_F64 ? 8 : 4;
  s.sec_lds = sc_sec_lds_need(M, n, sz);
  if (n >= 65535 || s.sec_lds > kLdsBytes) {
    err = "n too large: z must fit the section kernel's LDS image (" + std::to_string(s.sec_lds) + " bytes needed)";
    return SA_ERR_UNSUPPORTED;
  }
  s.R = R; s.C = C; s.L = L; s.M = M; s.n = n; s.prec = prec;
  s.n_r = n / R;
  s.L_c = L / C;
  s.gpc = (s.L_c + kSpw - 1) / kSpw;
  s.G = C * s.gpc;
  s.zpb = (s.n_r + kScRowsPerBlk - 1) / kScRowsPerBlk;
  s.NZ = R * s.zpb;
  s.own_fwd = s.L_c % kSpw != 0;
  const int mx = (M + 1) > (n + 1) ? (M + 1) : (n + 1);
  s.w = 1 << ilog2(mx);
  s.nhi = s.w / M;
  s.E = 1;
  while (s.E * 64 < M) s.E *= 2;
  return SA_OK;
}

// The Ab table of the padded groups, [G][n][4]: fwd_entry of each present
// section's ordering value, 0 for an absent section (whose T is zero).
inline void sc_fwd_table(const ScLayout& s, const uint32_t* ordering, uint16_t* out) {
  const int lgM = ilog2(s.M);
  for (int g = 0; g < s.G; ++g)
    for (int wv = 0; wv < kSpw; ++wv) {
      const int l = sc_group_section(s, g, wv);
      for (int r = 0; r < s.n; ++r)
        out[((size_t)g * s.n + r) * kSpw + wv] = l < 0 ? (uint16_t)0 : fwd_entry(ordering[(size_t)l * s.n + r], lgM, s.M);
    }
}

// What the kernels rely on, checked on a layout: every section in exactly one
// group, no group across a column block; every row in exactly one z^2
// partial, none across a row block; the LDS within the CU's.  Empty: holds.
inline std::string sc_check_layout(const ScLayout& s) {
  std::vector<int> seen(s.L, 0);
  for (int g = 0; g < s.G; ++g)
    for (int wv = 0; wv < kSpw; ++wv) {
      const int l = sc_group_section(s, g, wv);
      if (l < 0) continue;
      if (l >= s.L) return "group " + std::to_string(g) + " names section " + std::to_string(l);
      if (sc_col_block(s, l) != sc_group_block(s, g)) return "group " + std::to_string(g) + " straddles a column block";
      ++seen[l];
    }
  for (int l = 0; l < s.L; ++l)
    if (seen[l] != 1) return "section " + std::to_string(l) + " sits in " + std::to_string(seen[l]) + " groups";
  std::vector<int> rows(s.n, 0);
  for (int q = 0; q < s.NZ; ++q) {
    const int r0 = sc_zpart_row0(s, q), cnt = sc_zpart_rows(s, q);
    if (cnt < 1 || r0 < 0 || r0 + cnt > s.n) return "z^2 partial " + std::to_string(q) + " out of range";
    if (sc_row_block(s, r0) != sc_zpart_block(s, q) || sc_row_block(s, r0 + cnt - 1) != sc_zpart_block(s, q))
      return "z^2 partial " + std::to_string(q) + " straddles a row block";
    for (int i = r0; i < r0 + cnt; ++i) ++rows[i];
  }
  for (int i = 0; i < s.n; ++i)
    if (rows[i] != 1) return "row " + std::to_string(i) + " sits in " + std::to_string(rows[i]) + " z^2 partials";
  if (s.NZ > s.n) return "more z^2 partials than z slots (k_scsec stages them there)";
  if (s.sec_lds > kLdsBytes) return "k_scsec's LDS image past the CU's";
  return "";
}

// ---- the tolerance stop and the frozen column blocks ----
// taul, tau_c^2 of block c's last live iteration: [B][2][C] reals indexed by the
// parity of t.  In the launch of iteration t every group reads parity t - 1 and
// the first group of a block writes parity t, so no workgroup reads a word
// another workgroup of the same launch writes (section 13's launch rule).
inline size_t sc_taul_index(const ScLayout& s, int b, int t, int c) { return ((size_t)b * 2 + (t & 1)) * s.C + c; }
inline size_t sc_taul_bytes(const ScLayout& s, int B) { return (size_t)B * 2 * s.C * (s.prec == SA_PREC_F64 ? 8 : 4); }
// the live trace, [B][T][C] bytes
inline size_t sc_live_index(const ScLayout& s, int T, int b, int t, int c) { return ((size_t)b * T + t) * s.C + c; }
inline size_t sc_live_bytes(const ScLayout& s, int B, int T) { return (size_t)B * (T > 1 ? T : 1) * s.C; }

// What a decode with (stop_tol, freeze_tol) launches.  The tolerances are taken
// in the working precision (a binary32 context rounds them): wave == false, both
// 0 there, is the decode without tolerances, k_scsec's default instances and no
// extra workspace; else the wave form runs, with the table loads behind the
// liveness test (late_loads) where a block may be frozen.
struct ScWavePlan {
  bool wave = false, late_loads = false;
  double stop_tol = 0, freeze_tol = 0;  // as the kernel gets them
  size_t taul_bytes = 0, live_bytes = 0;
};

inline int sc_wave_plan(ScWavePlan& p, const ScLayout& s, int B, int T, double stop_tol, double freeze_tol, bool want_live,
                        std::string& err) {
  p = ScWavePlan();
  if (!std::isfinite(stop_tol) || stop_tol < 0) { err = "stop_tol must be finite and non-negative"; return SA_ERR_ARG; }
  if (!std::isfinite(freeze_tol) || freeze_tol < 0) { err = "freeze_tol must be finite and non-negative"; return SA_ERR_ARG; }
  if (B < 1 || T < 0) { err = "B must be positive and T non-negative"; return SA_ERR_ARG; }
  const bool f32 = s.prec != SA_PREC_F64;
  p.stop_tol = f32 ? (double)(float)stop_tol : stop_tol;
  p.freeze_tol = f32 ? (double)(float)freeze_tol : freeze_tol;
  if (!std::isfinite(p.stop_tol)) { err = "stop_tol is past the working precision's range"; return SA_ERR_ARG; }
  if (!std::isfinite(p.freeze_tol)) { err = "freeze_tol is past the working precision's range"; return SA_ERR_ARG; }
  p.wave = p.stop_tol > 0 || p.freeze_tol > 0;
  p.late_loads = p.freeze_tol > 0;
  if (p.wave) {
    p.taul_bytes = sc_taul_bytes(s, B);
    p.live_bytes = want_live ? sc_live_bytes(s, B, T) : 0;
  }
  return SA_OK;
}

// What the wave form relies on: in every launch the taul words read (parity
// t - 1) and written (parity t) are disjoint and inside the buffer, a block has
// exactly one writing group (g % gpc == 0), and the live trace's bytes are each
// written by one group and inside theirs.  Empty: holds.
inline std::string sc_check_wave(const ScLayout& s, int B, int T) {
  const size_t words = sc_taul_bytes(s, B) / (s.prec == SA_PREC_F64 ? 8 : 4), lb = sc_live_bytes(s, B, T);
  std::vector<int> writers(s.C, 0);
  for (int g = 0; g < s.G; ++g)
    if (g % s.gpc == 0) ++writers[sc_group_block(s, g)];
  for (int c = 0; c < s.C; ++c)
    if (writers[c] != 1) return "block " + std::to_string(c) + " has " + std::to_string(writers[c]) + " writing groups";
  std::vector<unsigned char> seen(lb, 0);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t) {
      for (int c = 0; c < s.C; ++c) {
        const size_t wr = sc_taul_index(s, b, t, c), li = sc_live_index(s, T, b, t, c);
        if (wr >= words) return "taul write out of range";
        if (li >= lb || seen[li]++) return "live trace byte out of range or written twice";
        if (t == 0) continue;
        for (int c2 = 0; c2 < s.C; ++c2)
          if (sc_taul_index(s, b, t - 1, c2) == wr || sc_taul_index(s, b, t - 1, c2) >= words)
            return "taul: a word read and written in the launch of iteration " + std::to_string(t);
      }
      // another codeword's words are never this one's
      if (b + 1 < B && sc_taul_index(s, b + 1, 0, 0) <= sc_taul_index(s, b, 1, s.C - 1)) return "taul: codewords overlap";
    }
  return "";
}

// ---- the beta_0 start, the staged context and the glue on it ----
// What a decode launches, in order.  Without a beta_0 it is the list the
// decoder has always had; with one, beta stays as staged and A beta_0 (sc_ab:
// k_scsec in SC_AB mode, k_scrow in SCR_ABOUT) and k_scstart (z = y - A beta_0,
// its z^2 partials, iters = -1, done = 0) stand in for the SCR_INIT row launch.
// sc_decode (sa_sc.hip) walks this list and launches nothing else.
enum ScStep {
  SCS_MEMSET_BETA, SCS_MEMSET_PHI, SCS_MEMSET_LIVE, SCS_ROW_INIT, SCS_SEC_AB, SCS_ROW_ABOUT, SCS_START, SCS_SEC_AMP,
  SCS_SEC_WAVE, SCS_ROW_AMP
};
struct ScLaunch {
  int step, t;
};

inline const char* sc_step_name(int step) {
  switch (step) {
    case SCS_MEMSET_BETA: return "memset beta";
    case SCS_MEMSET_PHI: return "memset phi";
    case SCS_MEMSET_LIVE: return "memset live";
    case SCS_ROW_INIT: return "k_scrow SCR_INIT";
    case SCS_SEC_AB: return "k_scsec SC_AB";
    case SCS_ROW_ABOUT: return "k_scrow SCR_ABOUT";
    case SCS_START: return "k_scstart";
    case SCS_SEC_AMP: return "k_scsec SC_AMP";
    case SCS_SEC_WAVE: return "k_scsec_wave SC_AMP";
    case SCS_ROW_AMP: return "k_scrow SCR_AMP";
  }
  return "?";
}

inline std::vector<ScLaunch> sc_decode_launches(int T, bool beta0, const ScWavePlan& wv) {
  std::vector<ScLaunch> v;
  if (!beta0) v.push_back({SCS_MEMSET_BETA, 0});
  v.push_back({SCS_MEMSET_PHI, 0});
  if (wv.wave && wv.live_bytes) v.push_back({SCS_MEMSET_LIVE, 0});
  if (beta0) {
    v.push_back({SCS_SEC_AB, 0});
    v.push_back({SCS_ROW_ABOUT, 0});
    v.push_back({SCS_START, 0});
  } else {
    v.push_back({SCS_ROW_INIT, 0});
  }
  for (int t = 0; t < T; ++t) {
    v.push_back({wv.wave ? SCS_SEC_WAVE : SCS_SEC_AMP, t});
    v.push_back({SCS_ROW_AMP, t});
  }
  return v;
}

// The staged life cycle: what is on the device between calls.  power: c_l and
// P_c of a sa_sc_stage_power (or of a one-call decode, which stages its own); y: a staged input
// of B codewords in d_y; beta: a beta in d_beta a decode may start from (staged,
// written by the glue, or left by the last run).
struct ScStageState {
  bool power = false, y = false, beta = false;
  int B = 0;
};

enum ScCall {
  SC_CALL_RESIZE,       // the workspace was reallocated: nothing staged survives
  SC_CALL_ONE_CALL,     // sa_sc_amp*, sa_sc_mc*, sa_sc_Ab / Az: they overwrite the workspace
  SC_CALL_STAGE_POWER,
  SC_CALL_STAGE,        // y alone
  SC_CALL_STAGE_BETA0,  // y and beta_0
  SC_CALL_ENCODE,       // sa_sc_encode, sa_sc_encode_bits
  SC_CALL_RUN,
  SC_CALL_RUN_BETA0,    // SA_FLAG_BETA0
  SC_CALL_FETCH,        // sa_sc_fetch, sa_sc_decide
  SC_CALL_LLR,          // reads beta
  SC_CALL_HARD,         // sa_sc_hard_indices: reads the app alone
  SC_CALL_SOFT_BETA0,   // rewrites beta
  SC_CALL_ONEHOT
};

// The argument and state checks of a staged call of B codewords on a context
// whose workspace holds Bcap, and the state it leaves.  SA_ERR_ARG with err
// naming the reason, state untouched; SA_OK and the new state otherwise.
inline int sc_stage_rule(ScStageState& st, int call, int B, int Bcap, std::string& err) {
  if (call == SC_CALL_RESIZE || call == SC_CALL_ONE_CALL) {
    st.y = st.beta = false;
    st.B = 0;
    return SA_OK;
  }
  if (call == SC_CALL_STAGE_POWER) {
    st.power = true;
    return SA_OK;
  }
  if (B < 1 || B > 65535) { err = "B must be in [1, 65535]"; return SA_ERR_ARG; }
  if (B > Bcap) { err = "batch larger than the reserved workspace (sa_sc_reserve)"; return SA_ERR_ARG; }
  const bool needs_power = call != SC_CALL_STAGE && call != SC_CALL_STAGE_BETA0 && call != SC_CALL_FETCH;
  if (needs_power && !st.power) { err = "power allocation not staged"; return SA_ERR_ARG; }
  switch (call) {
    case SC_CALL_STAGE:
    case SC_CALL_STAGE_BETA0:
    case SC_CALL_ENCODE:
      st.y = true;
      st.B = B;
      st.beta = call == SC_CALL_STAGE_BETA0;
      return SA_OK;
    case SC_CALL_RUN:
    case SC_CALL_RUN_BETA0:
      if (!st.y) { err = "nothing staged"; return SA_ERR_ARG; }
      if (B > st.B) { err = "B above the staged batch"; return SA_ERR_ARG; }
      if (call == SC_CALL_RUN_BETA0 && !st.beta) { err = "SA_FLAG_BETA0: no beta staged"; return SA_ERR_ARG; }
      st.beta = true;  // the estimate the run leaves
      return SA_OK;
    case SC_CALL_LLR:
      if (!st.beta) { err = "no beta staged"; return SA_ERR_ARG; }
      return SA_OK;
    case SC_CALL_SOFT_BETA0:
    case SC_CALL_ONEHOT:
      st.beta = true;
      return SA_OK;
    default:
      return SA_OK;
  }
}

// The section range of a glue call: the LDPC code's sections [l0, l0 + ns).
// Any l0 is legal, 0 (every section protected) and one inside a column block included.
inline int sc_glue_check(const ScLayout& s, int l0, int ns, std::string& err) {
  if (l0 < 0) { err = "l0 must be non-negative"; return SA_ERR_ARG; }
  if (ns < 1) { err = "ns must be at least 1"; return SA_ERR_ARG; }
  if ((long long)l0 + ns > s.L) { err = "section range outside [0, L)"; return SA_ERR_ARG; }
  if (s.M < 2) { err = "M < 2 carries no bits"; return SA_ERR_UNSUPPORTED; }
  return SA_OK;
}

// What the staged context and the glue hold beyond the decoder's workspace: c_l
// in binary64 for the glue kernels, and the binary64 staging buffer of a glue
// call that is handed host LLRs / a-posteriori values (none with SA_PTR_DEVICE).
inline size_t sc_cd_bytes(const ScLayout& s) { return (size_t)s.L * sizeof(double); }
inline size_t sc_glue_stage_bytes(const ScLayout& s, int B, int ns) {
  return (size_t)B * ns * ilog2(s.M) * sizeof(double);
}

}  // namespace sa
