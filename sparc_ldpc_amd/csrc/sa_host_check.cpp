// sa_host_check — the operator's host rules from the command line, on a
// machine without a GPU (sa_shape.h, sa_seq.h and sa_tables.h only; no HIP).
//
//   sa_host_check shape L M n backend prec plan n_cus B
//     one JSON object: the Shape of the operator, the plan of a decode of B
//     codewords in sa_plan's field order and, where B runs k_secb,
//     sa_plan_batched's four numbers; {"error", "message"} for a shape that
//     sa_create refuses as unsupported.
//   sa_host_check sweep L M backend prec plan n_cus B n0 n1
//     the section path of a decode of B codewords at every n of [n0, n1], as
//     one JSON list of runs [first n, last n, sec, big]: consecutive n with
//     the same section path (sa_plan's number; -1: sa_create refuses the
//     shape) and the same `big`.
//   sa_host_check seq L M n backend prec plan n_cus B T flags has_b0 profiled
//     the launch sequence of a decode (sa_seq.h: decode_seq) as one JSON
//     object: the DecodeSeq summary (fused, the deferred row step or null,
//     zil, beta_final, nsteps) and "steps", every Step in launch order.  (A
//     dense backend's Ab partial count is device state: 0 here.)
//   sa_host_check tables L M n prec plan
//     draws a valid ordering (per section a seeded shuffle of 1 .. w-1, its
//     first n), builds every table of the Hadamard operator with the pure
//     builders and checks what the kernels rely on; exit status 1 with the
//     first violation on stderr.
//   sa_host_check packed L M n prec plan
//     the same ordering; builds the packed bucket and pair Ab tables of
//     k_sec4 / k_sec44 where the shape rules ask for them, unpacks them and
//     compares every entry with inv and fwd2; one JSON object with the rule's
//     answer and the byte counts, exit status 1 at the first difference.
//   sa_host_check sc L M n prec R C W[0,0] W[0,1] ... W[R-1,C-1]
//     the layout of a spatially coupled design (sa_sc.h: sc_layout) as one JSON
//     object: the block sizes, the section groups [column block, first
//     section, sections], the z^2 partials [row block, first row, rows], the
//     LDS bytes and the limits; {"error", "message"} for a (R, C, W) that
//     sa_sc_create refuses.  Runs the layout's invariants and compares the
//     padded groups' Ab table with fwd_entry on a drawn ordering: exit status
//     1 with the first violation on stderr.  W entries are read by strtod
//     ("nan", "inf" included).
//   sa_host_check scwave L M n prec R C B T stop_tol freeze_tol want_live W[0,0] ... W[R-1,C-1]
//   sa_host_check scjoint L M n prec R C B T l0 ns beta0 stop_tol freeze_tol W[0,0] ... W[R-1,C-1] [call ...]
//     the plan of a coupled decode with a tolerance stop and frozen column
//     blocks (sa_sc.h: sc_wave_plan) as one JSON object: whether k_scsec's wave
//     form runs and which instance ("k_scsec<f32, 8>" / "k_scsec_wave<f32, 8>"),
//     the tolerances as the kernel gets them (17 significant digits), whether
//     the table loads wait for the liveness test, the grid, the LDS bytes and
//     the bytes of the taul buffer and of the live trace; {"error", "message"}
//     for a layout or a tolerance that is refused.  Runs the layout's and the
//     wave form's invariants (sc_check_layout, sc_check_wave): exit status 1
//     with the first violation on stderr.  Reals are read by strtod.
//   sa_host_check scse B L M T S  then per configuration  n R C sigma W[0,0] ... W[R-1,C-1] Pl[0] ... Pl[L-1]
//     the plan of a coupled state-evolution batch (sa_scse.h: scse_plan) as one
//     JSON object: the per-configuration offsets (tau slots, row blocks, W,
//     classes), the class range of every tau slot, every class [tau slot, c,
//     weight, multiplicity], the class of every section, P_c, sigma^2, phi^0
//     and tau^2^0, the chunking; {"error", "message"} for a batch that
//     sa_sc_se refuses.  Runs the plan's invariants: exit status 1 with the
//     first violation on stderr.  Reals are read by strtod and printed with 17
//     significant digits.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "sa_sc.h"
#include "sa_scse.h"
#include "sa_seq.h"
#include "sa_shape.h"
#include "sa_tables.h"

using namespace sa;

static int usage() {
  std::fprintf(stderr, "usage: sa_host_check shape L M n backend prec plan n_cus B\n"
                       "       sa_host_check sweep L M backend prec plan n_cus B n0 n1\n"
                       "       sa_host_check seq L M n backend prec plan n_cus B T flags has_b0 profiled\n"
                       "       sa_host_check tables L M n prec plan\n"
                       "       sa_host_check packed L M n prec plan\n"
                       "       sa_host_check sc L M n prec R C W...\n"
                       "       sa_host_check scwave L M n prec R C B T stop_tol freeze_tol want_live W...\n"
                       "       sa_host_check scjoint L M n prec R C B T l0 ns beta0 stop_tol freeze_tol W... [call ...]\n"
                       "       sa_host_check scse B L M T S {n R C sigma W... Pl...}...\n");
  return 2;
}

static int shape_of(Shape& s, int L, int M, int n, int backend, int prec, int plan, int n_cus) {
  std::string err;
  int rc = SA_OK;
  if (L <= 0 || M <= 0 || n <= 0 || n_cus <= 0 || backend < SA_BACKEND_HADAMARD || backend > SA_BACKEND_MATRIX ||
      (prec != SA_PREC_F32 && prec != SA_PREC_F64) || (plan & ~SA_PLAN_ALL)) {
    rc = SA_ERR_ARG;
    err = "bad arguments";
  }
  if (!rc) rc = shape_limits(M, n, backend, err);
  if (!rc) rc = shape_for(s, L, M, n, backend, prec, plan, n_cus, err);
  if (rc) std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
  return rc;
}

static int cmd_shape(int L, int M, int n, int backend, int prec, int plan, int n_cus, int B) {
  Shape s;
  if (shape_of(s, L, M, n, backend, prec, plan, n_cus)) return 0;  // reported
  if (B <= 0) return usage();
#define F(x) std::printf("\"" #x "\": %lld, ", (long long)s.x);
  std::printf("{");
  F(L) F(M) F(Mu) F(dead) F(n) F(w) F(nhi) F(E) F(pow2) F(big)
  F(G) F(Gb) F(Gd) F(G2) F(G3) F(G4)
  F(NZ) F(NZ16) F(NZh) F(NZ4) F(NZ2)
  F(sec_lds) F(sec2_lds) F(sec4_lds) F(sec3_lds) F(sec4q_lds) F(secb_lds)
  F(sec3) F(sec4) F(sec4q) F(pt_on) F(row16)
  F(WB) F(CB) F(gpx)
  F(backend) F(prec) F(plan) F(n_cus)
#undef F
  const Plan p = plan_for(s, B);  // (a dense backend's Ab partial count is device state: 0 here)
  std::printf("\"B\": %d, \"zil\": %d, \"plan_of_B\": [%d, %d, %d, %d, %d, %d, %d, %d]", B, p.zil ? 1 : 0, (int)p.sec, p.G,
              (p.sec == SA_SEC_K_SEC || p.sec == SA_SEC_K_SECG) ? p.rs : 1, p.CB, p.nz, s.w, (int)p.row, s.n_cus);
  if (p.batched()) {
    const SecbOrder so = secb_order(s, B);
    std::printf(", \"plan_batched\": [%d, %d, %d, %d]", s.Gb, s.WB, so.gp, so.passes);
  }
  std::printf("}\n");
  return 0;
}

static int cmd_sweep(int L, int M, int backend, int prec, int plan, int n_cus, int B, int n0, int n1) {
  if (L <= 0 || M <= 0 || n_cus <= 0 || B <= 0 || n0 <= 0 || n1 < n0 || backend < SA_BACKEND_HADAMARD ||
      backend > SA_BACKEND_MATRIX || (prec != SA_PREC_F32 && prec != SA_PREC_F64) || (plan & ~SA_PLAN_ALL))
    return usage();
  int first = n0, sec = 0, big = 0, runs = 0;
  std::printf("[");
  for (int n = n0; n <= n1 + 1; ++n) {
    int s1 = -1, b1 = 0;
    if (n <= n1) {
      Shape s;
      std::string err;
      if (!shape_limits(M, n, backend, err) && !shape_for(s, L, M, n, backend, prec, plan, n_cus, err)) {
        s1 = (int)plan_for(s, B).sec;
        b1 = s.big ? 1 : 0;
      }
    }
    if (n > n0 && (n > n1 || s1 != sec || b1 != big)) {
      std::printf("%s[%d, %d, %d, %d]", runs++ ? ", " : "", first, n - 1, sec, big);
      first = n;
    }
    sec = s1;
    big = b1;
  }
  std::printf("]\n");
  return 0;
}

static int print_step(const Step& s) {
  static const char* const kinds[] = {"fill_iters", "zero_beta", "dense_start", "sec_ab",      "row",       "sec",
                                      "sec_mw",     "sec_b",     "dense_iter",  "iters_final", "beta_final"};
  std::printf("{\"kind\": \"%s\", \"t\": %d, \"mode\": %d, \"rd\": %d, \"wr\": %d, \"bzero\": %d, \"decide\": %d, "
              "\"itset\": %d, \"G\": %d, \"Gb\": %d, \"es\": %d}",
              kinds[s.kind], s.t, s.mode, s.rd, s.wr, s.bzero ? 1 : 0, s.decide ? 1 : 0, s.itset, s.G, s.Gb, s.es);
  return 0;
}

static int cmd_seq(const std::vector<int>& a) {
  Shape s;
  if (shape_of(s, a[0], a[1], a[2], a[3], a[4], a[5], a[6])) return 0;  // reported
  const int B = a[7], T = a[8], flags = a[9];
  if (B <= 0 || T < 0) return usage();
  const DecodeSeq q = decode_seq(s, plan_for(s, B), T, flags, a[10] != 0, a[11] != 0);
  std::printf("{\"fused\": %d, \"row\": ", q.fused ? 1 : 0);
  if (q.fused) print_step(q.row);
  else std::printf("null");
  std::printf(", \"zil\": %d, \"beta_final\": %d, \"nsteps\": %d, \"steps\": [", q.zil ? 1 : 0, q.beta_final ? 1 : 0, q.nsteps);
  int k = 0;
  for_each_step(q, [&](const Step& st) {
    if (k++) std::printf(", ");
    return print_step(st);
  });
  std::printf("]}\n");
  return 0;
}

// ---- tables ------------------------------------------------------------------
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::fprintf(stderr, "FAILED: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");              \
      return 1;                                \
    }                                          \
  } while (0)

template <typename T>
static int check_inv(const Shape& s, const std::vector<uint32_t>& ord, std::vector<T>& inv) {
  const int L = s.L, n = s.n, w = s.w;
  inv.assign((size_t)L * w, (T)n);
  for (int l = 0; l < L; ++l) {
    std::string bad;
    CHECK(inv_row(ord.data() + (size_t)l * n, l, n, w, inv.data() + (size_t)l * w, bad), "inv_row: %s", bad.c_str());
    std::vector<int> where(w, n);  // the inverse, by its definition
    for (int r = 0; r < n; ++r) where[ord[(size_t)l * n + r]] = r;
    for (int v = 0; v < w; ++v)
      CHECK((int)inv[(size_t)l * w + v] == where[v], "inv[%d][%d] = %d, expected %d", l, v, (int)inv[(size_t)l * w + v],
            where[v]);
  }
  // a repeated and an out-of-range value are refused with their messages
  std::vector<uint32_t> o2(ord.begin(), ord.begin() + n);
  std::vector<T> il(w, (T)n);
  std::string bad;
  if (n > 1) {
    o2[n - 1] = o2[0];
    CHECK(!inv_row(o2.data(), 0, n, w, il.data(), bad) && bad.find("repeats value") != std::string::npos,
          "a repeated value passed inv_row");
  }
  o2[0] = (uint32_t)w;
  std::fill(il.begin(), il.end(), (T)n);
  CHECK(!inv_row(o2.data(), 0, n, w, il.data(), bad) && bad.find("outside [1, w=") != std::string::npos,
        "an out-of-range value passed inv_row");
  return 0;
}

static int check_fwd(const Shape& s, const std::vector<uint32_t>& ord, std::vector<uint16_t>& fwd) {
  const int L = s.L, n = s.n, M = s.M, lgM = ilog2(M);
  fwd.assign((size_t)fwd_groups(L) * n * kSpw, 0);
  std::vector<uint32_t> fwd2(s.big ? 0 : (size_t)((L + 1) / 2) * n, 0), fwd3(s.sec3 ? (size_t)s.G3 * n : 0, 0);
  for (int l = 0; l < L; ++l)
    fwd_section(ord.data() + (size_t)l * n, l, n, M, fwd.data(), s.big ? nullptr : fwd2.data(),
                s.sec3 ? fwd3.data() : nullptr);
  CHECK(!s.sec3 || M <= 512, "k_sec43's 10-bit fields with M = %d", M);
  const int Lp = fwd_groups(L) * kSpw;
  for (int l = 0; l < Lp; ++l)
    for (int r = 0; r < n; ++r) {
      const uint32_t v = l < L ? ord[(size_t)l * n + r] : 0;
      const unsigned k = l < L ? (v & (uint32_t)(M - 1)) : 0, sg = l < L ? (__builtin_popcount(v >> lgM) & 1) : 0;
      const uint16_t e = fwd[((size_t)(l / kSpw) * n + r) * kSpw + (l % kSpw)];
      CHECK((e & 0x7fffu) == k && (unsigned)(e >> 15) == sg, "fwd[%d][%d] = %#x, expected k %u sign %u", l, r, e, k, sg);
      if (!s.big && l < (L + 1) / 2 * 2) {
        const uint32_t e2 = (fwd2[(size_t)(l / 2) * n + r] >> (16 * (l & 1))) & 0xffffu;
        CHECK((e2 & 0x7fffu) == k && (e2 >> 15) == sg, "fwd2[%d][%d] = %#x, expected k %u sign %u", l, r, e2, k, sg);
      }
      if (s.sec3 && l < s.G3 * 3) {
        const uint32_t e3 = (fwd3[(size_t)(l / 3) * n + r] >> (10 * (l % 3))) & 0x3ffu;
        CHECK((e3 & 0x1ffu) == k && (e3 >> 9) == sg, "fwd3[%d][%d] = %#x, expected k %u sign %u", l, r, e3, k, sg);
      }
    }
  return 0;
}

static int check_banked(const Shape& s, const std::vector<uint16_t>& inv) {
  const int L = s.L, n = s.n, w = s.w, M = s.M, nhi = s.nhi, Sh = nhi / 2, kh = invb_kh(s);
  const std::vector<int> sets = invb_sets(s.E, s.prec == SA_PREC_F32);
  {  // the sets cover every column once
    std::vector<int> seen(M, 0);
    for (int col : sets) {
      CHECK(col >= 0 && col < M, "invb_sets: column %d outside the section", col);
      ++seen[col];
    }
    for (int col = 0; col < M; ++col) CHECK(seen[col] == 1, "invb_sets: column %d in %d sets", col, seen[col]);
  }
  std::vector<uint16_t> out((size_t)L * w, 0xffff);
  std::vector<uint32_t> hs(L, 0);
  for (int l = 0; l < L; ++l)
    banked_section(M, n, nhi, l, inv.data() + (size_t)l * w, out.data() + (size_t)l * w, sets, 16, 16, hs.data(), kh);
  for (int l = 0; l < L; ++l) {
    const uint16_t *il = inv.data() + (size_t)l * w, *ob = out.data() + (size_t)l * w;
    for (int cls = 0; cls < 2; ++cls) {
      const int S = (int)((hs[l] >> (16 * cls)) & 0xffffu);
      // whole blocks of kh steps within the half (a half shorter than kh: all of it)
      CHECK((S % kh == 0 && S >= kh && S <= Sh) || (Sh < kh && S == Sh), "hs[%d] class %d = %d (kh %d, nhi/2 %d)", l, cls, S,
            kh, Sh);
      for (int col = 0; col < M; ++col) {
        std::vector<int> want, got;
        for (int h = 0; h < nhi; ++h)
          if ((__builtin_popcount(h) & 1) == cls && il[(size_t)h * M + col] != (uint16_t)n) want.push_back(il[(size_t)h * M + col]);
        for (int st = 0; st < Sh; ++st) {
          const int v = ob[(size_t)(cls * Sh + st) * M + col];
          if (st >= S) CHECK(v == n, "invb[%d] class %d step %d column %d = %d past hs = %d, expected n", l, cls, st, col, v, S);
          else if (v < n) got.push_back(v);
          else CHECK(v < n + kInvbZeroRows, "invb[%d] class %d step %d column %d = %d: no zero row", l, cls, st, col, v);
        }
        std::sort(want.begin(), want.end());
        std::sort(got.begin(), got.end());
        CHECK(want == got, "invb[%d] class %d column %d: its rows are not those of inv", l, cls, col);
      }
    }
  }
  return 0;
}

static int check_fwdb(const Shape& s, const std::vector<uint16_t>& fwd) {
  const int W = s.WB, M = s.M, n = s.n, L = s.L, E = s.E, npad = (n + 63) & ~63;
  const int rowb = s.CB * (int)rsz(&s);
  const bool search = !(s.plan & SA_PLAN_NO_BANKS), b128 = rowb == 16;
  CHECK(W * M < 32768, "k_secb: W * M >= 2^15");
  std::vector<uint16_t> out((size_t)s.Gb * W * npad, 0xffff);
  for (int g = 0; g < s.Gb; ++g) fwdb_group(W, M, n, L, E, rowb, search, g, fwd.data(), npad, out.data());
  auto at = [&](int g, int r, int st) { return out[((size_t)(g * (W / 4) + st / 4) * npad + r) * 4 + (st % 4)]; };
  const int gsize = b128 ? 16 : 32;
  for (int g = 0; g < s.Gb; ++g) {
    for (int r = 0; r < n; ++r) {
      std::vector<int> want(W), got(W);
      for (int sl = 0; sl < W; ++sl) {
        const int l = g * W + sl;
        const uint16_t e = l < L ? fwd[((size_t)(l / kSpw) * n + r) * kSpw + (l % kSpw)] : 0;  // past L: column 0, +
        want[sl] = (int)(((unsigned)sl * M + t_pos(E, e & 0x7fffu)) | (e & 0x8000u));
        got[sl] = at(g, r, sl);
      }
      if (search) {  // a re-ordering of the same terms
        std::sort(want.begin(), want.end());
        std::sort(got.begin(), got.end());
      }
      CHECK(want == got, "fwdb group %d row %d: its entries are not the row's sections%s", g, r,
            search ? "" : " in section order");
    }
    for (int b0 = 0; b0 < npad; b0 += 64)
      for (int G = 0; G < 64 / gsize; ++G) {
        int lanes[32], real = -1;
        for (int j = 0; j < gsize; ++j) {
          lanes[j] = b128 ? kLdsGroups16[G][j] : G * 32 + j;
          if (real < 0 && b0 + lanes[j] < n) real = b0 + lanes[j];
        }
        for (int j = 0; j < gsize; ++j) {
          const int r = b0 + lanes[j];
          if (r < n) continue;
          for (int st = 0; st < W; ++st)  // an idle row: a real row of its lane group, else column 0 of section st
            CHECK(at(g, r, st) == (real >= 0 ? at(g, real, st) : (uint16_t)((unsigned)st * M)),
                  "fwdb group %d idle row %d step %d = %#x", g, r, st, at(g, r, st));
        }
      }
  }
  return 0;
}

static int cmd_tables(int L, int M, int n, int prec, int plan) {
  Shape s;
  if (shape_of(s, L, M, n, SA_BACKEND_HADAMARD, prec, plan, Shape().n_cus)) return 1;
  std::vector<uint32_t> ord((size_t)L * n), all(s.w - 1);
  for (int l = 0; l < L; ++l) {
    std::mt19937 rng(0x0d0000u + (uint32_t)l);
    std::iota(all.begin(), all.end(), 1u);
    std::shuffle(all.begin(), all.end(), rng);
    std::copy(all.begin(), all.begin() + n, ord.begin() + (size_t)l * n);
  }
  std::vector<uint16_t> inv, fwd;
  std::vector<uint32_t> inv32;
  if (s.big ? check_inv(s, ord, inv32) : check_inv(s, ord, inv)) return 1;
  if (check_fwd(s, ord, fwd)) return 1;
  const bool secb = s.CB > 0 && !s.big, banked = invb_banked(s);
  if (secb && check_fwdb(s, fwd)) return 1;
  if (banked && check_banked(s, inv)) return 1;
  std::printf("{\"ok\": 1, \"M\": %d, \"dead\": %d, \"w\": %d, \"E\": %d, \"big\": %d, \"sec3\": %d, \"CB\": %d, \"WB\": %d, "
              "\"fwdb\": %d, \"fwdb_lanes\": %d, \"banked\": %d, \"kh\": %d, \"search\": %d}\n",
              s.M, s.dead, s.w, s.E, s.big ? 1 : 0, s.sec3 ? 1 : 0, s.CB, s.WB, secb ? 1 : 0,
              secb ? (s.CB * (int)rsz(&s) == 16 ? 16 : 32) : 0, banked ? 1 : 0, banked ? invb_kh(s) : 0,
              (plan & SA_PLAN_NO_BANKS) ? 0 : 1);
  return 0;
}

// The packed tables of k_sec4 / k_sec44 (Shape::pack_inv, pack_fwd): built from
// inv and fwd2 as build_tables does, unpacked again, compared entry for entry
static int cmd_packed(int L, int M, int n, int prec, int plan) {
  Shape s;
  if (shape_of(s, L, M, n, SA_BACKEND_HADAMARD, prec, plan, Shape().n_cus)) return 1;
  size_t invp_bytes = 0, fwd2p_bytes = 0;
  if (s.pack_inv || s.pack_fwd) {
    std::vector<uint32_t> ord((size_t)L * n), all(s.w - 1);
    for (int l = 0; l < L; ++l) {
      std::mt19937 rng(0x0d0000u + (uint32_t)l);
      std::iota(all.begin(), all.end(), 1u);
      std::shuffle(all.begin(), all.end(), rng);
      std::copy(all.begin(), all.begin() + n, ord.begin() + (size_t)l * n);
    }
    std::vector<uint16_t> inv((size_t)L * s.w, (uint16_t)n), fwd((size_t)fwd_groups(L) * n * kSpw, 0);
    std::vector<uint32_t> fwd2((size_t)s.G2 * n, 0);
    for (int l = 0; l < L; ++l) {
      std::string bad;
      CHECK(inv_row(ord.data() + (size_t)l * n, l, n, s.w, inv.data() + (size_t)l * s.w, bad), "inv_row: %s", bad.c_str());
      fwd_section(ord.data() + (size_t)l * n, l, n, s.M, fwd.data(), fwd2.data(), nullptr);
    }
    if (s.pack_inv) {
      const int kh = s.pack_kh, EQ = s.M / 256, rd = pack_rd(EQ, kh);
      CHECK(EQ >= 1 && EQ <= 2 && n <= kPackMaxN, "packed bucket records at M = %d, n = %d", s.M, n);
      const size_t per = pack_inv_section_dwords(s.M, s.nhi, kh);
      CHECK(per == (size_t)4 * ((s.nhi + kh - 1) / kh) * 64 * rd, "section size");
      // a wave's block: every dword of every record has a place of its own
      std::vector<int> seen((size_t)64 * rd, 0);
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < rd; ++j) {
          const unsigned pos = pack_dword_pos(rd, lane, j);
          CHECK(pos < (unsigned)(64 * rd) && !seen[pos]++, "pack_dword_pos(%d, %d, %d) = %u", rd, lane, j, pos);
        }
      std::vector<uint32_t> invp((size_t)L * per, 0);
      for (int l = 0; l < L; ++l) pack_inv_section(s.M, n, s.nhi, kh, inv.data() + (size_t)l * s.w, invp.data() + (size_t)l * per);
      for (int l = 0; l < L; ++l)
        for (int h = 0; h < s.nhi; ++h)
          for (int col = 0; col < s.M; ++col) {
            const uint32_t got = pack_inv_get(s.M, s.nhi, kh, invp.data() + (size_t)l * per, h, col);
            CHECK(got == inv[(size_t)l * s.w + (size_t)h * s.M + col], "invp[%d] step %d column %d = %u, inv has %u", l, h, col,
                  got, (unsigned)inv[(size_t)l * s.w + (size_t)h * s.M + col]);
          }
      // steps past nhi in the last block hold the zero slot
      for (int l = 0; l < L; ++l)
        for (int h = s.nhi; h < (s.nhi + kh - 1) / kh * kh; ++h)
          for (int col = 0; col < s.M; ++col)
            CHECK(pack_inv_get(s.M, s.nhi, kh, invp.data() + (size_t)l * per, h, col) == (uint32_t)n,
                  "invp[%d] step %d (past nhi) column %d is not the zero slot", l, h, col);
      invp_bytes = invp.size() * 4;
    }
    if (s.pack_fwd) {
      CHECK(s.M <= 512 && !s.sec4q, "packed pair table at M = %d, quads %d", s.M, s.sec4q ? 1 : 0);
      const int words = pack_fwd_words(n);
      const size_t per = (size_t)words * kPackNT;
      std::vector<uint64_t> fwd2p((size_t)s.G2 * per, 0);
      for (int g = 0; g < s.G2; ++g) pack_fwd_pair(n, fwd2.data() + (size_t)g * n, fwd2p.data() + (size_t)g * per);
      for (int g = 0; g < s.G2; ++g)
        for (int r = 0; r < words * 3 * kPackNT; ++r) {  // rows past n: row 0's entry
          const uint32_t want = fwd2[(size_t)g * n + (r < n ? r : 0)], got = pack_fwd_get(fwd2p.data() + (size_t)g * per, r);
          CHECK(got == want, "fwd2p[%d] row %d = %#x, fwd2 has %#x", g, r, got, want);
        }
      for (uint64_t wv : fwd2p) CHECK((wv >> 60) == 0, "fwd2p: bits past the three fields");
      fwd2p_bytes = fwd2p.size() * 8;
    }
  }
  std::printf("{\"ok\": 1, \"M\": %d, \"n\": %d, \"nhi\": %d, \"pack_inv\": %d, \"pack_fwd\": %d, \"kh\": %d, \"rd\": %d, "
              "\"blocks\": %d, \"words\": %d, \"inv_bytes\": %zu, \"invp_bytes\": %zu, \"fwd2_bytes\": %zu, \"fwd2p_bytes\": %zu}\n",
              s.M, n, s.nhi, s.pack_inv ? 1 : 0, s.pack_fwd ? 1 : 0, s.pack_kh,
              s.pack_inv ? pack_rd(s.M / 256, s.pack_kh) : 0, s.pack_inv ? (s.nhi + s.pack_kh - 1) / s.pack_kh : 0,
              s.pack_fwd ? pack_fwd_words(n) : 0, (size_t)L * s.w * 2, invp_bytes, (size_t)s.G2 * n * 4, fwd2p_bytes);
  return 0;
}

// The coupled design's layout (sa_sc.h), its invariants, and the padded groups' Ab table
static int cmd_sc(int L, int M, int n, int prec, int R, int C, const std::vector<double>& W) {
  ScLayout s;
  std::string err;
  if (int rc = sc_layout(s, L, M, n, prec, R, C, W.data(), err)) {
    std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
    return 0;
  }
  const std::string bad = sc_check_layout(s);
  CHECK(bad.empty(), "%s", bad.c_str());
  std::vector<uint32_t> ord((size_t)L * n), all(s.w - 1);
  for (int l = 0; l < L; ++l) {
    std::mt19937 rng(0x0d0000u + (uint32_t)l);
    std::iota(all.begin(), all.end(), 1u);
    std::shuffle(all.begin(), all.end(), rng);
    std::copy(all.begin(), all.begin() + n, ord.begin() + (size_t)l * n);
  }
  std::vector<uint16_t> fwd((size_t)s.G * n * kSpw, 0xffffu);
  sc_fwd_table(s, ord.data(), fwd.data());
  const int lgM = ilog2(M);
  for (int g = 0; g < s.G; ++g)
    for (int wv = 0; wv < kSpw; ++wv) {
      const int l = sc_group_section(s, g, wv);
      for (int r = 0; r < n; ++r) {
        const uint16_t e = fwd[((size_t)g * n + r) * kSpw + wv];
        const uint16_t want = l < 0 ? (uint16_t)0 : fwd_entry(ord[(size_t)l * n + r], lgM, M);
        CHECK(e == want && (e & 0x7fffu) < (unsigned)M, "sc fwd[%d][%d][%d] = %#x, expected %#x", g, r, wv, e, want);
      }
    }
  if (!s.own_fwd) {  // the groups are the parent's: group g holds sections 4 g .. 4 g + 3
    for (int g = 0; g < s.G; ++g)
      for (int wv = 0; wv < kSpw; ++wv)
        CHECK(sc_group_section(s, g, wv) == g * kSpw + wv, "group %d is not the parent's", g);
  }
  std::printf("{\"R\": %d, \"C\": %d, \"L\": %d, \"M\": %d, \"n\": %d, \"n_r\": %d, \"L_c\": %d, \"gpc\": %d, \"G\": %d, "
              "\"zpb\": %d, \"NZ\": %d, \"own_fwd\": %d, \"w\": %d, \"nhi\": %d, \"E\": %d, \"sec_lds\": %zu, "
              "\"lds_limit\": %zu, \"max_blocks\": %d, \"groups\": [",
              s.R, s.C, s.L, s.M, s.n, s.n_r, s.L_c, s.gpc, s.G, s.zpb, s.NZ, s.own_fwd ? 1 : 0, s.w, s.nhi, s.E, s.sec_lds,
              kLdsBytes, kScMaxBlocks);
  for (int g = 0; g < s.G; ++g) {
    int cnt = 0;
    for (int wv = 0; wv < kSpw; ++wv) cnt += sc_group_section(s, g, wv) >= 0;
    std::printf("%s[%d, %d, %d]", g ? ", " : "", sc_group_block(s, g), sc_group_section(s, g, 0), cnt);
  }
  std::printf("], \"zparts\": [");
  for (int q = 0; q < s.NZ; ++q)
    std::printf("%s[%d, %d, %d]", q ? ", " : "", sc_zpart_block(s, q), sc_zpart_row0(s, q), sc_zpart_rows(s, q));
  std::printf("]}\n");
  return 0;
}

// The plan of a coupled decode with tolerances (sa_sc.h: sc_wave_plan) and the wave form's invariants
static int cmd_scwave(int L, int M, int n, int prec, int R, int C, int B, int T, double stop_tol, double freeze_tol,
                      bool want_live, const std::vector<double>& W) {
  ScLayout s;
  ScWavePlan p;
  std::string err;
  int rc = sc_layout(s, L, M, n, prec, R, C, W.data(), err);
  if (!rc) rc = sc_wave_plan(p, s, B, T, stop_tol, freeze_tol, want_live, err);
  if (rc) {
    std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
    return 0;
  }
  std::string bad = sc_check_layout(s);
  CHECK(bad.empty(), "%s", bad.c_str());
  bad = sc_check_wave(s, B, T);
  CHECK(bad.empty(), "%s", bad.c_str());
  CHECK(p.wave || (p.taul_bytes == 0 && p.live_bytes == 0 && !p.late_loads), "a decode without tolerances has extra workspace");
  std::printf("{\"wave\": %d, \"instance\": \"%s<%s, %d>\", \"E\": %d, \"stop_tol\": %.17g, \"freeze_tol\": %.17g, "
              "\"late_loads\": %d, \"grid\": [%d, %d], \"block\": 256, \"sec_lds\": %zu, \"lds_limit\": %zu, "
              "\"taul_bytes\": %zu, \"live_bytes\": %zu, \"R\": %d, \"C\": %d, \"G\": %d, \"gpc\": %d}\n",
              p.wave ? 1 : 0, p.wave ? "k_scsec_wave" : "k_scsec", prec == SA_PREC_F64 ? "f64" : "f32", s.E, s.E, p.stop_tol,
              p.freeze_tol, p.late_loads ? 1 : 0, s.G, B, s.sec_lds, kLdsBytes, p.taul_bytes, p.live_bytes, s.R, s.C, s.G,
              s.gpc);
  return 0;
}

// The staged coupled context and the glue on it (sa_sc.h): the section-range check, the
// launch list of a decode with or without a beta_0, the extra workspace, and the state rule walked over `calls`
// (reserve sizes the workspace to B; every other call is made with B codewords, `runbig` with B + 1)
static int cmd_scjoint(int L, int M, int n, int prec, int R, int C, int B, int T, int l0, int ns, bool beta0,
                       double stop_tol, double freeze_tol, const std::vector<double>& W,
                       const std::vector<std::string>& calls) {
  ScLayout s;
  ScWavePlan p;
  std::string err;
  int rc = sc_layout(s, L, M, n, prec, R, C, W.data(), err);
  if (!rc) rc = sc_glue_check(s, l0, ns, err);
  if (!rc) rc = sc_wave_plan(p, s, B, T, stop_tol, freeze_tol, false, err);
  if (rc) {
    std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
    return 0;
  }
  const std::string bad = sc_check_layout(s);
  CHECK(bad.empty(), "%s", bad.c_str());
  const std::vector<ScLaunch> with = sc_decode_launches(T, beta0, p), plain = sc_decode_launches(T, false, p);
  // a beta_0 changes the head of the list alone: the loop's launches are the decode's without one
  CHECK(with.size() == plain.size() + (beta0 ? 1 : 0), "launch list lengths %zu, %zu", with.size(), plain.size());
  for (int k = 1; k <= 2 * T; ++k) {
    const ScLaunch &a = with[with.size() - k], &b = plain[plain.size() - k];
    CHECK(a.step == b.step && a.t == b.t, "loop launch %d from the end differs", k);
  }
  // k_scstart's grid is k_scrow's: every row of every z^2 partial inside [0, n)
  for (int q = 0; q < s.NZ; ++q)
    CHECK(sc_zpart_row0(s, q) >= 0 && sc_zpart_row0(s, q) + sc_zpart_rows(s, q) <= s.n, "z^2 partial %d out of range", q);
  std::printf("{\"l0\": %d, \"ns\": %d, \"lgM\": %d, \"rescale\": %d, \"l0_block\": %d, \"l0_on_block_edge\": %d, "
              "\"cd_bytes\": %zu, \"glue_stage_bytes\": %zu, \"start_grid\": [%d, %d], \"start_block\": 64, "
              "\"n_r\": %d, \"L_c\": %d, \"zpb\": %d, \"own_fwd\": %d, \"launches\": [",
              l0, ns, ilog2(M), ns < L ? 1 : 0, sc_col_block(s, l0), l0 % s.L_c == 0 ? 1 : 0, sc_cd_bytes(s),
              sc_glue_stage_bytes(s, B, ns), s.NZ, B, s.n_r, s.L_c, s.zpb, s.own_fwd ? 1 : 0);
  for (size_t k = 0; k < with.size(); ++k) std::printf("%s\"%s\"", k ? ", " : "", sc_step_name(with[k].step));
  std::printf("], \"walk\": [");
  static const struct { const char* name; int call; } kCalls[] = {
      {"resize", SC_CALL_RESIZE}, {"onecall", SC_CALL_ONE_CALL}, {"power", SC_CALL_STAGE_POWER}, {"stage", SC_CALL_STAGE},
      {"stage0", SC_CALL_STAGE_BETA0}, {"encode", SC_CALL_ENCODE}, {"run", SC_CALL_RUN}, {"run0", SC_CALL_RUN_BETA0},
      {"fetch", SC_CALL_FETCH}, {"llr", SC_CALL_LLR}, {"hard", SC_CALL_HARD}, {"soft", SC_CALL_SOFT_BETA0},
      {"onehot", SC_CALL_ONEHOT}, {"runbig", SC_CALL_RUN}};
  ScStageState st;
  int Bcap = 0;
  for (size_t k = 0; k < calls.size(); ++k) {
    int call = -1;
    for (const auto& c : kCalls)
      if (calls[k] == c.name) call = c.call;
    std::string msg;
    int r = SA_OK;
    if (calls[k] == "reserve") {  // sc_workspace: grown, never shrunk; a reallocation drops the stage
      if (B > Bcap) {
        Bcap = B;
        sc_stage_rule(st, SC_CALL_RESIZE, 0, 0, msg);
      }
    } else {
      CHECK(call >= 0, "unknown call %s", calls[k].c_str());
      const ScStageState before = st;
      r = sc_stage_rule(st, call, calls[k] == "runbig" ? B + 1 : B, Bcap, msg);
      CHECK(r == SA_OK || (st.power == before.power && st.y == before.y && st.beta == before.beta && st.B == before.B),
            "a refused %s changed the state", calls[k].c_str());
    }
    std::printf("%s[\"%s\", %d, \"%s\", %d, %d, %d, %d]", k ? ", " : "", calls[k].c_str(), r, msg.c_str(), st.power ? 1 : 0,
                st.y ? 1 : 0, st.beta ? 1 : 0, st.B);
  }
  std::printf("]}\n");
  return 0;
}

// The plan of a coupled state-evolution batch (sa_scse.h) and its invariants
template <typename T>
static void print_list(const char* name, const std::vector<T>& v, const char* fmt, bool last = false) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) std::printf(", ");
    std::printf(fmt, v[i]);
  }
  std::printf(last ? "]" : "], ");
}

static int cmd_scse(int B, int L, int M, int T, int S, const std::vector<int>& n, const std::vector<int>& R,
                    const std::vector<int>& C, const std::vector<double>& sigma, const std::vector<double>& W,
                    const std::vector<double>& Pl) {
  ScSePlan p;
  std::string err;
  if (int rc = scse_plan(p, B, L, M, n.data(), R.data(), C.data(), W.data(), Pl.data(), sigma.data(), T, S, err)) {
    std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
    return 0;
  }
  const std::string bad = scse_check_plan(p, Pl.data());
  CHECK(bad.empty(), "%s", bad.c_str());
  std::printf("{\"B\": %d, \"L\": %d, \"M\": %d, \"K\": %d, \"NS\": %d, \"NR\": %d, \"Rmax\": %d, \"Cmax\": %d, "
              "\"SC\": %d, \"NCH\": %d, \"grid\": %lld, \"classes_per_group\": %d, \"max_blocks\": %d, \"max_M\": %d, ",
              p.B, p.L, p.M, p.K, p.NS, p.NR, p.Rmax, p.Cmax, p.SC, p.NCH, p.grid, kSeClasses, kScSeMaxBlocks, kSeMaxM);
  print_list("slot_off", p.slot_off, "%d");
  print_list("row_off", p.row_off, "%d");
  print_list("w_off", p.w_off, "%lld");
  print_list("cfg_off", p.cfg_off, "%d");
  print_list("blk_off", p.blk_off, "%d");
  print_list("sec_cls", p.sec_cls, "%d");
  print_list("Pc", p.Pc, "%.17g");
  print_list("sig2", p.sig2, "%.17g");
  print_list("phi0", p.phi0, "%.17g");
  print_list("tau20", p.tau20, "%.17g");
  std::printf("\"classes\": [");
  for (int k = 0; k < p.K; ++k)
    std::printf("%s[%d, %.17g, %.17g, %d]", k ? ", " : "", p.cls_slot[k], p.cls_c[k], p.cls_w[k], p.cls_mult[k]);
  std::printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  if (!std::strcmp(argv[1], "scse")) {
    if (argc < 7) return usage();
    int v[5];
    for (int i = 0; i < 5; ++i) v[i] = std::atoi(argv[2 + i]);
    const int B = v[0], L = v[1];
    std::vector<int> n, R, C;
    std::vector<double> sigma, W, Pl;
    int at = 7;
    // (a list that ends early: refused here, in front of scse_plan's reads)
    for (int b = 0; b < B; ++b) {
      if (at + 4 > argc) return usage();
      n.push_back(std::atoi(argv[at]));
      R.push_back(std::atoi(argv[at + 1]));
      C.push_back(std::atoi(argv[at + 2]));
      sigma.push_back(std::strtod(argv[at + 3], nullptr));
      at += 4;
      const long long nw = (long long)std::max(R[b], 0) * std::max(C[b], 0), np = std::max(L, 0);
      if (at + nw + np > argc) return usage();
      for (long long i = 0; i < nw; ++i) W.push_back(std::strtod(argv[at++], nullptr));
      for (long long i = 0; i < np; ++i) Pl.push_back(std::strtod(argv[at++], nullptr));
    }
    if (at != argc) return usage();
    // (scse_plan reads nothing of a configuration it refuses at R or C < 1; the lists are never empty for its reads)
    W.push_back(0.0);
    Pl.push_back(0.0);
    return cmd_scse(B, L, v[2], v[3], v[4], n, R, C, sigma, W, Pl);
  }
  if (!std::strcmp(argv[1], "scjoint")) {
    if (argc < 15) return usage();
    int v[11];
    for (int i = 0; i < 11; ++i) v[i] = std::atoi(argv[2 + i]);
    const double st = std::strtod(argv[13], nullptr), ft = std::strtod(argv[14], nullptr);
    if (v[4] < 1 || v[5] < 1 || 15 + (long long)v[4] * v[5] > argc) return usage();
    const int nw = v[4] * v[5];
    std::vector<double> W;
    for (int i = 15; i < 15 + nw; ++i) W.push_back(std::strtod(argv[i], nullptr));
    std::vector<std::string> calls(argv + 15 + nw, argv + argc);
    return cmd_scjoint(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10] != 0, st, ft, W, calls);
  }
  if (!std::strcmp(argv[1], "scwave")) {
    if (argc < 13) return usage();
    int v[8];
    for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[2 + i]);
    const double st = std::strtod(argv[10], nullptr), ft = std::strtod(argv[11], nullptr);
    const bool want_live = std::atoi(argv[12]) != 0;
    std::vector<double> W;
    for (int i = 13; i < argc; ++i) W.push_back(std::strtod(argv[i], nullptr));
    if (v[4] < 1 || v[5] < 1 || (long long)v[4] * v[5] != (long long)W.size()) return usage();
    return cmd_scwave(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], st, ft, want_live, W);
  }
  if (!std::strcmp(argv[1], "sc")) {
    if (argc < 8) return usage();
    int v[6];
    for (int i = 0; i < 6; ++i) v[i] = std::atoi(argv[2 + i]);
    std::vector<double> W;
    for (int i = 8; i < argc; ++i) W.push_back(std::strtod(argv[i], nullptr));
    // (a count that is not R x C: refused here, in front of sc_layout's reads)
    if (v[4] >= 1 && v[5] >= 1 && (long long)v[4] * v[5] != (long long)W.size()) return usage();
    return cmd_sc(v[0], v[1], v[2], v[3], v[4], v[5], W);
  }
  std::vector<int> a;
  for (int i = 2; i < argc; ++i) a.push_back(std::atoi(argv[i]));
  if (!std::strcmp(argv[1], "shape") && a.size() == 8) return cmd_shape(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  if (!std::strcmp(argv[1], "sweep") && a.size() == 9)
    return cmd_sweep(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
  if (!std::strcmp(argv[1], "seq") && a.size() == 12) return cmd_seq(a);
  if (!std::strcmp(argv[1], "tables") && a.size() == 5) return cmd_tables(a[0], a[1], a[2], a[3], a[4]);
  if (!std::strcmp(argv[1], "packed") && a.size() == 5) return cmd_packed(a[0], a[1], a[2], a[3], a[4]);
  return usage();
}
