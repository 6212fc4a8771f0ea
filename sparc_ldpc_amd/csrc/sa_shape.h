// sa_shape.h — the operator's shape rules as pure host code: everything
// (L, M, n, backend, precision, plan options, CUs) decides about an operator
// (Shape, shape_for) and about a decode of B codewords on it (Plan, plan_for).
// No HIP include: csrc/sa_host_check.cpp runs these rules on a machine without
// a GPU.  sa_ctx (sa_host.h) is a Shape; the kernel units read its fields.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "sparc_amp.h"

namespace sa {

// ---- operator constants --------------------------------------------------
constexpr int kSpw = 4;          // sections (wavefronts) per section-kernel workgroup
constexpr int kRowsPerBlk = 64;  // rows per row-kernel workgroup (one per lane)
constexpr int kRow2Rows = 32;    // k_row2: one 128-B line of a partial per row block
constexpr int kSG = 16;          // fwd table padding (sections)
// table bytes of the section groups one XCD works on at a time (SecArgs::gpx).
// C4 binary32 k_secb HBM bytes per launch (PMC, round 4; the 1.7 / 0.9 MB
// points on an intermediate build with an L2-budget switch since removed):
// one pass (6 groups, 4.7 MB) 1.715 GB; 2.5 MB -> 2 x 3 groups 1.495 GB;
// 1.7 MB -> 3 x 2 groups 1.514 GB; 0.9 MB -> 6 x 1 group 1.711 GB (every
// pass re-reads z)
constexpr size_t kSecbL2 = (size_t)5 << 19;  // 2.5 MB of the 4 MB L2
// sections (waves) per batched workgroup: 8 (two workgroups per CU), or 16
// (one per CU) where the wider workgroup's LDS holds a larger codeword chunk
// (Shape::WB, chosen at context creation)
constexpr int kWB = 8, kWB16 = 16;
// zero rows after z in the batched kernel's LDS image (empty bucket slots read
// them; 16, one per 16-byte bank group: banked_section)
constexpr int kInvbZeroRows = 16;
// k_secb's bucket h-steps with table loads in flight per block (binary32 at
// CB = 4 or E = 16 / binary64); the bank-aware table (ensure_invb) pads each
// half's occupied steps to a multiple of it
constexpr int kSecbKH32 = 2, kSecbKH64 = 2;
// the LDS of a CU: what a section kernel's image may take
constexpr size_t kLdsBytes = 160 * 1024;

// ---- packed tables of the pair / quad section kernels (k_sec4, k_sec44) -----
// Bucket table: an entry is a row index 0 .. n (n: the zero slot), 13 bits
// while n + 1 < 8192.  One record per (section, quarter q, lane, block of KH
// bucket steps) holds the lane's EQ * KH entries (element-major inside a step,
// steps in h order; steps past nhi hold n) as one little-endian bit string,
// padded to whole dwords.  The 64 records of a wave's block are contiguous and
// laid out for the wave's loads: dwords 0 .. 4 nv - 1 of a record as nv 16-byte
// pieces [piece][lane], the rest dword-interleaved [dword][lane], so that every
// load instruction reads one contiguous run (pack_dword_pos).
constexpr int kPackBits = 13;
constexpr int kPackMaxN = (1 << kPackBits) - 2;                                      // n + 1 < 8192
constexpr int pack_rd(int EQ, int KH) { return (EQ * KH * kPackBits + 31) / 32; }   // dwords of a record
// dword of a wave's block (64 records of rd dwords) that holds dword j of lane's record
constexpr unsigned pack_dword_pos(int rd, int lane, int j) {
  return j < rd / 4 * 4 ? (unsigned)((j / 4) * 256 + lane * 4 + j % 4)
                        : (unsigned)(rd / 4 * 256 + (j - rd / 4 * 4) * 64 + lane);
}
// Pair Ab table: one 64-bit word per three rows of a thread of the pair
// kernel's row phase (512 threads, passes of kPackRows rows): word
// [pair][j][tid] holds rows (3 j + f) 512 + tid, f = 0, 1, 2, as 20-bit
// fields k0 | s0 << 9 | k1 << 10 | s1 << 19 (M <= 512); a row past n holds
// row 0's entry
constexpr int kPackNT = 512, kPackKR = 9, kPackRows = kPackNT * kPackKR;
constexpr int pack_fwd_words(int n) { return (n + kPackRows - 1) / kPackRows * (kPackKR / 3); }  // per thread and pair

inline int ilog2(int x) {
  int r = 0;
  while ((1 << r) < x) ++r;
  return r;
}

// ---- the shape of an operator ----------------------------------------------
struct Shape {
  // what the caller asked for
  int L = 0, n = 0, backend = 0, prec = 0;
  int plan = 0;     // SA_PLAN_* options of sa_create_ex (0: every choice by the built-in rules)
  int n_cus = 256;  // compute units of the device
  // the section: M columns on the device.  The caller's section size is Mu;
  // the Hadamard backend pads a section of any Mu to M = 2^ceil(log2 Mu)
  // columns, the first dead = M - Mu of them never used (column c of the
  // reference is column dead + c: sparc_ldpc.py:54, 68)
  int M = 0, Mu = 0, dead = 0;
  bool pow2 = true;  // Mu a power of two (the Hadamard kernels, bit-level glue)
  // the transform: length w = 2^ceil(log2(max(M+1, n+1))), nhi = w / M bucket
  // steps, E elements per lane of a one-wave section
  int w = 0, nhi = 0, E = 1;
  // operators whose z does not fit the section kernels' LDS (n >= 65535, or
  // the z image past 160 KB): k_secg with 32-bit bucket entries, no batched /
  // multi-wave kernels
  bool big = false;
  // row kernels: blocks per codeword of k_row (64 rows), k_row2 (32, and 16
  // where row16), k_rowv<4> (256) and k_rowv<2> / k_rowc (128)
  int NZ = 0, NZ16 = 0, NZh = 0, NZ4 = 0, NZ2 = 0;
  bool row16 = false;  // k_row2<16> after k_sec4 (row-block-major partials, NZh <= 320)
  bool pt_on = false;  // row-block-major Ab partials between k_sec4 / k_sec43 and k_row2 (SecArgs::pt)
  // one-codeword section kernels: workgroups per codeword and LDS bytes
  int G = 0;           // k_sec / k_secg groups of 4 sections
  size_t sec_lds = 0;
  int G2 = 0;          // k_sec2 / k_sec4 pairs of sections (0: unavailable)
  size_t sec2_lds = 0;
  bool sec4 = false;   // k_sec4 (4 waves per section) fits and is chosen
  size_t sec4_lds = 0;
  int G3 = 0;          // k_sec43 triples of sections (used when sec3)
  bool sec3 = false;   // k_sec43 (three sections x 4 waves per workgroup) chosen over k_sec4
  size_t sec3_lds = 0;
  int G4 = 0;          // k_sec44 quads of sections (used when sec4q)
  bool sec4q = false;  // k_sec44 (four sections x 4 waves per workgroup, the pair table) chosen over k_sec4
  size_t sec4q_lds = 0;
  // packed tables of k_sec4 / k_sec44 (n <= kPackMaxN, M <= 512; SA_PLAN_NO_PACK)
  bool pack_inv = false;  // 13-bit bucket records (Tables::invp) in blocks of pack_kh steps
  bool pack_fwd = false;  // three rows per 64-bit word of the pair Ab table (Tables::fwd2p); pairs only
  int pack_kh = 0;        // the kernel's bucket steps per block (secq_body's KH)
  // batched kernel k_secb
  int WB = 8;          // sections per workgroup (kWB or kWB16)
  int CB = 0;          // codewords per workgroup (0 = off)
  int Gb = 0;          // groups of WB sections
  int gpx = 1 << 20;   // section groups per XCD per pass (SecArgs::gpx)
  size_t secb_lds = 0;
  int Gd = 0;          // dense backends: denoiser groups
};

inline size_t rsz(const Shape* s) { return s->prec == SA_PREC_F64 ? 8 : 4; }

// ---- LDS bytes of each section kernel's image (s: bytes per real) -----------
// z slots (n rows and the zero slot), rounded to 16 bytes
inline size_t zbytes(int n, size_t s) { return ((size_t)(n + 1) * s + 15) / 16 * 16; }
// k_sec: z slots + 4 sections x M + 4 beta^2 partials (k_secg: no z)
inline size_t sec_lds_need(int M, int n, size_t s, bool z) {
  return (z ? zbytes(n, s) : 0) + (size_t)kSpw * M * s + (size_t)kSpw * s;
}
// k_sec2: z + 2 sections' T + top-bit exchange + reductions
inline size_t sec2_need(int M, int n, size_t s) {
  return zbytes(n, s) + 2 * (size_t)M * s + 4 * (size_t)(M / 2) * s + 16 * s;
}
// k_sec4: z + 2 sections' T + one exchange image per section + reductions
inline size_t sec4_need(int M, int n, size_t s) { return zbytes(n, s) + 4 * (size_t)M * s + 32 * s; }
// k_sec43: the same for three sections
inline size_t sec43_need(int M, int n, size_t s) { return zbytes(n, s) + 6 * (size_t)M * s + 48 * s; }
// k_sec44: z + 4 sections' T + one exchange image per section + reductions
inline size_t sec44_need(int M, int n, size_t s) { return zbytes(n, s) + 8 * (size_t)M * s + 64 * s; }
// k_secb with W sections and cb codewords per workgroup: z (with its zero
// rows) and T share one region
inline size_t secb_need(int W, int cb, int M, int n, size_t s) {
  const size_t zb = (((size_t)(n + kInvbZeroRows) * cb * s) + 15) / 16 * 16;
  const size_t tb = (size_t)W * M * cb * s;
  return (zb > tb ? zb : tb) + (size_t)W * cb * s + (s == 8 ? 64 * 8 : 0);
}
// what a k_secb workgroup may take: half of the LDS, so that two 8-section
// workgroups share a CU; all of it for one codeword or 16 sections
inline size_t secb_limit(int W, int cb) { return cb == 1 || W > kWB ? kLdsBytes : kLdsBytes / 2; }

// The limits of a shape no backend passes (checked in front of shape_for).
inline int shape_limits(int M, int n, int backend, std::string& err) {
  if (M > 4096) {
    err = "M must be <= 4096";
    return SA_ERR_UNSUPPORTED;
  }
  // the Hadamard operator takes n past 16-bit row indices (k_secg); the
  // materialised designs and the host-operator loop keep the 16-bit limit
  if (n >= (backend == SA_BACKEND_HADAMARD ? (1 << 24) : 65535)) {
    err = backend == SA_BACKEND_HADAMARD ? "n must be < 2^24" : "n must be < 65535";
    return SA_ERR_UNSUPPORTED;
  }
  return SA_OK;
}

// Every shape number of an operator of L sections of M columns and n rows
// (valid arguments within shape_limits) on a device of n_cus compute units.
// SA_OK, or SA_ERR_UNSUPPORTED with the reason in err.
inline int shape_for(Shape& c, int L, int M, int n, int backend, int prec, int plan, int n_cus, std::string& err) {
  c = Shape();
  c.L = L; c.M = M; c.n = n; c.backend = backend; c.prec = prec; c.plan = plan; c.n_cus = n_cus;
  c.Mu = M;
  const bool pow2 = (M & (M - 1)) == 0;
  const int mx = (M + 1) > (n + 1) ? (M + 1) : (n + 1);
  c.w = 1 << ilog2(mx);  // 2^ceil(log2(max(M+1, n+1))), sparc_ldpc.py:52/:110
  if (!pow2 && backend == SA_BACKEND_HADAMARD) {
    // any M on the matrix-free operator: the reference keeps the last M of the
    // w columns (sparc_ldpc.py:68/:77), which are the last M of the last
    // Mp = 2^ceil(log2 M) <= w, whose high index bits are all ones: a section
    // is a padded section of Mp columns whose first Mp - M never carry an
    // estimate (the denoiser excludes them, beta stays 0 there); the caller's
    // beta / A^T z move in and out of the padded layout at the boundary
    c.M = 1 << ilog2(M);
    c.dead = c.M - M;
    M = c.M;
  }
  c.nhi = c.w / M;
  c.E = 1;  // elements per lane of a one-wave section: the power of two covering M
  while (c.E * 64 < M) c.E *= 2;
  c.pow2 = pow2;
  c.NZ = (n + kRowsPerBlk - 1) / kRowsPerBlk;
  c.NZ16 = (n + kRow2Rows - 1) / kRow2Rows;
  c.NZh = (n + 15) / 16;
  c.NZ4 = (n + 255) / 256;
  c.NZ2 = (n + 127) / 128;
  const size_t s = rsz(&c);
  c.sec_lds = sec_lds_need(M, n, s, true);
  if (backend == SA_BACKEND_HADAMARD && (n >= 65535 || c.sec_lds > kLdsBytes)) {
    // z from global memory, 32-bit bucket entries (k_secg); the multi-wave and
    // batched kernels' LDS images need z too: they stay off (G2, CB below)
    c.big = true;
    c.sec_lds = sec_lds_need(M, n, s, false);
  }
  if (c.dead > 0 && c.big) {
    err = "M not a power of two: the Hadamard operator keeps z in LDS (n < 65535 and "
          "the z image within 160 KB)";
    return SA_ERR_UNSUPPORTED;
  }
  if (c.sec_lds > kLdsBytes) {
    err = "section kernel does not fit in LDS (n and M too large for this precision)";
    return SA_ERR_UNSUPPORTED;
  }
  c.G = (L + kSpw - 1) / kSpw;
  // (a padded section runs on k_sec alone, the one section kernel that masks dead columns)
  if (M >= 128 && M <= 4096 && !c.big && c.dead == 0) {
    if (sec2_need(M, n, s) <= kLdsBytes) {
      c.G2 = (L + 1) / 2;
      c.sec2_lds = sec2_need(M, n, s);
    }
    if (c.G2 > 0 && M >= 256 && sec4_need(M, n, s) <= kLdsBytes) {
      c.sec4 = true;
      c.sec4_lds = sec4_need(M, n, s);
    }
    // row-block-major Ab partials for k_row2 (SA_PLAN_NO_PT: the [G][n] layout):
    // each k_row2 workgroup reads one contiguous G x 128-B block instead of G
    // lines n rows apart.  C4 single codeword 880 -> 950 cw/s (k_row2 4.1 ->
    // 3.4 us, two interleaved A/B rounds); c2 within noise
    c.pt_on = !(plan & SA_PLAN_NO_PT);
    // 16-row k_row2 blocks for one codeword where the z^2 partials still fit
    // the section kernels' registers (ceil(n / 16) <= 320; C2: 288 workgroups
    // instead of 144, every CU pulls partials): c2 1362-1374 -> 1396 cw/s
    // (two interleaved A/B rounds).  Binary32 only: in binary64 the 32-row
    // blocks are faster (c2 fp64 984-988 -> 990-1013 cw/s, two interleaved
    // rounds, round 3).  SA_PLAN_NO_ROW16 / SA_PLAN_ROW16 force 32- / 16-row blocks
    const bool r16 = (plan & SA_PLAN_ROW16) ? true : (plan & SA_PLAN_NO_ROW16) ? false : s == 4;
    c.row16 = r16 && c.pt_on && c.sec4 && c.NZh <= 320;
  }

  // batched kernel: the most codewords per workgroup (CB in {4, 2, 1}; 4 for
  // fp32 only) whose LDS image (z and T share one region) still lets two
  // 8-section workgroups share a CU (CB = 1 takes the whole LDS if it must);
  // one 16-section workgroup per CU instead where its whole-LDS image holds a
  // larger chunk (L = 768, n = 8294: CB 4 instead of 2; binary64 2 instead of
  // 1), and also at equal CB (half the Ab partials: the row kernel's HBM read
  // halves, the section kernel pays a 16-wave barrier): C4 batch 256 4.45 k
  // -> 5.51 k cw/s (binary64 2.17 k -> 2.41 k), C3 11.10 k -> 11.26 k; in
  // binary64 at equal CB since round 4 (C3 fp64 with ZIL 6.44 k -> 7.02 k,
  // the joint configs[4] step 1.65 k -> 1.75 k).  SA_PLAN_WB8 / WB16 force it.
  {
    auto cb_for = [&](int W) {
      if (c.big || c.dead > 0) return 0;
      for (int cb = (s == 4 ? 4 : 2); cb >= 1 && M <= 1024; cb >>= 1)
        if (secb_need(W, cb, M, n, s) <= secb_limit(W, cb)) return cb;
      return 0;
    };
    const int c8 = cb_for(kWB), c16 = cb_for(kWB16);
    const bool w16 = (plan & SA_PLAN_WB16) ? true : (plan & SA_PLAN_WB8) ? false : c16 >= c8;
    c.WB = w16 && c16 > 0 ? kWB16 : kWB;
    c.CB = c.WB == kWB16 ? c16 : c8;
    c.secb_lds = c.CB > 0 ? secb_need(c.WB, c.CB, M, n, s) : 0;
    c.Gb = (L + c.WB - 1) / c.WB;
    // passes over each XCD's section groups so one pass's bucket and Ab
    // tables (W sections x (w + n) x 2 B per group) stay within kSecbL2
    // bytes of the XCD's 4 MB L2 (the rest: z chunks, streamed beta)
    const size_t per_group = (size_t)c.WB * ((size_t)c.w + (size_t)n) * 2;
    const int gx = c.Gb / 8 > 0 ? c.Gb / 8 : 1;
    const int fit = (int)std::max<size_t>(1, kSecbL2 / per_group);
    const int npass = (gx + fit - 1) / fit;
    c.gpx = (gx + npass - 1) / npass;  // balanced passes
    if (plan & SA_PLAN_ONE_PASS) c.gpx = 1 << 20;
  }
  c.Gd = (L + 3) / 4;
  {
    // k_sec43: three sections per workgroup where pairs overfill the chip
    // (ceil(L/2) > CUs >= ceil(L/3), e.g. L = 768) — one workgroup per CU
    // instead of two on half of them; in binary64 also where pairs fill the
    // chip exactly (L = 2 x CUs, c2): a third fewer 8-byte Ab partials for
    // k_row2 outweigh the longer section step (c2 fp64 989-997 -> 1026-1027
    // cw/s, two interleaved A/B rounds, round 3; binary32 at c2: neutral, pairs
    // kept).  SA_PLAN_NO_SEC3 / SA_PLAN_SEC3 force it off / on
    const int G3 = (L + 2) / 3;
    const bool fits = c.sec4 && backend == SA_BACKEND_HADAMARD && M <= 512 && sec43_need(M, n, s) <= kLdsBytes;
    const bool over = c.G2 > c.n_cus || (s == 8 && c.G2 == c.n_cus);
    const bool want = (plan & SA_PLAN_SEC3) ? true : (plan & SA_PLAN_NO_SEC3) ? false : (over && G3 <= c.n_cus);
    if (fits && want) {
      c.sec3 = true;
      c.G3 = G3;
      c.sec3_lds = sec43_need(M, n, s);
    }
    // k_sec44: four sections per workgroup on the pair table.  SA_PLAN_SEC4Q runs it
    // wherever pairs would run (SA_PLAN_SEC3 beside it keeps triples) and is
    // never chosen otherwise.  At c2 (L = 2 x CUs) one launch takes half the
    // CUs, so the section kernels of two decodes in flight (decode lanes) stop
    // sharing CUs, and the Ab partials and z fills halve: +4.2 % to +4.8 % over
    // pairs with lanes (as much as triples), but a lone decode, which leaves
    // the other half of the chip idle, takes 0.74 ms against 0.68 ms (DESIGN.md
    // section 8, "lane shapes"), so it stays an option for throughput callers
    // (M <= 512: the larger sections' instances spill at 128 VGPRs)
    const bool fits4q = c.sec4 && backend == SA_BACKEND_HADAMARD && M <= 512 && sec44_need(M, n, s) <= kLdsBytes;
    if (fits4q && (plan & SA_PLAN_SEC4Q) && !(plan & (SA_PLAN_SEC3 | SA_PLAN_NO_SEC4Q))) {
      c.sec4q = true;
      c.sec3 = false;
      c.G4 = (L + 3) / 4;
      c.sec4q_lds = sec44_need(M, n, s);
    }
    // 32-row k_row2 blocks where pairs fill the chip exactly (L = 2 x CUs,
    // c2): with two decodes in flight every CU already holds a section
    // workgroup of each lane, and the 144 32-row workgroups of a row step
    // disturb them less than 288 16-row ones: c2 +3 % with lanes, every run
    // above every 16-row run, the lone decode inside its run-to-run range
    // ("lane shapes").  SA_PLAN_ROW16
    // keeps 16-row blocks, and so does SA_PLAN_NO_SEC3, which asks for the
    // pair shape as it was (k_sec4 in front of 16-row blocks)
    if (c.G2 == c.n_cus && !(plan & (SA_PLAN_ROW16 | SA_PLAN_NO_SEC3))) c.row16 = false;
    // packed tables where pairs or quads run (triples pack their own Ab table
    // and C4's n needs 14 bits): the tables are over half of the bytes a c2
    // iteration moves, and with two decodes in flight the headline follows
    // the bytes ("packed tables").  Either precision;
    // M <= 512 (EQ <= 2: the 9-bit columns of a field, 13 dwords of a record)
    const bool packable = c.sec4 && !c.sec3 && backend == SA_BACKEND_HADAMARD && M <= 512 && n <= kPackMaxN;
    c.pack_inv = packable && !(plan & SA_PLAN_NO_PACK);
    c.pack_fwd = packable && !c.sec4q && !(plan & SA_PLAN_NO_PACK);
    c.pack_kh = c.sec4q && s == 8 ? 8 : 16;
  }
  return SA_OK;
}

// ---- backend / kernel choice rules of a decode of B codewords ----------------
constexpr int kI8MinB = 4;   // dense backend: batches at least this large take the int8 GEMM path
constexpr int kI8MaxS = 16;  // K splits of the int8 A beta GEMM (its Ab partials)
constexpr int kFMinB = 4;    // matrix backend: batches at least this large take the f32 / f64 GEMM path
constexpr int kFMaxS = 16;   // K splits of its A beta GEMM

// the dense backends: a materialised n x (L*M) matrix streamed by GEMVs
// (the Hadamard design's, or a caller's own: SA_BACKEND_MATRIX)
inline bool is_dense(const Shape& c) { return c.backend == SA_BACKEND_DENSE || c.backend == SA_BACKEND_MATRIX; }
inline bool use_i8(const Shape& c, int B) { return c.backend == SA_BACKEND_DENSE && B >= kI8MinB; }
inline bool use_fgemm(const Shape& c, int B) { return c.backend == SA_BACKEND_MATRIX && B >= kFMinB; }
inline bool use_batched(const Shape& c, int B) { return c.CB > 0 && B >= 4; }

// The batched decode with z and the Ab partials interleaved by codeword chunk
// (SecArgs::zil, 16-byte rows of CB codewords: binary32 CB = 4, binary64
// CB = 2), row kernel k_rowc.  The default in binary32 (C3 +1.7 %, C4
// +4.7 %) and, since the binary64 k_secb no longer spills (round 4: one
// bucket h-step in flight, 16-byte non-temporal beta), in binary64 too (C3
// 6.30 k -> 6.44 k, C4 3.09-3.12 k -> 3.19 k cw/s; round 3's spilling kernel
// lost 1.6 %); SA_PLAN_NO_ZIL keeps [B][n]
inline bool zil_for(const Shape& c, int B) {
  const bool on = (c.plan & SA_PLAN_NO_ZIL) ? false : true;
  return on && c.backend == SA_BACKEND_HADAMARD && use_batched(c, B) && c.CB * (int)rsz(&c) == 16;
}

// Which kernels a decode of B codewords runs, and the counts that follow from
// the choice: everything (context, B) decides, filled by plan_for alone.  An
// entry point that launches decode kernels computes it once and hands it to
// the launchers; nothing of it is kept in the context.
struct Plan {
  sa_sec_path sec = SA_SEC_K_SEC;    // the section path of the iterations
  sa_row_kernel row = SA_ROW_K_ROW;  // the row kernel of the decode (ROW_ABOUT: always k_row)
  int nz = 0;          // z^2 partials per codeword: the row kernel's blocks per codeword
  int G = 0, Gb = 0;   // partials per codeword of the loop's producer of abp (A beta) and bbp (beta^2)
  int pt = 0;          // Ab partials of the loop row-block major (SecArgs::pt): rows per block, 0 for [G][n]
  int rs = 1;          // row splits of a k_sec / k_secg launch (the loop's, the beta0 start's, sa_Ab / sa_Az)
  int CB = 1;          // codewords per k_secb workgroup
  bool zil = false;    // z and the Ab partials codeword-interleaved (zil_for)
  bool dense() const { return sec == SA_SEC_DENSE || sec == SA_SEC_DENSE_I8 || sec == SA_SEC_MATRIX; }
  bool batched() const { return sec == SA_SEC_K_SECB; }
  bool multiwave() const {
    return sec == SA_SEC_K_SEC2 || sec == SA_SEC_K_SEC4 || sec == SA_SEC_K_SEC43 || sec == SA_SEC_K_SEC44;
  }
  // k_row2 launches can carry the iters writes (RowArgs::itset); the small-batch Hadamard decode uses them
  bool row_sets_iters() const { return row == SA_ROW_K_ROW2 || row == SA_ROW_K_ROW2_16; }
  bool it_row() const { return !dense() && !batched() && row_sets_iters(); }
  // k_sec4 / k_sec43 / k_sec44 can take the previous estimate as zero (SecArgs::bzero)
  bool bzero() const { return sec == SA_SEC_K_SEC4 || sec == SA_SEC_K_SEC43 || sec == SA_SEC_K_SEC44; }
};

// Row kernel for B codewords: k_row2 (32-row blocks, 16-row for one codeword
// where row16) while B * ceil(n/64) < 4 CUs, else in binary32 k_rowv<4>
// (n % 4 == 0) or k_rowv<2> (n even) when their blocks cover the CUs twice,
// else k_row (64 rows); k_rowc behind the codeword-interleaved k_secb.
// Section path: the GEMMs / GEMVs of a dense backend; k_secb from 4 codewords;
// a multi-wave kernel (k_sec43 over k_sec44 over k_sec4 over k_sec2) when its workgroups
// fill at least half of the CUs; else k_sec's (k_secg's) row splits.
// dense_G: the Ab partials of a dense backend's A beta, which the context's
// device state decides (sa_host.h: plan_for of a context).
inline Plan plan_for(const Shape& c, int B, int dense_G = 0) {
  Plan p;
  const bool f32 = c.prec == SA_PREC_F32;
  p.zil = zil_for(c, B);
  if (p.zil) {
    p.row = SA_ROW_K_ROWC; p.nz = c.NZ2;  // 128-row blocks
  } else if ((long long)B * c.NZ < 4LL * c.n_cus) {
    if (c.row16 && B == 1) { p.row = SA_ROW_K_ROW2_16; p.nz = c.NZh; }
    else { p.row = SA_ROW_K_ROW2; p.nz = c.NZ16; }
  } else if (c.n % (f32 ? 4 : 2) == 0 && (long long)B * (f32 ? c.NZ4 : c.NZ2) >= 2LL * c.n_cus) {
    // 16-byte rows: binary32 n % 4 == 0 (256-row blocks) or binary64 n even (128)
    p.row = SA_ROW_K_ROWV16; p.nz = f32 ? c.NZ4 : c.NZ2;
  } else if (f32 && c.n % 2 == 0 && (long long)B * c.NZ2 >= 2LL * c.n_cus) {
    p.row = SA_ROW_K_ROWV8; p.nz = c.NZ2;
  } else {
    p.row = SA_ROW_K_ROW; p.nz = c.NZ;
  }
  const int wgs = c.G * B;  // k_sec / k_secg: enough row splits to cover every CU
  p.rs = std::min(4, std::max(1, (c.n_cus + wgs - 1) / wgs));
  if (is_dense(c)) {
    p.sec = use_i8(c, B) ? SA_SEC_DENSE_I8 : (use_fgemm(c, B) ? SA_SEC_MATRIX : SA_SEC_DENSE);
    p.G = dense_G;
    p.Gb = c.Gd;
  } else if (use_batched(c, B)) {
    p.sec = SA_SEC_K_SECB;
    p.G = p.Gb = c.Gb;
    p.CB = c.CB;
  } else if (c.backend == SA_BACKEND_HADAMARD && c.G2 > 0 && c.G2 * B * 2 >= c.n_cus) {
    p.sec = c.sec3 ? SA_SEC_K_SEC43 : (c.sec4q ? SA_SEC_K_SEC44 : (c.sec4 ? SA_SEC_K_SEC4 : SA_SEC_K_SEC2));
    p.G = p.Gb = c.sec3 ? c.G3 : (c.sec4q ? c.G4 : c.G2);  // triples / quads / pairs of sections
    if (p.sec != SA_SEC_K_SEC2 && p.row_sets_iters() && c.pt_on) p.pt = p.row == SA_ROW_K_ROW2_16 ? 16 : kRow2Rows;
  } else {
    p.sec = c.big ? SA_SEC_K_SECG : SA_SEC_K_SEC;
    p.G = p.Gb = c.G;
  }
  return p;
}

// k_secb's XCD-grouped work order (sa_secb.hip computes it per workgroup):
// used when the section groups and the workgroups split evenly over the 8
// XCDs, else one plain pass.  gp: groups per pass; passes: per XCD.
struct SecbOrder {
  int gp, passes;
};
inline SecbOrder secb_order(const Shape& c, int B) {
  const int NC = (B + c.CB - 1) / c.CB;
  const bool xcd = (c.Gb % 8) == 0 && ((long long)c.Gb * NC) % 8 == 0;
  const int gx = xcd ? c.Gb / 8 : c.Gb;
  const int gp = xcd ? std::min(c.gpx, gx) : gx;
  return {gp, (gx + gp - 1) / gp};
}

}  // namespace sa
