// sa_tables.h — the operator tables: the device pointers a context holds
// (Tables) and the pure host algorithms that fill them from an ordering.  No
// HIP include: csrc/sa_host_check.cpp checks the builders' invariants on a
// machine without a GPU.  sa_tables.hip runs them over the sections and
// uploads the results.
#pragma once
#include <cstdint>
#include <random>
#include <vector>

#include "sa_shape.h"

namespace sa {

// The operator tables on the device: built once per operator (the batched
// kernel's at its first use: ensure_invb), read-only during a decode, shared
// with the operator's twins (sa_ctx::borrowed).  A table is declared here,
// freed in tables_free and handed to the kernels in sec_args.
struct Tables {
  uint16_t* inv = nullptr;    // [L][w] bucket table: row of ordering value o, or n (zero slot)
  uint32_t* inv32 = nullptr;  // the same with 32-bit rows (Shape::big: k_secg)
  uint16_t* invb = nullptr;   // k_secb's bank-aware bucket table (banked_section)
  uint16_t* invl = nullptr;   // the codeword-interleaved k_secb's bucket table, lane-major (k_lane_major)
  uint32_t* hs = nullptr;     // [L] occupied steps of invb's halves (banked_section)
  uint16_t* fwd = nullptr;    // [G][n][4] Ab table, 4 sections per entry group (fwd_entry)
  uint16_t* fwdb = nullptr;   // k_secb's Ab table, bank-aware step order per row (fwdb_group)
  uint32_t* fwd2 = nullptr;   // [ceil(L/2)][n] section pairs
  uint32_t* fwd3 = nullptr;   // [ceil(L/3)][n] section triples (Shape::sec3)
  uint32_t* invp = nullptr;   // [L][4][blocks][64 records] 13-bit bucket records (Shape::pack_inv; pack_inv_section)
  uint64_t* fwd2p = nullptr;  // [ceil(L/2)][words][512] three rows of a section pair per word (Shape::pack_fwd)
  bool invb_done = false;     // ensure_invb has run
};

// Ab table entry of ordering value v: column k = v & (M - 1), sign
// (-1)^popcount(v >> log2 M) in bit 15.
inline uint16_t fwd_entry(uint32_t v, int lgM, int M) {
  return (uint16_t)((v & (uint32_t)(M - 1)) | ((__builtin_popcount(v >> lgM) & 1u) << 15));
}

// Sections padded to whole groups of the fwd table ([G][n][4])
inline int fwd_groups(int L) { return (L + kSG - 1) / kSG * (kSG / kSpw); }

// Inverse of ordering row l (o[0 .. n)) into il[0 .. w), which holds the
// sentinel n everywhere: il[o[r]] = r.  False at the first entry outside
// [1, w) or repeated, with the message in bad.  T: uint16_t, or uint32_t for
// a k_secg operator.
template <typename T>
bool inv_row(const uint32_t* o, int l, int n, int w, T* il, std::string& bad) {
  for (int r = 0; r < n; ++r) {
    const uint32_t v = o[r];
    if (v == 0 || v >= (uint32_t)w) {
      bad = "ordering[" + std::to_string(l) + "," + std::to_string(r) + "] = " + std::to_string(v) +
            " outside [1, w=" + std::to_string(w) + ")";
      return false;
    }
    if (il[v] != (T)n) {
      bad = "ordering row " + std::to_string(l) + " repeats value " + std::to_string(v);
      return false;
    }
    il[v] = (T)r;
  }
  return true;
}

// Ab table entries of section l: fwd [G][n][4], and where asked for the pair
// words fwd2 [ceil(L/2)][n] and the triple words fwd3 [ceil(L/3)][n] (or-ed
// in: the sections of a word are filled by one thread)
inline void fwd_section(const uint32_t* o, int l, int n, int M, uint16_t* fwd, uint32_t* fwd2, uint32_t* fwd3) {
  const int lgM = ilog2(M);
  for (int r = 0; r < n; ++r) {
    const uint16_t e = fwd_entry(o[r], lgM, M);
    fwd[((size_t)(l / kSpw) * n + r) * kSpw + (l % kSpw)] = e;
    if (fwd2) fwd2[(size_t)(l / 2) * n + r] |= (uint32_t)e << (16 * (l & 1));
    if (fwd3)  // M <= 512: k in 9 bits, the sign in bit 9 of a 10-bit field
      fwd3[(size_t)(l / 3) * n + r] |= (uint32_t)((e & 0x1ffu) | ((e >> 15) << 9)) << (10 * (l % 3));
  }
}

// ---- packed tables of the pair / quad kernels (sa_shape.h: pack_rd, pack_dword_pos) ----
// column of a section held by (lane, register i) of a wave with E elements per lane (sa_common.h: elem_index)
inline int elem_index_host(int E, int lane, int i) {
  const int Q = E < 4 ? E : 4;
  return (i / Q) * (64 * Q) + lane * Q + (i % Q);
}
// dwords of one section of the packed bucket table: 4 quarters x blocks of kh steps x 64 records
inline size_t pack_inv_section_dwords(int M, int nhi, int kh) {
  return (size_t)4 * ((nhi + kh - 1) / kh) * 64 * pack_rd(M / 256, kh);
}
// dword and bit of entry (step hh of its block, element i) of a record
inline void pack_entry_at(int EQ, int hh, int i, int& dw, int& sh) {
  const int bit = (hh * EQ + i) * kPackBits;
  dw = bit / 32;
  sh = bit % 32;
}
// Section l of the packed bucket table from its row inv_l [w] of inv: out
// [4][blocks][64 x rd] (zeroed by the caller)
inline void pack_inv_section(int M, int n, int nhi, int kh, const uint16_t* inv_l, uint32_t* out) {
  const int EQ = M / 256, Mq = M / 4, rd = pack_rd(EQ, kh), nb = (nhi + kh - 1) / kh;
  for (int q = 0; q < 4; ++q)
    for (int blk = 0; blk < nb; ++blk) {
      uint32_t* wb = out + ((size_t)q * nb + blk) * 64 * rd;
      for (int lane = 0; lane < 64; ++lane)
        for (int hh = 0; hh < kh; ++hh)
          for (int i = 0; i < EQ; ++i) {
            const int h = blk * kh + hh;
            const uint32_t v = h < nhi ? inv_l[(size_t)h * M + q * Mq + elem_index_host(EQ, lane, i)] : (uint32_t)n;
            int dw, sh;
            pack_entry_at(EQ, hh, i, dw, sh);
            wb[pack_dword_pos(rd, lane, dw)] |= v << sh;
            if (sh + kPackBits > 32) wb[pack_dword_pos(rd, lane, dw + 1)] |= v >> (32 - sh);
          }
    }
}
// ... and its entry of bucket step h, column col, read back
inline uint32_t pack_inv_get(int M, int nhi, int kh, const uint32_t* sec, int h, int col) {
  const int EQ = M / 256, Mq = M / 4, rd = pack_rd(EQ, kh), nb = (nhi + kh - 1) / kh;
  const int q = col / Mq, e = col % Mq, Q = EQ < 4 ? EQ : 4;
  const int lane = (e % (64 * Q)) / Q, i = (e / (64 * Q)) * Q + e % Q;  // elem_index inverted
  const uint32_t* wb = sec + ((size_t)q * nb + h / kh) * 64 * rd;
  int dw, sh;
  pack_entry_at(EQ, h % kh, i, dw, sh);
  uint64_t x = wb[pack_dword_pos(rd, lane, dw)];
  if (sh + kPackBits > 32) x |= (uint64_t)wb[pack_dword_pos(rd, lane, dw + 1)] << 32;
  return (uint32_t)(x >> sh) & ((1u << kPackBits) - 1u);
}

// 20-bit field of a pair-table entry (k0 | s0 << 15 | k1 << 16 | s1 << 31, M <= 512), and back
inline uint32_t pack_fwd_field(uint32_t e) {
  return (e & 0x1ffu) | (((e >> 15) & 1u) << 9) | (((e >> 16) & 0x1ffu) << 10) | ((e >> 31) << 19);
}
inline uint32_t pack_fwd_entry(uint32_t f) {
  return (f & 0x1ffu) | (((f >> 9) & 1u) << 15) | (((f >> 10) & 0x1ffu) << 16) | (((f >> 19) & 1u) << 31);
}
// Pair g of the packed pair Ab table from its row fwd2_g [n]: out [words][512]
inline void pack_fwd_pair(int n, const uint32_t* fwd2_g, uint64_t* out) {
  const int words = pack_fwd_words(n);
  for (int j = 0; j < words; ++j)
    for (int tid = 0; tid < kPackNT; ++tid) {
      uint64_t wv = 0;
      for (int f = 0; f < 3; ++f) {
        const int r = (3 * j + f) * kPackNT + tid;
        wv |= (uint64_t)pack_fwd_field(fwd2_g[r < n ? r : 0]) << (20 * f);
      }
      out[(size_t)j * kPackNT + tid] = wv;
    }
}
// ... and row r's entry, in fwd2's form, read back
inline uint32_t pack_fwd_get(const uint64_t* pair, int r) {
  const int u = r / kPackNT, tid = r % kPackNT;
  return pack_fwd_entry((uint32_t)(pair[(size_t)(u / 3) * kPackNT + tid] >> (20 * (u % 3))) & 0xfffffu);
}

// ---- bank-aware bucket order --------------------------------------------
// The batched section kernel gathers z from LDS, one read per (bucket step,
// element) for a whole wave: 64 random row addresses, served in fixed lane
// groups (MI355X_MICROARCH.md §LDS) where each extra distinct address on a
// busy bank adds one LDS cycle.  k_secb reads 16-byte rows of CB codewords
// (ds_read_b128: four 16-lane groups, 16 bank groups = row % 16).  Visited in
// h order the c3 gather took 2.30 LDS cycles per lane group.  (The same
// order for the single-codeword kernels' 4-byte reads — two 32-lane groups,
// 32 banks — measured neutral: those kernels are latency-bound)  The sum of a
// bucket column k over its slots h does not depend on the order of the
// slots, so these tables re-order them: the slots of sign +1 (popcount(h)
// even) fill steps 0 .. nhi/2 - 1, those of sign -1 steps nhi/2 .. nhi - 1
// (the sign stays uniform per step), and within each half a local search
// swaps a column's slots between steps to minimise, per lane group, the
// largest number of distinct rows on one bank (c3: 1.1 cycles per group
// instead of 2.3).  Empty slots read one of `nbank` zero rows n .. n+nbank-1,
// the one on the step's least loaded bank (all empty lanes of a group read the
// same row: a broadcast).  Seeded per section: the table, and every decode,
// is reproducible.
constexpr int kLdsGroups16[4][16] = {  // ds_read_b128
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// k_secb reads 16-byte rows (binary32 CB = 4, binary64 CB = 2)
inline bool secb_rows16(const Shape& c) {
  return c.backend == SA_BACKEND_HADAMARD && c.CB > 0 && c.CB * (int)rsz(&c) == 16 && !c.big;
}
// ... and gets the bank-aware bucket table
inline bool invb_banked(const Shape& c) {
  return secb_rows16(c) && !(c.plan & SA_PLAN_NO_BANKS) && c.E >= 4 && c.nhi >= 2 && c.n + kInvbZeroRows <= 65535;
}
// its h-steps per table block: kSecbKH64 in binary64, kSecbKH32 at CB = 4
inline int invb_kh(const Shape& c) { return c.prec == SA_PREC_F32 ? kSecbKH32 : kSecbKH64; }

// The column sets of k_secb's gather (16-byte rows, E >= 4): lane L of a wave
// holds columns elem_index<E>(L ^ 3 in binary32 (sgn), i) (quad-mirrored
// positions); one set per (register, 16-lane group)
inline std::vector<int> invb_sets(int E, bool sgn) {
  std::vector<int> sets;
  for (int i = 0; i < E; ++i)
    for (int G = 0; G < 4; ++G)
      for (int j = 0; j < 16; ++j) {
        const int lane = kLdsGroups16[G][j], lp = sgn ? (lane ^ 3) : lane;
        sets.push_back((i / 4) * 256 + lp * 4 + (i % 4));  // elem_index<E >= 4>
      }
  return sets;
}

// Section l of a bank-aware bucket table for sections of M columns, n rows
// and nhi bucket steps.  sets: nsets x gsize columns read by one lane group
// of one read instruction; writes out[h * M + k] (h < nhi) for every column
// of the sets
inline void banked_section(int M, int n, int nhi, int l, const uint16_t* inv_l, uint16_t* out,
                           const std::vector<int>& sets, int gsize, int nbank, uint32_t* hs, int kh) {
  const int Sh = nhi / 2;
  const int nsets = (int)sets.size() / gsize;
  std::mt19937 rng(0x5eed0000u + (uint32_t)l);
  // per sign class, the section's largest number of occupied slots in one
  // column (rounded up to whole blocks of kh steps): the steps used
  int Sc[2] = {0, 0};
  for (int cls = 0; cls < 2; ++cls) {
    for (int col = 0; col < M; ++col) {
      int m = 0;
      for (int h = 0; h < nhi; ++h)
        if ((__builtin_popcount(h) & 1) == cls && inv_l[(size_t)h * M + col] != (uint16_t)n) ++m;
      Sc[cls] = std::max(Sc[cls], m);
    }
    Sc[cls] = std::min(Sh, std::max(kh, (Sc[cls] + kh - 1) / kh * kh));
  }
  if (hs) hs[l] = (uint32_t)Sc[0] | ((uint32_t)Sc[1] << 16);
  std::vector<int> A((size_t)gsize * Sh), cnt((size_t)Sh * nbank), emp(Sh), cost(Sh);
  auto step_cost = [&](int st) {
    const int* ct = &cnt[(size_t)st * nbank];
    int mx = 0, mn = 1 << 30;
    for (int g = 0; g < nbank; ++g) { mx = std::max(mx, ct[g]); mn = std::min(mn, ct[g]); }
    return emp[st] ? std::max(mx, mn + 1) : mx;
  };
  auto take = [&](int st, int v, int d) {
    if (v < 0) emp[st] += d;
    else cnt[(size_t)st * nbank + (v % nbank)] += d;
  };
  for (int si = 0; si < nsets; ++si) {
    const int* cols = &sets[(size_t)si * gsize];
    for (int cls = 0; cls < 2; ++cls) {
      const int S = Sc[cls];
      std::fill(cnt.begin(), cnt.end(), 0);
      std::fill(emp.begin(), emp.end(), 0);
      for (int j = 0; j < gsize; ++j) {
        int m = 0;
        int* a = &A[(size_t)j * S];
        for (int h = 0; h < nhi; ++h)
          if ((__builtin_popcount(h) & 1) == cls && inv_l[(size_t)h * M + cols[j]] != (uint16_t)n)
            a[m++] = inv_l[(size_t)h * M + cols[j]];
        for (; m < S; ++m) a[m] = -1;
        std::shuffle(a, a + S, rng);
        for (int st = 0; st < S; ++st) take(st, a[st], +1);
      }
      for (int st = 0; st < S; ++st) cost[st] = step_cost(st);
      // moves target the conflict: a column of the worst step that sits on
      // that step's most loaded bank (random columns: the same tables after
      // 4000 moves that these reach after 256, c3 1.10 / c4 1.005 LDS cycles
      // per lane group, ~1 / 16 of the host time)
      for (int it = 0; it < 256; ++it) {
        int s1 = 0;
        for (int st = 1; st < S; ++st)
          if (cost[st] > cost[s1]) s1 = st;
        if (cost[s1] <= 1) break;  // conflict-free
        int j;
        {
          const int* ct = &cnt[(size_t)s1 * nbank];
          int bm = 0;
          for (int g = 1; g < nbank; ++g)
            if (ct[g] > ct[bm]) bm = g;
          int cand[64], nc = 0;
          for (int jj = 0; jj < gsize && nc < 64; ++jj) {
            const int v = A[(size_t)jj * S + s1];
            if (v >= 0 && v % nbank == bm) cand[nc++] = jj;
          }
          j = nc > 0 ? cand[rng() % (unsigned)nc] : (int)(rng() % (unsigned)gsize);
        }
        const int s2 = (int)(rng() % (unsigned)S);
        if (s2 == s1) continue;
        int& x = A[(size_t)j * S + s1];
        int& y = A[(size_t)j * S + s2];
        if (x == y) continue;
        take(s1, x, -1); take(s2, y, -1); take(s1, y, +1); take(s2, x, +1);
        const int n1 = step_cost(s1), n2 = step_cost(s2);
        if (n1 + n2 <= cost[s1] + cost[s2]) {
          std::swap(x, y);
          cost[s1] = n1;
          cost[s2] = n2;
        } else {
          take(s1, y, -1); take(s2, x, -1); take(s1, x, +1); take(s2, y, +1);
        }
      }
      for (int st = 0; st < S; ++st) {
        int zg = 0;
        for (int g = 1; g < nbank; ++g)
          if (cnt[(size_t)st * nbank + g] < cnt[(size_t)st * nbank + zg]) zg = g;
        const int zrow = n + ((zg - n % nbank + nbank) % nbank);  // the zero row on bank zg
        for (int j = 0; j < gsize; ++j) {
          const int v = A[(size_t)j * S + st];
          out[(size_t)(cls * Sh + st) * M + cols[j]] = (uint16_t)(v >= 0 ? v : zrow);
        }
      }
      for (int st = S; st < Sh; ++st)  // never gathered (every column's slots sit in the first S steps)
        for (int j = 0; j < gsize; ++j) out[(size_t)(cls * Sh + st) * M + cols[j]] = (uint16_t)n;
    }
  }
}

// ---- bank-aware Ab row order ----------------------------------------------
// k_secb's Ab pass gives lane L of a wave row r0 + L and reads, per step, one
// staged T element (section s, column k(r, s)) per lane: for 16-byte T rows a
// ds_read_b128 whose four 16-lane groups each take one LDS cycle per distinct
// row on their busiest 16-byte bank group (MI355X_MICROARCH.md §LDS).  In
// section order the columns k(r, s) of 16 rows are random: ~3 cycles per
// group.  A row's partial sum does not care in which order its W sections
// are added, so each row gets its own step order: a local search over swaps
// of two steps of one row that lowers, per lane group, the largest number of
// rows on one bank in a step (the addition order changes, the terms do not).
// Rows n .. npad-1 (the last block's idle lanes) repeat a real row of their
// lane group (a broadcast); sections past L read column 0 (a broadcast).
// LDS position of T column e in k_secb's staged image: the element index of
// (lane, register i) is (i / Q) 64 Q + lane Q + i % Q (elem_index), staged at
// (i / Q) 64 Q + (i % Q) 64 + lane
inline unsigned t_pos(int E, unsigned e) {
  const unsigned Q = E < 4 ? (unsigned)E : 4u;
  const unsigned blk = e / (64 * Q), rem = e % (64 * Q);
  return blk * 64 * Q + (rem % Q) * 64 + rem / Q;
}

// Group g (W sections of M = 64 E columns, of L) of k_secb's Ab table from
// fwd [G][n][4].  rowb: bytes per staged T element; search: the bank-aware
// step order (else section order); out [Gb * W / 4][npad][4].
inline void fwdb_group(int W, int M, int n, int L, int E, int rowb, bool search, int g, const uint16_t* fwd,
                       int npad, uint16_t* out) {
  const bool b128 = rowb == 16;
  const int gsize = b128 ? 16 : 32, nbank = b128 ? 16 : 32, ngroups = 64 / gsize;
  std::mt19937 rng(0xab0000u + (uint32_t)g);
  std::vector<int> cnt((size_t)W * nbank), perm((size_t)gsize * W), bank((size_t)gsize * W), cost(W);
  std::vector<uint16_t> ent((size_t)gsize * W);
  auto step_cost = [&](int st) {
    int mx = 0;
    for (int b = 0; b < nbank; ++b) mx = std::max(mx, cnt[(size_t)st * nbank + b]);
    return mx;
  };
  for (int b0 = 0; b0 < npad; b0 += 64) {
    for (int G = 0; G < ngroups; ++G) {
      int rows[32], nreal = 0;
      for (int j = 0; j < gsize; ++j) {
        const int lane = b128 ? kLdsGroups16[G][j] : G * 32 + j;
        rows[j] = b0 + lane;
      }
      // entries (s * M + k | sign) and banks of the real rows, identity order
      std::fill(cnt.begin(), cnt.end(), 0);
      for (int j = 0; j < gsize; ++j) {
        const int r = rows[j];
        if (r >= n) continue;
        ++nreal;
        for (int sl = 0; sl < W; ++sl) {
          const int l = g * W + sl;
          uint16_t e = 0;
          if (l < L) e = fwd[((size_t)(l / kSpw) * n + r) * kSpw + (l % kSpw)];
          const unsigned k = t_pos(E, e & 0x7fffu);
          ent[(size_t)j * W + sl] = (uint16_t)(((unsigned)sl * M + k) | (e & 0x8000u));
          bank[(size_t)j * W + sl] = l < L ? (int)(((unsigned)sl * M + k) % (unsigned)nbank) : -1;
          perm[(size_t)j * W + sl] = sl;
          if (l < L) ++cnt[(size_t)sl * nbank + bank[(size_t)j * W + sl]];
        }
      }
      if (search && nreal > 1) {
        for (int st = 0; st < W; ++st) cost[st] = step_cost(st);
        // 16 W moves: the searched tables reach a sum of step costs 1.17x that
        // of 64 W moves (C4), with the same C3 / C4 throughput, in a quarter
        // of the host time (0.11 -> 0.05 s at C4)
        for (int it = 0; it < 16 * W; ++it) {
          int s1 = 0;
          for (int st = 1; st < W; ++st)
            if (cost[st] > cost[s1]) s1 = st;
          if (cost[s1] <= 1) break;
          int bm = 0;
          for (int b = 1; b < nbank; ++b)
            if (cnt[(size_t)s1 * nbank + b] > cnt[(size_t)s1 * nbank + bm]) bm = b;
          int cand[32], nc = 0;
          for (int j = 0; j < gsize; ++j)
            if (rows[j] < n && bank[(size_t)j * W + perm[(size_t)j * W + s1]] == bm) cand[nc++] = j;
          if (nc == 0) break;
          const int j = cand[rng() % (unsigned)nc];
          const int s2 = (int)(rng() % (unsigned)W);
          if (s2 == s1) continue;
          int& x = perm[(size_t)j * W + s1];
          int& y = perm[(size_t)j * W + s2];
          const int bx = bank[(size_t)j * W + x], by = bank[(size_t)j * W + y];
          auto mv = [&](int st, int b, int d) {
            if (b >= 0) cnt[(size_t)st * nbank + b] += d;
          };
          mv(s1, bx, -1); mv(s2, by, -1); mv(s1, by, +1); mv(s2, bx, +1);
          const int n1 = step_cost(s1), n2 = step_cost(s2);
          if (n1 + n2 <= cost[s1] + cost[s2]) {
            std::swap(x, y);
            cost[s1] = n1;
            cost[s2] = n2;
          } else {
            mv(s1, by, -1); mv(s2, bx, -1); mv(s1, bx, +1); mv(s2, by, +1);
          }
        }
      }
      // out [g * W/4 + q][npad][4]: step st = 4 q + slot; idle rows copy the
      // group's first real row (or, with none, row 0 of the block's order)
      int jr = -1;
      for (int j = 0; j < gsize && jr < 0; ++j)
        if (rows[j] < n) jr = j;
      for (int j = 0; j < gsize; ++j) {
        const int src = rows[j] < n ? j : jr;
        for (int st = 0; st < W; ++st) {
          const uint16_t e = src >= 0 ? ent[(size_t)src * W + perm[(size_t)src * W + st]] : (uint16_t)((unsigned)st * M);
          out[((size_t)(g * (W / 4) + st / 4) * npad + rows[j]) * 4 + (st % 4)] = e;
        }
      }
    }
  }
}

}  // namespace sa
