// sa_seq.h — the launch sequence of an AMP decode as a pure host rule: which
// launches a decode of (shape, B, T, flags, beta0) makes, in which order, which
// buffer its estimate ends in and what it leaves pending (Step, DecodeSeq,
// decode_seq, for_each_step).  No HIP include: csrc/sa_host_check.cpp prints
// the sequence on a machine without a GPU.  seq_amp (sparc_amp.hip) walks the
// steps into the launchers; nothing else decides a launch of a decode.
#pragma once
#include "sa_shape.h"

namespace sa {

enum { SEC_AMP = 0, SEC_AZ = 1, SEC_AB = 2 };                     // SecArgs::mode
enum { ROW_INIT0 = 0, ROW_INIT = 1, ROW_AMP = 2, ROW_ABOUT = 3 };  // RowArgs::mode

// One launch of a decode.
enum StepKind {
  ST_FILL_ITERS,   // k_fill32: iters = -1
  ST_ZERO_BETA,    // k_fill32: d_beta = 0
  ST_DENSE_START,  // dense backends: z = y - A beta0
  ST_SEC_AB,       // launch_sec, SEC_AB: the partials of A beta0
  ST_ROW,          // launch_row
  ST_SEC,          // launch_sec, SEC_AMP
  ST_SEC_MW,       // launch_sec2: the multi-wave kernels
  ST_SEC_B,        // launch_secb: the batched kernel
  ST_DENSE_ITER,   // dense backends: A^T z, denoiser, A beta partials
  ST_ITERS_FINAL,  // k_iters_final
  ST_BETA_FINAL,   // k_beta_final
};

struct Step {
  StepKind kind = ST_ROW;
  int t = 0;            // the iteration (section, dense and ROW_AMP steps)
  int mode = 0;         // ST_ROW: ROW_INIT0 / ROW_INIT / ROW_AMP
  int rd = 0, wr = 0;   // ST_SEC, ST_SEC_MW: the estimate read and written, 0 = d_beta, 1 = d_beta2
  bool bzero = false;   // ST_SEC_MW: the previous estimate is taken as zero (SecArgs::bzero)
  bool decide = false;  // ST_SEC_MW: the launch writes the section decisions (SecArgs::dec)
  int itset = 0;        // the iters value the launch writes, 0: none (ST_ITERS_FINAL: T)
  int G = 0, Gb = 0;    // ST_ROW: the partial counts of whatever produced abp / bbp
  int es = 0;           // the early stop is on
};

inline Step row_step(int mode, int t, int es, int G, int Gb, int itset) {
  Step s;
  s.kind = ST_ROW; s.mode = mode; s.t = t; s.es = es; s.G = G; s.Gb = Gb; s.itset = itset;
  return s;
}

// The row step a fused tail leaves undone: iteration T - 1, no stop test, no
// iters write (the last section launch set them).  row_flush launches it.
inline Step deferred_row(const Plan& p, int T) { return row_step(ROW_AMP, T - 1, 0, p.G, p.Gb, 0); }

// A decode of T iterations: what a run needs to know without walking the
// steps, and the decisions for_each_step unfolds into them.
struct DecodeSeq {
  // Fused tail: with the early stop off the last launch is known when the
  // sequence is built, so the last section launch of the pair / triple / quad
  // kernels also writes the section decisions and iters = T (Step::decide,
  // itset), k_decide is never launched, and the sequence ends there: the
  // k_row2 step behind it, whose z_T only sa_fetch_z reads, is `row`, left
  // pending in the lane (sa_host.h: tail_issued).  Not under sa_profile, which
  // times every launch, and not with a padded section.
  bool fused = false;
  Step row;                 // the deferred row step (fused only)
  bool zil = false;         // the decode leaves z codeword-interleaved (zil_for)
  bool beta_final = false;  // k_beta_final runs: the estimate may have ended in d_beta2
  int nsteps = 0;           // launches of the sequence (the deferred row not among them)
  // The fixed launches around the T iterations.  Behind k_row2 (it_row) the
  // iters writes ride on row launches the decode makes anyway: -1 with the
  // residual's initialisation, T with the last iteration.  Behind k_sec4 /
  // k_sec43 / k_sec44 a decode without beta0 fills no zero estimate (bz): its
  // first section launch takes the previous estimate as zero.  With the early
  // stop off the final estimate's buffer is known: without beta0 the ping-pong
  // starts on the side (flip) that ends in d_beta, and k_beta_final is launched
  // only where the estimate ends in d_beta2 (beta0 lies in d_beta: no choice).
  int T = 0, es = 1, flip = 0;
  bool has_b0 = false, it_row = false, bz = false;
  StepKind sec = ST_SEC;    // the section step of an iteration
  int G = 0, Gb = 0;        // the plan's partial counts
  int G0 = 0;               // Shape::G: A beta0 comes from k_sec, whatever the loop's producer
};

inline DecodeSeq decode_seq(const Shape& c, const Plan& p, int T, int flags, bool has_b0, bool profiled) {
  DecodeSeq q;
  q.T = T;
  q.es = (flags & SA_FLAG_NO_EARLY_STOP) ? 0 : 1;
  q.has_b0 = has_b0;
  q.it_row = p.it_row() && T > 0;
  q.bz = !has_b0 && p.bzero() && T > 0;
  q.flip = (q.bz && !q.es) ? (T & 1) : 0;
  q.sec = p.dense() ? ST_DENSE_ITER : p.batched() ? ST_SEC_B : p.multiwave() ? ST_SEC_MW : ST_SEC;
  q.G = p.G; q.Gb = p.Gb; q.G0 = c.G;
  q.zil = p.zil;
  q.fused = p.bzero() && q.it_row && !q.es && c.dead == 0 && !profiled && !(c.plan & SA_PLAN_NO_FUSED_TAIL);
  if (q.fused) q.row = deferred_row(p, T);
  // early stop off: every codeword runs T iterations, the last one into wr(T - 1);
  // else the estimate of codeword b is in the buffer of parity iters[b]
  const bool one = q.sec == ST_SEC || q.sec == ST_SEC_MW, home = !q.es && (((T - 1) ^ q.flip) & 1);
  q.beta_final = one && T > 0 && !home;
  const int start = has_b0 ? (p.dense() ? 1 : 2) : (q.bz ? 1 : 2);
  q.nsteps = (q.it_row ? 0 : 2) + start + 2 * T - (q.fused ? 1 : 0) + (q.beta_final ? 1 : 0);
  return q;
}

// f(const Step&) -> int for every launch of the sequence, in order; stops at
// the first nonzero answer and returns it.
template <typename F>
int for_each_step(const DecodeSeq& q, F f) {
  auto step = [&](StepKind k, int t) {
    Step s;
    s.kind = k; s.t = t;
    return s;
  };
  const int T = q.T, it0 = q.it_row ? -1 : 0;
  int rc;
  if (!q.it_row && (rc = f(step(ST_FILL_ITERS, 0)))) return rc;
  if (q.has_b0) {
    if (q.sec == ST_DENSE_ITER) {
      if ((rc = f(step(ST_DENSE_START, 0)))) return rc;
    } else {
      if ((rc = f(step(ST_SEC_AB, 0)))) return rc;
      if ((rc = f(row_step(ROW_INIT, 0, 0, q.G0, q.G0, it0)))) return rc;
    }
  } else {
    if (!q.bz && (rc = f(step(ST_ZERO_BETA, 0)))) return rc;
    if ((rc = f(row_step(ROW_INIT0, 0, 0, q.G, q.Gb, it0)))) return rc;
  }
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    Step s = step(q.sec, t);
    s.es = q.es;
    if (q.sec == ST_SEC || q.sec == ST_SEC_MW) {
      s.rd = (t ^ q.flip) & 1;
      s.wr = s.rd ^ 1;
    }
    if (q.sec == ST_SEC_MW) {
      s.bzero = q.bz && t == 0;
      s.decide = q.fused && last;
      s.itset = s.decide ? T : 0;
    }
    if ((rc = f(s))) return rc;
    if (q.fused && last) break;  // q.row stays pending
    if ((rc = f(row_step(ROW_AMP, t, q.es, q.G, q.Gb, q.it_row && last ? T : 0)))) return rc;
  }
  if (!q.it_row) {
    Step s = step(ST_ITERS_FINAL, 0);
    s.itset = T;
    if ((rc = f(s))) return rc;
  }
  if (q.beta_final && (rc = f(step(ST_BETA_FINAL, 0)))) return rc;
  return 0;
}

}  // namespace sa
