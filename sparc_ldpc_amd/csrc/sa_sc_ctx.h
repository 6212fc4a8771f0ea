// sa_sc_ctx.h — the coupled context (struct sa_sc) and the few host helpers
// its two translation units share: sa_sc.hip (kernels, decode, the one-call and
// the staged C ABI) and sa_glue.hip (the SPARC <-> LDPC glue on the context's
// d_beta, launched next to the glue kernels so that there is one copy of them).
// The host rules are sa_sc.h; DESIGN.md sections 13 and 13c.
#pragma once
#include "sa_host.h"
#include "sa_sc.h"

struct sa_sc {
  sa_ctx* parent = nullptr;
  sa::ScLayout lay;
  std::vector<double> W;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;  // ev0 / ev1 bracket the last decode's loop
  void *d_W = nullptr, *d_sqW = nullptr;  // [R][C] in the context precision: W and sqrt(W)
  uint16_t* d_fwd = nullptr;              // the padded groups' Ab table (ScLayout::own_fwd), else null
  void *d_c = nullptr, *d_Pc = nullptr;   // [L] sqrt(n Pl), [C] column-block powers
  double* d_cd = nullptr;                 // [L] sqrt(n Pl) in binary64: what the glue kernels read
  int Bcap = 0, Tcap = 0;
  void *d_y = nullptr, *d_z = nullptr, *d_beta = nullptr, *d_out = nullptr;
  void *d_abp = nullptr, *d_bbp = nullptr, *d_zzp = nullptr, *d_phi = nullptr;
  int *d_iters = nullptr, *d_done = nullptr;
  int32_t *d_idx = nullptr, *d_dec = nullptr, *d_errs = nullptr;
  double* d_noise = nullptr;
  double* d_stage = nullptr;
  size_t stage_cap = 0;
  // the wave form's state (a decode with a tolerance above 0): allocated at its first use
  void* d_taul = nullptr;            // [wBcap][2][C]
  unsigned char* d_live = nullptr;   // [wBcap][wTcap][C]
  int wBcap = 0, wTcap = 0;
  // the staged life cycle (sa_sc_reserve ... sa_sc_fetch; sa_sc.h: sc_stage_rule)
  sa::ScStageState st;
  int Trun = -1;  // T of the last sa_sc_run (-1: none since the workspace was sized)
};

namespace sa {

// a binary64 staging buffer of `count` values on the context's stream (grown, never shrunk)
int sc_stage(sa_sc* s, size_t count);
// k_bits_idx of sa_glue.hip on `stream`: message bits -> section indices
int launch_bits_idx(hipStream_t stream, const uint8_t* d_bits, int lgM, int L, int B, int32_t* d_idx);

}  // namespace sa
