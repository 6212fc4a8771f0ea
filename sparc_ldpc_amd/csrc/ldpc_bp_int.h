// ldpc_bp_int.h — what the translation units of libldpc_bp.so share: the
// decoder context and the helpers defined in ldpc_bp.hip that the Monte-Carlo
// unit (ldpc_mc.hip) builds on.  Not part of the C ABI (include/ldpc_bp.h).
#ifndef LDPC_BP_INT_H
#define LDPC_BP_INT_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "ldpc_bp.h"

struct lb_mc;  // the Monte-Carlo pipeline's state (ldpc_mc.hip)

struct lb_ctx {
  int dev = 0, Nv = 0, Nc = 0, Nmsg = 0, maxdv = 0, maxdc = 0, mindc = 0, nt = 0;
  bool fixed = false;  // check-regular with a straight-line check kernel (lxfb_fixed)
  bool lds = false;
  // tail launches (k_bp_tail): edge tables, per-word state, first tail iteration
  int tail_at = 0, nq = 0, ncu = 256;
  int* d_evar = nullptr;
  int *d_active = nullptr, *d_nact = nullptr, *d_done = nullptr, *d_lastbad = nullptr;
  int* h_nact = nullptr;  // pinned: [0] words entering the tail, [1..2] done counts of the last chunks,
                        // [3] the last device-sized tail's words
  hipEvent_t evc[2] = {nullptr, nullptr};
  hipEvent_t evn = nullptr;   // device-sized tails: its word count has landed in h_nact[0]
  bool est_pending = false;   // a device-sized tail's word count is in flight
  int est_n = 0, est_B = 0, est_Bq = 0;  // the last landed count and its batch; the batch in flight
  int capTailB = 0;
  int tail_default = 0;       // tail_at chosen at lb_create (kTailAt or LDPC_BP_TAIL)
  int* d_vedge = nullptr;
  uint8_t* d_vdeg = nullptr;
  int* d_cstart = nullptr;
  double *d_ch = nullptr, *d_app = nullptr, *d_msg = nullptr;
  int* d_it = nullptr;
  int capB = 0, capMsgB = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // layered schedule (k_bpl), set by lb_set_layers: the layers' first checks on
  // the device, where the messages live (2: r + app in LDS, 1: app in LDS,
  // 0: HBM), threads per workgroup; host copies of the edge tables for its checks
  std::vector<int> h_evar, h_cstart;
  int* d_lfirst = nullptr;
  int nlayers = 0, maxlayer = 0, lmode = 0, lnt = 0;
  int lmode32 = 0;            // lmode of the binary32 instances (LB_F32): the same choice at 4 bytes a message
  bool lfixed = false;
  bool lone32 = false;        // LDPC_BP_LAYERED_F32_RESIDENT = 1: binary32 workgroups padded to one per CU
  std::vector<const void*> raised;  // kernel instances whose dynamic LDS limit this context has raised
  // fixed-point layered min-sum (k_bplq), lb_set_fixed: the widths; the plan made by lb_set_layers /
  // lb_set_fixed: threads per workgroup, lanes per check, dynamic LDS bytes, whether the image fits
  int qfrac = 2, qmsg = 6, qapp = 8;
  int qnt = 0, qlanes = 0, qlds = 0;
  bool qfit = false;
  lb_mc* mc = nullptr;        // encoder tables, staging and counters of lb_mc_run (ldpc_mc.hip)
};

namespace lb {

// record the message lb_last_error returns (per thread) and hand `code` back
int fail(int code, const std::string& msg);

int dev_alloc(void** p, size_t bytes);
// the context's ch / app / iters buffers sized for B words
int ensure_io(lb_ctx* c, int B);
// the fixed-point kernels' parameters: fraction bits, the clips of r and app, 16 corr_factor
struct FixedPar {
  int frac, rmax, amax, alpha;
};
// A decoder type (`algo` of the C ABI: one of the five LB_* numbers, with LB_F32 or LB_FIXED) as
// lb::resolve found it on a context; what launch, stream_plan and launch_stream take.
struct DecType {
  int base = 0;   // LB_SUMPROD2 .. LB_LAYERED_MINSUM
  bool f32 = false, fixed = false;
  bool hbm = false;  // a layered type that keeps each word's messages in a slice of HBM (lmode < 2)
  FixedPar par{};    // fixed
};
// Fill `t`, or refuse algo / corr / max_iter on this context (LB_ERR_ARG, LB_ERR_UNSUPPORTED): every
// refusal of a decoder type is here.  for_stream: the block stream, which has the layered types only
// and refuses up front what the batch path refuses once it has work (lb::launch).
int resolve(lb_ctx* c, int algo, double corr, int max_iter, bool for_stream, DecType* t);
// queue a decode of B words on the context's stream; sized_on_host = false never waits
int launch(lb_ctx* c, int B, const double* d_ch, double* d_app, int* d_it, const DecType& t, double corr,
           int max_iter, bool sized_on_host);
// One chunk of lb_mc_stream_seeds for the persistent layered kernels (k_bpls,
// k_bpls32, k_bplsq in ldpc_bp.hip): a grid of `slots` workgroups takes the chunk's
// blocks by ticket, decodes and counts them.
struct StreamChunk {
  const double* ch;   // [chunk][Nv]
  const uint8_t* x;   // [chunk][Nv]
  double* app;        // [slots][Nv]
  double* msg;        // [slots][Nmsg] (unused with r and app in LDS)
  int* slot_iters;    // [slots]
  int* errs;          // [chunk]
  int* iters;         // [chunk], -1: skipped by the stop rule
  int* ticket;        // zeroed
  const int* eprev;   // block errors of the chunk before
  int* ecur;          // zeroed: block errors of this chunk
  int chunk, base, min_errors;
};
// resident: workgroups of the type's persistent instance a CU holds at once (t resolved for_stream)
int stream_plan(lb_ctx* c, const DecType& t, int* resident);
// queue one chunk on `st`; never waits
int launch_stream(lb_ctx* c, hipStream_t st, int slots, const StreamChunk& k, const DecType& t, double corr,
                  int max_iter);
// free the Monte-Carlo state of a context (ldpc_mc.hip)
void mc_release(lb_ctx* c);

}  // namespace lb

#define HIP_TRY(expr)                                                                \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess)                                                            \
      return lb::fail(LB_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

#endif  // LDPC_BP_INT_H
