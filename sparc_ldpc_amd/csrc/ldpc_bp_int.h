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
#include "ldpc_plan.h"

struct lb_mc;  // the Monte-Carlo pipeline's state (ldpc_mc.hip)

// The plans are lb_ctx's bases: lb_create sets the GraphPlan, lb_set_layers the LayerPlan and the
// FixedPlan, lb_set_tail and lb_set_fixed change tail_at and the FixedPlan (ldpc_plan.h has the fields).
struct lb_ctx : lb::GraphPlan, lb::LayerPlan, lb::FixedPlan {
  int dev = 0, ncu = 256;
  // tail launches (k_bp_tail): edge tables, per-word state
  int* d_evar = nullptr;
  int *d_active = nullptr, *d_nact = nullptr, *d_done = nullptr, *d_lastbad = nullptr;
  int* h_nact = nullptr;  // pinned: [0] words entering the tail, [1..2] done counts of the last chunks,
                        // [3] the last device-sized tail's words
  hipEvent_t evc[2] = {nullptr, nullptr};
  hipEvent_t evn = nullptr;   // device-sized tails: its word count has landed in h_nact[0]
  bool est_pending = false;   // a device-sized tail's word count is in flight
  int est_n = 0, est_B = 0, est_Bq = 0;  // the last landed count and its batch; the batch in flight
  int capTailB = 0;
  int* d_vedge = nullptr;
  uint8_t* d_vdeg = nullptr;
  int* d_cstart = nullptr;
  double *d_ch = nullptr, *d_app = nullptr, *d_msg = nullptr;
  int* d_it = nullptr;
  int capB = 0, capMsgB = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // layered schedule (k_bpl), set by lb_set_layers: the layers' first checks on the device; host
  // copies of the edge tables for its checks
  std::vector<int> h_evar, h_cstart;
  int* d_lfirst = nullptr;
  std::vector<const void*> raised;  // kernel instances whose dynamic LDS limit this context has raised
  lb_mc* mc = nullptr;        // encoder tables, staging and counters of lb_mc_run (ldpc_mc.hip)
};

namespace lb {

// record the message lb_last_error returns (per thread) and hand `code` back
int fail(int code, const std::string& msg);

int dev_alloc(void** p, size_t bytes);
// the context's ch / app / iters buffers sized for B words
int ensure_io(lb_ctx* c, int B);
// ldpc_plan.h's resolve on the context's plans, the refusal recorded by fail (DecType: there)
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
