// sa_host.h — the operator context (sa_ctx), launch timing and the host-side
// helpers shared by the kernel units and the C ABI (sparc_amp.hip).
#pragma once
#include "sa_common.h"
#include "sa_tables.h"

namespace sa {

// Per-launch timing for sa_profile (eager sequence only).
// Event mode: every profiled launch is bracketed by two HIP event records;
// with rep > 1 it is issued rep times back to back between them
// (sa_profile_rep: mean = elapsed / rep, which excludes the event packets'
// own dispatch overhead but lets each repeat re-read what its predecessor
// left in the caches).  Dispatch mode (sa_profile_dispatch): each launch goes
// out once through hipExtLaunchKernel with a start / stop event pair that the
// runtime binds to the kernel's own dispatch packet, so the pair times the
// kernel's execution in the decode's order (the quantity a rocprofv3 kernel
// trace records), with no marker packets in the stream.
struct Prof {
  std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> ev;
  int rep = 1;
  bool dispatch = false;
  int kind = 0;
  int begin(hipStream_t s, int k) {
    kind = k;
    if (dispatch) return 0;
    hipEvent_t a = nullptr, b = nullptr;
    if (add(&a, &b)) return -1;
    return hipEventRecord(a, s) == hipSuccess ? 0 : -1;
  }
  void end(hipStream_t s) {
    if (!dispatch) (void)hipEventRecord(std::get<2>(ev.back()), s);
  }
  int add(hipEvent_t* a, hipEvent_t* b) {
    *a = *b = nullptr;
    if (hipEventCreate(a) != hipSuccess || hipEventCreate(b) != hipSuccess) return -1;
    ev.emplace_back(kind, *a, *b);
    return 0;
  }
  ~Prof() {
    for (auto& e : ev) {
      (void)hipEventDestroy(std::get<1>(e));
      (void)hipEventDestroy(std::get<2>(e));
    }
  }
};

enum { K_SEC = 0, K_ROW = 1, K_DAZ = 2, K_DDEN = 3, K_DAB = 4, K_QNT = 5, K_NKINDS = 6 };

}  // namespace sa

// A decode lane: everything one small-batch decode mutates, so that two
// consecutive decodes of a context can share the chip (step k + 1 reads
// nothing step k writes; the tables, the power arrays and the decision ring
// are read-only during a decode and stay shared).  A lane's state lives here
// and nowhere else: the context holds lane[kLanes] and the index cur of the
// current lane (the lane of the last sa_run), and every entry point reaches
// the stream / d_* / graphs of that lane through sa_ctx::at().  A field added
// to a lane is declared here once.  A reference taken from at() names a lane
// object, not "the current lane": take it after the last call that can change
// cur (lane_switch, lanes_release, ensure_workspace, ensure_beta2, run_graph).
struct sa_lane {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void *d_y = nullptr, *d_z = nullptr, *d_beta = nullptr, *d_abp = nullptr;
  void *d_bbp = nullptr, *d_zzp = nullptr, *d_tau = nullptr;  // d_bbp lies in d_tau's allocation (lane_alloc)
  void* d_beta2 = nullptr;  // ping-pong partner of d_beta for k_sec (B x L*M), sized beta2_cap
  int* d_iters = nullptr;
  double* d_stage = nullptr;  // a lane's uploads go through its own staging buffer
  size_t stage_cap = 0;
  int beta2_cap = 0;
  std::map<std::tuple<int, int, int, int>, hipGraphExec_t> graphs;  // their kernel arguments hold the lane's pointers
  hipEvent_t y_ev = nullptr;      // behind the last write of this lane's d_y (staging, or the copy from the other lane)
  unsigned long long y_ver = 0;   // version of the y this lane holds (sa_ctx::y_ver: the latest staged)
  bool y_read = false;            // this lane's last y copy read the other lane's d_y (that lane's next y write waits for y_ev)
  // Fused tail (sa_seq.h: DecodeSeq::fused): the lane's last run ended with its
  // last section launch, which wrote the decisions of fused_B codewords into
  // h_dec (pinned, device-mapped at d_dec, Bcap x L; marked by ev1), and left
  // the row step of iteration row_T - 1 of row_B codewords undone: nothing of
  // the decode, its decisions or its estimate reads z_T.  row_flush launches
  // that step for whoever reads d_z / d_zzp, or is about to change what it
  // reads (y, the power, the partials); the lane's next run drops it.
  // Assigned by the tail_* transitions below and nowhere else.
  int32_t *h_dec = nullptr, *d_dec = nullptr;
  int fused_B = 0;
  int row_B = 0, row_T = 0;
};

// The operator context.  Its shape numbers are the base (sa_shape.h: Shape,
// filled by shape_for alone), its tables are `tab` (sa_tables.h: Tables).
struct sa_ctx : sa::Shape {
  sa::Prof* prof = nullptr;
  // decode lanes (compile-time 2: the ring and bench protocols keep at most two steps in flight)
  enum { kLanes = 2 };
  sa_lane lane[kLanes];
  int cur = 0;            // the current lane
  sa_lane& at() { return lane[cur]; }
  const sa_lane& at() const { return lane[cur]; }
  bool lanes_on = false;  // lane 1's buffers exist (created at the first eligible sa_run)
  unsigned long long y_ver = 0;  // version of the y staged last
  int y_lane = 0;                // the lane that holds it
  std::vector<double> h_Pl;      // the Pl behind d_c / d_cd / d_P1 (set_power skips an unchanged one)
  std::vector<double> h_Plb;     // the Pl behind d_cb / d_Pb (set_power_batch)
  int device = 0;
  int RS = 1, KS = 1;  // dense splits
  size_t lda = 0;
  // (describes one lane's d_z, yet stays here: in the lane, sa_fetch_z after sa_mc_stage would answer differently)
  bool zil_last = false;  // the last decode left z codeword-interleaved ([NC][n][CB], zil_for)
  std::vector<uint32_t> ordering;
  sa::Tables tab;         // the operator tables (sa_tables.h)
  bool borrowed = false;  // ... are another context's (sa_create_twin): not freed here
  void* d_A = nullptr;  // dense [np][lda] design matrix (binary32; SA_BACKEND_MATRIX: the context precision)
  // int8 matrix-core dense path (B >= 4; dense_i8.hip): A8 [np8][LMp8], AT8 [LMp8][np8],
  // digit planes of z [3][Bp8][np8] and beta [3][Bp8][LMp8], per-codeword scales
  int8_t *d_A8 = nullptr, *d_AT8 = nullptr, *d_zq = nullptr, *d_bq = nullptr;
  double *d_zsc = nullptr, *d_bsc0 = nullptr, *d_bfix = nullptr;
  long long np8 = 0, LMp8 = 0;
  int Bp8 = 0;
  // caller's dense matrix (SA_BACKEND_MATRIX): rows padded to np (a whole
  // number of 256-row GEMM tiles); for B >= kFMinB codewords (dense_mfma.hip)
  // its transpose AT [LMy][nk] and the padded GEMM vectors xz [Bcap][nk] (z)
  // and xb [Bcap][lda] (beta, when L*M is not a whole number of K stages)
  long long np = 0, nk = 0, LMy = 0;
  void *d_AT = nullptr, *d_xz = nullptr, *d_xb = nullptr;
  int fg_cap = 0;
  double cmax = 0;  // max_l sqrt(n Pl_l) of the shared power allocation
  // workspace shared by the lanes (lane 0's decode buffers are sized with it)
  int Bcap = 0, Tcap = 0;
  void *d_out = nullptr, *d_c = nullptr, *d_azp = nullptr;
  int* d_stop = nullptr;  // host-operator loop: codewords whose exact-tau stop fired
  int32_t* d_idx = nullptr;
  double* d_cd = nullptr;  // c_l = sqrt(n Pl_l) in binary64 (joint-decoding glue)
  double P = 0;
  bool power_set = false;
  // per-codeword power allocation (sa_stage_power_batch): c [Bcap][L], P [Bcap]
  void* d_cb = nullptr;
  void* d_Pb = nullptr;
  void* d_P1 = nullptr;  // the shared P = sum(Pl) of set_power (one `real`)
  bool pb_on = false;
  bool shared_power = false;  // sa_stage's Pl staged (c_l of the binary64 glue kernels)
  size_t bytes = 0;
  int last_B = 0, last_T = 0;
  // pinned ring of sa_decide_async: SA_DECIDE_SLOTS slots of dec_cap indices
  int32_t* h_dec = nullptr;
  int32_t* d_dec = nullptr;  // the ring's device address (k_decide writes the slots itself)
  size_t dec_cap = 0;
  hipEvent_t dec_ev[SA_DECIDE_SLOTS] = {};
  int dec_B[SA_DECIDE_SLOTS] = {};
  // where a queued slot's decisions are: -1 the ring (behind dec_ev), else the
  // h_dec of that lane (behind its ev1: the fused tail wrote them, sa_decide_async enqueued nothing)
  int dec_lane[SA_DECIDE_SLOTS] = {-1, -1, -1, -1};
  // Monte-Carlo stream (sa_mc_stage / sa_mc_run, sa_mc.hip): the staged reps'
  // section indices [mc_cap][L] and noise [mc_cap][n], their decisions and stop
  // indices, the slot state of the refilled batch, and its captured graphs
  int mc_cap = 0, mc_nreps = 0;
  int32_t *d_mc_idx = nullptr, *d_mc_dec = nullptr, *d_mc_its = nullptr;
  double* d_mc_noise = nullptr;
  void *d_mc_y = nullptr, *d_mc_zzp = nullptr;  // the staged reps encoded: y [mc_cap][n], z^2 partials [mc_cap][NZ2]
  // sa_mc_draw: the reps' seeds and sigmas [mc_seed_cap], the generator's error flag
  uint32_t* d_mc_seeds = nullptr;
  double* d_mc_sigma = nullptr;
  int* d_mc_err = nullptr;
  int mc_seed_cap = 0;
  int* d_slots = nullptr;   // [4][slot_cap]: rep, t, done rep, fresh; then ctl {next, live, nreps}
  int slot_cap = 0;
  int* h_mc_live = nullptr;  // pinned ring of the live-slot counts the host polls
  hipEvent_t mc_ev[4] = {};
  std::map<std::tuple<int, int, int, int>, hipGraphExec_t> mc_graphs;
  // host copies of the bucket table inv [L][w] and the Ab table fwd [G][n][4]
  // (build_tables, sa_tables.hip), kept until the batched tables are built from them (ensure_invb)
  std::vector<uint16_t> h_inv, h_fwd;
};

namespace sa {

// Launch of a loop kernel on the context's stream, timed as sa_profile asks
// (plain launch when no profile is running).
template <typename F, typename... Args>
void plaunch(sa_ctx* c, F kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
  if (c->prof && c->prof->dispatch) {
    hipEvent_t a = nullptr, b = nullptr;
    if (c->prof->add(&a, &b) == 0) {
      hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, c->at().stream, a, b, 0u, args...);
      return;
    }
  }
  const int nrep = c->prof ? c->prof->rep : 1;
  for (int r = 0; r < nrep; ++r) kernel<<<grid, block, lds, c->at().stream>>>(args...);
}

// The launches seq() makes on stream s, captured and instantiated as a graph.
template <typename F>
int capture_graph(hipStream_t s, F seq, hipGraphExec_t* out) {
  HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int rc = seq();
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(s, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return fail(SA_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(SA_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  return SA_OK;
}

// ---- the kernel choice of a context (sa_shape.h: plan_for) ---------------------
int dense_parts(const sa_ctx* c, int B);  // sa_dense.hip: Ab partials of the dense A beta (GEMM K splits or GEMV splits)
inline Plan plan_for(const sa_ctx* c, int B) { return plan_for(*c, B, is_dense(*c) ? dense_parts(c, B) : 0); }

// t_b: the Monte-Carlo stream's per-slot iteration indices (SecArgs::tb), else null
template <typename real>
SecArgs<real> sec_args(sa_ctx* c, const Plan& p, int mode, int t, int early_stop, const int* tb = nullptr) {
  SecArgs<real> a;
  const sa_lane& ln = c->at();
  const Tables& tab = c->tab;
  a.inv = tab.inv; a.inv32 = tab.inv32; a.invb = tab.invb; a.invl = tab.invl; a.hs = tab.hs;
  a.fwd = (const ushort4*)tab.fwd; a.fwdb = (const ushort4*)tab.fwdb; a.fwd2 = tab.fwd2; a.fwd3 = tab.fwd3;
  a.c = (const real*)c->d_c;
  a.z = (const real*)ln.d_z; a.beta = (real*)ln.d_beta; a.beta_out = (real*)ln.d_beta; a.out = (real*)c->d_out;
  a.abp = (real*)ln.d_abp; a.bbp = (real*)ln.d_bbp; a.zzp = (const real*)ln.d_zzp;
  a.tau = (real*)ln.d_tau; a.iters = ln.d_iters;
  a.L = c->L; a.M = c->M; a.n = c->n; a.w = c->w; a.nhi = c->nhi; a.G = c->G; a.NZ = p.nz;
  a.T1 = c->Tcap + 1; a.t = t; a.mode = mode; a.early_stop = early_stop;
  a.RS = 1;
  a.pt = 0;
  a.B = 0; a.NC = 0; a.zil = 0; a.gpx = 1 << 20;
  a.cst = c->pb_on ? c->L : 0;
  if (c->pb_on) a.c = (const real*)c->d_cb;
  a.sqrt_n = (real)std::sqrt((double)c->n);
  a.tb = tb;
  a.dead = c->dead;
  a.bzero = 0;
  a.dec = nullptr;
  a.itset = 0;
  a.invp = nullptr; a.fwd2p = nullptr; a.pj = 0;  // set by launch_sec2 for the kernels that read them
  return a;
}

template <typename real>
RowArgs<real> row_args(sa_ctx* c, const Plan& p, int mode, int t, int early_stop, int G, int Gb, const int* tb = nullptr) {
  RowArgs<real> a;
  const sa_lane& ln = c->at();
  a.y = (const real*)ln.d_y; a.z = (real*)ln.d_z; a.z_in = a.z; a.abp = (const real*)ln.d_abp;
  a.bbp = (const real*)ln.d_bbp; a.zzp = (real*)ln.d_zzp; a.tau = (const real*)ln.d_tau;
  a.out = (real*)c->d_out;
  a.n = c->n; a.G = G; a.NZ = p.nz;
  a.Gb = Gb; a.T1 = c->Tcap + 1; a.t = t; a.mode = mode;
  a.early_stop = early_stop;
  // the dense matrix already carries the 1/sqrt(n) of sparc_ldpc.py:143-146
  a.sqrt_n = c->backend != SA_BACKEND_HADAMARD ? (real)1 : (real)std::sqrt((double)c->n);
  a.Pb = c->pb_on ? (const real*)c->d_Pb : (const real*)c->d_P1;
  a.Pbst = c->pb_on ? 1 : 0;
  a.pt = 0;
  a.Bc = 0;
  a.tb = tb;
  a.iters = ln.d_iters;
  a.itset = 0;
  return a;
}

// f(i) for i in [0, count) over the host's cores (at most 16 threads), in
// contiguous blocks of `grain` (callers write disjoint outputs per block)
template <typename F>
void parallel_for(int count, int grain, F f) {
  const int blocks = (count + grain - 1) / grain;
  unsigned nth = std::thread::hardware_concurrency();
  nth = nth == 0 ? 1 : (nth > 16 ? 16 : nth);
  if ((int)nth > blocks) nth = blocks > 0 ? blocks : 1;
  auto run = [&](int t) {
    for (int b = t; b < blocks; b += (int)nth)
      for (int i = b * grain; i < count && i < (b + 1) * grain; ++i) f(i);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < (int)nth; ++t) th.emplace_back(run, t);
  run(0);
  for (auto& x : th) x.join();
}

// ---- defined in sparc_amp.hip ------------------------------------------------
int check_ctx(const sa_ctx* c);
int check_tables(const sa_ctx* c, const char* what);
int dev_alloc(sa_ctx* c, void** p, size_t bytes);
void dev_free(void* p);
using GraphMap = std::map<std::tuple<int, int, int, int>, hipGraphExec_t>;
void graphs_clear(GraphMap& m);
void drop_graphs(sa_ctx* c);  // every lane's, and sa_mc_run's
// decode lanes: wait for every lane; make lane k current; drop lane 1's buffers
// (after waiting for every lane; lane 0 becomes current and keeps the staged y)
int sync_all(sa_ctx* c);
inline void lane_switch(sa_ctx* c, int k) { c->cur = k; }
int lanes_release(sa_ctx* c);
// ---- a lane's tail state (sa_lane: fused_B, row_B, row_T) and its transitions ----
// A new decode begins on the lane (sa_run, sa_profile, sa_mc_run; its buffers
// go): a deferred row step of the lane's previous run is dropped (z starts
// from y again) and that run's fused decisions no longer stand.
inline void tail_begin(sa_lane& l) { l.fused_B = l.row_B = l.row_T = 0; }
// The decode q of B codewords finished issuing on the current lane: what it
// leaves there beside the results, and the layout it leaves d_z in.  Set by
// every run (a replayed graph walks no steps).
inline void tail_issued(sa_ctx* c, int B, const DecodeSeq& q) {
  sa_lane& l = c->at();
  l.fused_B = l.row_B = q.fused ? B : 0;
  l.row_T = q.fused ? q.T : 0;
  c->zil_last = q.zil;
}
// d_beta was rewritten outside a run: it no longer holds the estimate the
// fused decisions were taken from, decisions come from k_decide again.
inline void tail_beta_rewritten(sa_lane& l) { l.fused_B = 0; }
// Take the lane's pending row step: false if there is none, else its decode's
// (B, T), and the lane holds none any more.
inline bool tail_take_row(sa_lane& l, int* B, int* T) {
  if (!l.row_B) return false;
  *B = l.row_B;
  *T = l.row_T;
  l.row_B = l.row_T = 0;
  return true;
}
// row_flush launches lane k's pending row step, if there is one, on its
// stream; tail_settle: that, and beta is about to be rewritten (entry points
// that change the current lane's d_beta and partials)
int row_flush(sa_ctx* c, int k);
inline int tail_settle(sa_ctx* c) {
  tail_beta_rewritten(c->at());
  return row_flush(c, c->cur);
}
// the staged y across lanes: y_sync brings lane k's d_y up to the latest
// staged version (a device-to-device copy on its stream, behind the event
// recorded after the staging); a writer of B codewords of lane k's d_y on
// stream s calls y_begin_write before it launches and y_mark after (when s is
// not the lane's own stream: after waiting for s).  Without k: the current lane.
int y_sync(sa_ctx* c, int k);
int y_begin_write(sa_ctx* c, int k, hipStream_t s, int B);
int y_mark(sa_ctx* c, int k);
inline int y_sync(sa_ctx* c) { return y_sync(c, c->cur); }
inline int y_begin_write(sa_ctx* c, hipStream_t s, int B) { return y_begin_write(c, c->cur, s, B); }
inline int y_mark(sa_ctx* c) { return y_mark(c, c->cur); }
int ensure_workspace(sa_ctx* c, int B, int T);
// host fp64 <-> a device `real` buffer through lane l's staging buffer, on its
// stream.  Without l: the current lane.
int ensure_stage(sa_ctx* c, sa_lane& l, size_t count);
int upload(sa_ctx* c, sa_lane& l, void* dst, const double* src, size_t count);
int download(sa_ctx* c, sa_lane& l, double* dst, const void* src, size_t count);
inline int ensure_stage(sa_ctx* c, size_t count) { return ensure_stage(c, c->at(), count); }
inline int upload(sa_ctx* c, void* dst, const double* src, size_t count) { return upload(c, c->at(), dst, src, count); }
inline int download(sa_ctx* c, double* dst, const void* src, size_t count) { return download(c, c->at(), dst, src, count); }
int set_power(sa_ctx* c, const double* Pl);
int create_impl(sa_ctx** out, int L, int M, int n, const uint32_t* ordering, int backend, int prec, int device,
                int plan, const sa_ctx* share = nullptr);
extern __global__ void k_fill32(uint32_t* p, uint32_t v, size_t nw);

// ---- sa_tables.hip: the operator tables ------------------------------------------
int build_tables(sa_ctx* c);   // inv / fwd / fwd2 / fwd3 from the ordering, which it validates
int ensure_invb(sa_ctx* c);    // k_secb's tables (fwdb, invb, hs, invl), built at its first use
void tables_free(Tables& t);

// ---- sa_sec.hip: the single-codeword section kernels ---------------------------
template <typename real>
int launch_sec(sa_ctx* c, const Plan& p, int B, int mode, int t, int es, void* bin = nullptr, void* bout = nullptr);
template <typename real>
int launch_sec2(sa_ctx* c, const Plan& p, int B, int t, int es, void* bin, void* bout, int bzero = 0,
                int32_t* dec = nullptr, int itset = 0);  // dec, itset: the fused tail's last launch (SecArgs::dec)
hipError_t sec_lds_attrs();

// ---- sa_secb.hip: the batched section kernel ------------------------------------
template <typename real>
int launch_secb(sa_ctx* c, const Plan& p, int B, int t, int es, const int* tb = nullptr);
hipError_t secb_lds_attrs();
bool secb_no_static_lds();

// ---- sa_row.hip: row kernels, decisions ----------------------------------------
// G, Gb: the partial counts of whatever produced abp / bbp for this launch
// (the plan's for the loop; the beta0 start, the host loop and the
// Monte-Carlo stream pass their own).  ROW_ABOUT is always k_row.
template <typename real>
int launch_row(sa_ctx* c, const Plan& p, int B, int mode, int t, int es, int G, int Gb, int itset = 0,
               const int* tb = nullptr);
int launch_decide(sa_ctx* c, int B, int32_t* idx);  // idx: device-visible [B][L]
// ---- sa_row2.hip: k_row2 (R rows per workgroup) out of launch_row's RowArgs ------
template <typename real, int R>
int launch_row2(sa_ctx* c, const Plan& p, int B, const RowArgs<real>& a);

// ---- sa_dense.hip: the materialised-matrix backends ----------------------------
int dense_den_groups(const sa_ctx* c);
template <typename real>
int dense_start(sa_ctx* c, const Plan& p, int B);  // z = y - A beta0 (the beta0 start)
template <typename real>
int dense_iter(sa_ctx* c, const Plan& p, int B, int t, int es);  // A^T z -> denoiser -> A beta partials
template <typename real>
int dense_ab(sa_ctx* c, const Plan& p, int B);  // A beta of d_beta -> d_out
template <typename real>
int dense_az(sa_ctx* c, const Plan& p, int B);  // A^T z of d_z -> d_out
int ensure_i8(sa_ctx* c, int B);
int ensure_fgemm(sa_ctx* c, int B);
int i8_set_bfix(sa_ctx* c);
int build_dense(sa_ctx* c);
int matrix_init(sa_ctx* c);  // a caller's matrix: padded layout, zeroed d_A
hipError_t dense_lds_attrs();

// ---- sa_mc.hip: the Monte-Carlo rep stream ------------------------------------
void mc_release(sa_ctx* c);  // its buffers and graphs (sa_destroy)
hipError_t mc_lds_attrs();

#ifdef SA_STAMPS
hipError_t stamps_add_sec(unsigned long long* out);   // adds the unit's s_memtime stamps into out
hipError_t stamps_add_secb(unsigned long long* out);
#endif

}  // namespace sa
