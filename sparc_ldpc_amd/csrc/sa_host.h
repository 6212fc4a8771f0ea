// sa_host.h — the operator context (sa_ctx), launch timing and the host-side
// helpers shared by the kernel units and the C ABI (sparc_amp.hip).
#pragma once
#include "sa_common.h"

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
  void *d_bbp = nullptr, *d_zzp = nullptr, *d_tau = nullptr;
  void* d_beta2 = nullptr;  // ping-pong partner of d_beta for k_sec (B x L*M), sized beta2_cap
  int* d_iters = nullptr;
  double* d_stage = nullptr;  // a lane's uploads go through its own staging buffer
  size_t stage_cap = 0;
  int beta2_cap = 0;
  std::map<std::tuple<int, int, int, int>, hipGraphExec_t> graphs;  // their kernel arguments hold the lane's pointers
  hipEvent_t y_ev = nullptr;      // behind the last write of this lane's d_y (staging, or the copy from the other lane)
  unsigned long long y_ver = 0;   // version of the y this lane holds (sa_ctx::y_ver: the latest staged)
  bool y_read = false;            // this lane's last y copy read the other lane's d_y (that lane's next y write waits for y_ev)
  // Fused tail (fused_tail below): the lane's last run ended with its last
  // section launch, which wrote the decisions of fused_B codewords into h_dec
  // (pinned, device-mapped at d_dec, Bcap x L; marked by ev1), and left the
  // row step of iteration row_T - 1 of row_B codewords undone: nothing of the
  // decode, its decisions or its estimate reads z_T.  row_flush launches that
  // step for whoever reads d_z / d_zzp, or is about to change what it reads
  // (y, the power, the partials); the lane's next run drops it.
  int32_t *h_dec = nullptr, *d_dec = nullptr;
  int fused_B = 0;
  int row_B = 0, row_T = 0;
};

struct sa_ctx {
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
  int L = 0, M = 0, n = 0, w = 0, nhi = 0, backend = 0, prec = 0, device = 0;
  int plan = 0;       // SA_PLAN_* options of sa_create_ex (0: every choice by the built-in rules)
  bool pow2 = true;  // M a power of two (the Hadamard kernels, bit-level glue)
  // the caller's section size Mu; the Hadamard backend pads a section of any
  // Mu to M = 2^ceil(log2 Mu) columns, the first dead = M - Mu of them never
  // used (column c of the reference is column dead + c: sparc_ldpc.py:54, 68)
  int Mu = 0, dead = 0;
  int G = 0, NZ = 0, E = 1;
  int n_cus = 256;
  int Gb = 0, CB = 0;  // batched kernel: groups of WB sections, codewords per workgroup (0 = off)
  int WB = 8;          // batched kernel: sections per workgroup (kWB or kWB16)
  int gpx = 1 << 20;   // batched kernel: section groups per XCD per pass (SecArgs::gpx)
  size_t secb_lds = 0;
  int RS = 1, KS = 1, Gd = 0;  // dense splits; Gd = dense denoiser groups
  size_t lda = 0;
  size_t sec_lds = 0;
  int G2 = 0;          // k_sec2 pairs of sections (0: k_sec2 unavailable)
  int G3 = 0;          // k_sec43 triples of sections (used when sec3)
  bool sec3 = false;   // k_sec43 (three sections x 4 waves per workgroup) chosen over k_sec4
  size_t sec3_lds = 0;
  int G4 = 0;          // k_sec44 quads of sections (used when sec4q)
  bool sec4q = false;  // k_sec44 (four sections x 4 waves per workgroup, the pair table) chosen over k_sec4
  size_t sec4q_lds = 0;
  uint32_t* d_fwd3 = nullptr;
  bool pt_on = false;  // row-block-major Ab partials between k_sec4 / k_sec43 and k_row2 (SecArgs::pt)
  bool sec4 = false;   // k_sec4 (4 waves per section) fits and is chosen
  size_t sec4_lds = 0;
  int NZ16 = 0;        // k_row2 32-row blocks
  int NZh = 0;         // k_row2 16-row blocks (row16)
  bool row16 = false;  // k_row2<16> after k_sec4 (row-block-major partials, NZh <= 320)
  int NZ4 = 0, NZ2 = 0;  // k_rowv<4> 256-row / k_rowv<2> 128-row blocks
  // (describes one lane's d_z, yet stays here: in the lane, sa_fetch_z after sa_mc_stage would answer differently)
  bool zil_last = false;  // the last decode left z codeword-interleaved ([NC][n][CB], zil_for)
  size_t sec2_lds = 0;
  std::vector<uint32_t> ordering;
  uint16_t* d_inv = nullptr;
  // operators whose z does not fit the section kernels' LDS (n >= 65535, or
  // the z image past 160 KB): k_secg with 32-bit bucket entries, no batched /
  // multi-wave kernels
  bool big = false;
  uint32_t* d_inv32 = nullptr;
  uint16_t* d_invb = nullptr;  // k_secb's bank-aware bucket table (build_invb), built on first batched use
  uint16_t* d_fwdb = nullptr;  // k_secb's Ab table, bank-aware step order per row (build_fwdb), the same
  uint16_t* d_invl = nullptr;  // the codeword-interleaved k_secb's bucket table, lane-major (k_lane_major)
  uint32_t* d_hs = nullptr;    // [L] occupied steps of d_invb's halves (build_banked)
  bool borrowed = false;       // the operator tables are another context's (sa_create_twin): not freed here
  bool invb_done = false;
  uint16_t* d_fwd = nullptr;
  uint32_t* d_fwd2 = nullptr;
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
  // (build_tables), kept until the batched tables are built from them (ensure_invb)
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

// ---- backend / kernel choice rules (shared by the units) --------------------
constexpr int kI8MinB = 4;   // dense backend: batches at least this large take the int8 GEMM path
constexpr int kI8MaxS = 16;  // K splits of the int8 A beta GEMM (its Ab partials)
constexpr int kFMinB = 4;    // matrix backend: batches at least this large take the f32 / f64 GEMM path
constexpr int kFMaxS = 16;   // K splits of its A beta GEMM

inline size_t rsz(const sa_ctx* c) { return c->prec == SA_PREC_F64 ? 8 : 4; }

// the dense backends: a materialised n x (L*M) matrix streamed by GEMVs
// (the Hadamard design's, or a caller's own: SA_BACKEND_MATRIX)
inline bool is_dense(const sa_ctx* c) { return c->backend == SA_BACKEND_DENSE || c->backend == SA_BACKEND_MATRIX; }
inline bool use_i8(const sa_ctx* c, int B) { return c->backend == SA_BACKEND_DENSE && B >= kI8MinB; }
inline bool use_fgemm(const sa_ctx* c, int B) { return c->backend == SA_BACKEND_MATRIX && B >= kFMinB; }
inline bool use_batched(const sa_ctx* c, int B) { return c->CB > 0 && B >= 4; }

// The batched decode with z and the Ab partials interleaved by codeword chunk
// (SecArgs::zil, 16-byte rows of CB codewords: binary32 CB = 4, binary64
// CB = 2), row kernel k_rowc.  The default in binary32 (C3 +1.7 %, C4
// +4.7 %) and, since the binary64 k_secb no longer spills (round 4: one
// bucket h-step in flight, 16-byte non-temporal beta), in binary64 too (C3
// 6.30 k -> 6.44 k, C4 3.09-3.12 k -> 3.19 k cw/s; round 3's spilling kernel
// lost 1.6 %); SA_PLAN_NO_ZIL keeps [B][n]
inline bool zil_for(const sa_ctx* c, int B) {
  const bool on = (c->plan & SA_PLAN_NO_ZIL) ? false : true;
  return on && c->backend == SA_BACKEND_HADAMARD && use_batched(c, B) && c->CB * (int)rsz(c) == 16;
}

int dense_parts(const sa_ctx* c, int B);  // sa_dense.hip: Ab partials of the dense A beta (GEMM K splits or GEMV splits)

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
inline Plan plan_for(const sa_ctx* c, int B) {
  Plan p;
  const bool f32 = c->prec == SA_PREC_F32;
  p.zil = zil_for(c, B);
  if (p.zil) {
    p.row = SA_ROW_K_ROWC; p.nz = c->NZ2;  // 128-row blocks
  } else if ((long long)B * c->NZ < 4LL * c->n_cus) {
    if (c->row16 && B == 1) { p.row = SA_ROW_K_ROW2_16; p.nz = c->NZh; }
    else { p.row = SA_ROW_K_ROW2; p.nz = c->NZ16; }
  } else if (c->n % (f32 ? 4 : 2) == 0 && (long long)B * (f32 ? c->NZ4 : c->NZ2) >= 2LL * c->n_cus) {
    // 16-byte rows: binary32 n % 4 == 0 (256-row blocks) or binary64 n even (128)
    p.row = SA_ROW_K_ROWV16; p.nz = f32 ? c->NZ4 : c->NZ2;
  } else if (f32 && c->n % 2 == 0 && (long long)B * c->NZ2 >= 2LL * c->n_cus) {
    p.row = SA_ROW_K_ROWV8; p.nz = c->NZ2;
  } else {
    p.row = SA_ROW_K_ROW; p.nz = c->NZ;
  }
  const int wgs = c->G * B;  // k_sec / k_secg: enough row splits to cover every CU
  p.rs = std::min(4, std::max(1, (c->n_cus + wgs - 1) / wgs));
  if (is_dense(c)) {
    p.sec = use_i8(c, B) ? SA_SEC_DENSE_I8 : (use_fgemm(c, B) ? SA_SEC_MATRIX : SA_SEC_DENSE);
    p.G = dense_parts(c, B);
    p.Gb = c->Gd;
  } else if (use_batched(c, B)) {
    p.sec = SA_SEC_K_SECB;
    p.G = p.Gb = c->Gb;
    p.CB = c->CB;
  } else if (c->backend == SA_BACKEND_HADAMARD && c->G2 > 0 && c->G2 * B * 2 >= c->n_cus) {
    p.sec = c->sec3 ? SA_SEC_K_SEC43 : (c->sec4q ? SA_SEC_K_SEC44 : (c->sec4 ? SA_SEC_K_SEC4 : SA_SEC_K_SEC2));
    p.G = p.Gb = c->sec3 ? c->G3 : (c->sec4q ? c->G4 : c->G2);  // triples / quads / pairs of sections
    if (p.sec != SA_SEC_K_SEC2 && p.row_sets_iters() && c->pt_on) p.pt = p.row == SA_ROW_K_ROW2_16 ? 16 : kRow2Rows;
  } else {
    p.sec = c->big ? SA_SEC_K_SECG : SA_SEC_K_SEC;
    p.G = p.Gb = c->G;
  }
  return p;
}

// Fused tail of a decode: with the early stop off the last launch is known at
// capture time, so the last section launch of the pair / triple / quad kernels
// also writes the section decisions and iters (SecArgs::dec, itset), k_decide
// is never launched, and the last k_row2 step, whose z_T only sa_fetch_z
// reads, is deferred (sa_lane::row_B).  Depends on (context, B, T, flags) alone.
inline bool fused_tail(const sa_ctx* c, const Plan& p, int T, int flags) {
  return p.bzero() && p.it_row() && (flags & SA_FLAG_NO_EARLY_STOP) && T > 0 && c->dead == 0 && !c->prof &&
         !(c->plan & SA_PLAN_NO_FUSED_TAIL);
}

// t_b: the Monte-Carlo stream's per-slot iteration indices (SecArgs::tb), else null
template <typename real>
SecArgs<real> sec_args(sa_ctx* c, const Plan& p, int mode, int t, int early_stop, const int* tb = nullptr) {
  SecArgs<real> a;
  const sa_lane& ln = c->at();
  a.inv = c->d_inv; a.inv32 = c->d_inv32; a.invb = c->d_invb; a.invl = c->d_invl; a.hs = c->d_hs;
  a.fwd = (const ushort4*)c->d_fwd;
  a.fwdb = (const ushort4*)c->d_fwdb; a.fwd2 = c->d_fwd2; a.fwd3 = c->d_fwd3; a.c = (const real*)c->d_c;
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
// fused tail: launch lane k's deferred row step, if one is pending, on its
// stream; tail_settle: that, and the lane's fused decisions no longer stand
// for its d_beta (entry points that change the current lane's buffers)
int row_flush(sa_ctx* c, int k);
inline int tail_settle(sa_ctx* c) {
  c->at().fused_B = 0;
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
int ensure_invb(sa_ctx* c);
int create_impl(sa_ctx** out, int L, int M, int n, const uint32_t* ordering, int backend, int prec, int device,
                int plan, const sa_ctx* share = nullptr);
extern __global__ void k_fill32(uint32_t* p, uint32_t v, size_t nw);

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
