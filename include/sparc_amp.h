/*
 * sparc_amp.h — C ABI of the MI355X (gfx950) SPARC AMP decoder.
 *
 * Library: sparc_ldpc_amd/libsparc_amp.so (hipcc --offload-arch=gfx950).
 *
 * The reference (Spimp/sparc_ldpc) has no native boundary on this path: the
 * whole AMP decoder is Python/NumPy.  These entry points replace the Python
 * functions named on each declaration, with the reference's own native
 * boundary conventions (ldpc/py/ldpc.py:859-929 -> ldpc/src/c_ldpc.c:32-113):
 * plain pointers and sizes, caller-allocated outputs, int status returns,
 * no Python objects across the ABI.  fp64 at the ABI (the reference computes
 * in fp64); fp32 or fp64 on the device (precision argument of sa_create).
 *
 * Status codes: 0 = OK, < 0 = error (sa_last_error() describes the last one
 * raised on the calling thread).  A context is bound to one device and one
 * HIP stream; it is not thread-safe, but contexts on different devices may be
 * driven concurrently from different threads.
 */
#ifndef SPARC_AMP_H
#define SPARC_AMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_ctx sa_ctx;

enum {
  SA_OK = 0,
  SA_ERR_ARG = -1,          /* bad size / shape / pointer (reference: AssertionError) */
  SA_ERR_HIP = -2,          /* HIP runtime failure */
  SA_ERR_NOMEM = -3,        /* device allocation failed (reference: c_ldpc.c:40-42 -> -1) */
  SA_ERR_ORDERING = -4,     /* ordering row not distinct / out of [1, w) */
  SA_ERR_UNSUPPORTED = -5,  /* configuration outside this backend's limits */
  SA_ERR_NO_DEVICE = -6     /* no HIP device visible */
};

enum {
  SA_BACKEND_HADAMARD = 0,  /* matrix-free sub-sampled Walsh-Hadamard operator (default) */
  SA_BACKEND_DENSE = 1,     /* materialised n x (L*M) design matrix: fp32 GEMVs for B < 4
                               codewords, int8 matrix-core GEMMs on exact +-1 entries with
                               three-digit fixed-point vectors for B >= 4 */
  SA_BACKEND_HOST = 2,      /* no device operator: the caller's own Ab / Az (any operator, as the
                               reference's amp() accepts any callables) applied on the host, the
                               loop's tau, denoiser and residual on the device (sa_host_*) */
  SA_BACKEND_MATRIX = 3     /* a caller's own dense n x (L*M) design matrix (e.g. i.i.d. Gaussian;
                               sa_create_matrix) held on the device in the context precision:
                               GEMVs for B < 4 codewords, f32 / f64 MFMA GEMMs for B >= 4 */
};

enum { SA_PREC_F32 = 0, SA_PREC_F64 = 1 };

/* sa_amp / sa_run flags */
enum {
  SA_FLAG_NO_EARLY_STOP = 1, /* run exactly T iterations (ignore the tau == last_tau stop) */
  SA_FLAG_BETA0 = 0x100,     /* sa_run: start from the beta0 staged by sa_stage */
  SA_PTR_DEVICE = 0x200      /* sa_llr / sa_soft_beta0 / sa_hard_cancel: llr / app are device pointers */
};

/* Replaces sparc_transforms(L, M, n, seed) / block_sub_fht(n, M, L, ordering)
 * (ldpc/sparc_ldpc.py:140-147, :81-136): builds the design operator of L
 * sections of M columns over n rows from `ordering` (L x n, row-major,
 * values in [1, w), w = 2^ceil(log2(max(M+1, n+1))), distinct per row) on
 * `device`.  The ordering itself is generated on the host by the caller with
 * the reference's RandomState algorithm (sparc_ldpc.py:107-117). */
int sa_create(sa_ctx** out, int L, int M, int n, const uint32_t* ordering,
              int backend, int precision, int device);

/* sa_create with plan options: which kernels and layouts a decode uses is
 * normally chosen by built-in rules from (L, M, n, precision, batch, CUs)
 * (sa_plan reports the choice); these bits override a rule, e.g. to test a
 * kernel on shapes where the rule would not pick it.  Every option keeps the
 * results within the same parity bounds; SA_PLAN_NO_PT, SA_PLAN_EAGER,
 * SA_PLAN_ONE_PASS, SA_PLAN_NO_LANES, SA_PLAN_NO_FUSED_TAIL and SA_PLAN_NO_PACK are bit-identical to the default plan.  `sa_subset` contexts
 * inherit their parent's options. */
enum {
  SA_PLAN_DEFAULT = 0,
  SA_PLAN_SEC3 = 1 << 0,      /* one codeword: three sections per workgroup (k_sec43) where it fits */
  SA_PLAN_NO_SEC3 = 1 << 1,   /* one codeword: never k_sec43 (pairs, k_sec4, in front of 16-row blocks in binary32) */
  SA_PLAN_ROW16 = 1 << 2,     /* one codeword: 16-row k_row2 blocks where they fit (the binary32 default, except at L = 2 x CUs) */
  SA_PLAN_NO_ROW16 = 1 << 3,  /* one codeword: 32-row k_row2 blocks (the default in binary64, and at L = 2 x CUs) */
  SA_PLAN_NO_PT = 1 << 4,     /* Ab partials [G][n] instead of row-block major (bit-identical) */
  SA_PLAN_ZIL = 1 << 5,       /* batched: z / Ab partials codeword-interleaved (the default since round 4) */
  SA_PLAN_NO_ZIL = 1 << 6,    /* batched: z / Ab partials [B][n] (binary32 too) */
  SA_PLAN_WB8 = 1 << 7,       /* batched: 8 sections per workgroup */
  SA_PLAN_WB16 = 1 << 8,      /* batched: 16 sections per workgroup */
  SA_PLAN_NO_BANKS = 1 << 9,  /* batched: bucket slots summed in h order (no bank-aware slot order) */
  SA_PLAN_EAGER = 1 << 10,    /* sa_run launches eagerly instead of replaying a captured hipGraph */
  SA_PLAN_ONE_PASS = 1 << 11, /* batched: every section group of an XCD in one pass of the work order */
  SA_PLAN_NO_LANES = 1 << 12, /* every sa_run on one stream and one set of state buffers (no decode lanes) */
  SA_PLAN_SEC4Q = 1 << 13,    /* one codeword: four sections per workgroup (k_sec44) wherever pairs would run, M <= 512
                                 (never chosen by the rules: faster with two decodes in flight, slower alone) */
  SA_PLAN_NO_SEC4Q = 1 << 14, /* one codeword: never k_sec44 (the default; overrides SA_PLAN_SEC4Q) */
  SA_PLAN_NO_FUSED_TAIL = 1 << 15, /* one codeword, early stop off: keep the decode's last k_row2 launch and decide
                                      with k_decide (no decisions out of the last section launch; bit-identical) */
  SA_PLAN_NO_PACK = 1 << 16,  /* one codeword, pairs / quads: the 16-bit bucket table and the 32-bit pair Ab table
                                 instead of their packed forms (13-bit bucket records; pairs: three rows per
                                 64-bit word), which are then not built (bit-identical) */
  SA_PLAN_ALL = (1 << 17) - 1
};
int sa_create_ex(sa_ctx** out, int L, int M, int n, const uint32_t* ordering,
                 int backend, int precision, int device, int plan);

/* A caller's own dense design (the reference's amp() with any pair of
 * callables, sparc_ldpc.py:189,213,220, e.g. Ab = lambda b: A @ b,
 * Az = lambda z: A.T @ z for an i.i.d. Gaussian A): A is n x (L*M) row-major
 * binary64, copied to the device in `precision`; the context's sa_Ab / sa_Az
 * compute A beta / A^T z (no 1/sqrt(n): the matrix is used as given) and
 * sa_amp / sa_run run the whole loop on the device.  Section sizes M need not
 * be powers of two.  sa_encode / sa_cancel / sa_subset need an ordering
 * (SA_ERR_UNSUPPORTED here). */
int sa_create_matrix(sa_ctx** out, int L, int M, int n, const double* A,
                     int precision, int device);

/* The same backend with an i.i.d. N(0, scale^2) design generated on the
 * device (e.g. scale = 1/sqrt(n): unit-norm columns on average) for
 * simulations that never need the matrix on the host: Philox4x32-10 keyed by
 * `seed`, counter = row-major element index / 4, Box-Muller; reproducible per
 * (seed, element), not NumPy's stream. */
int sa_create_matrix_random(sa_ctx** out, int L, int M, int n, uint64_t seed, double scale,
                            int precision, int device);

/* Replaces sparc_transforms_shorter(L, M, n, ordering[sections])
 * (ldpc/sparc_ldpc.py:154-168; called with a fancy-indexed subset at
 * ldpc/amp_exit.py:113-116): a new context over the given parent sections. */
int sa_subset(const sa_ctx* parent, const int64_t* sections, int Ls, sa_ctx** out);

/* A second context over src's operator (the same L, M, n, ordering, backend,
 * precision, device and plan) that shares src's device tables, read-only,
 * and has its own stream, workspace and power allocation: concurrent decodes
 * of one operator (joint.JointPipeline's slices) read one copy of the tables
 * from L2.  src must outlive the twin.  Hadamard backend only. */
int sa_create_twin(sa_ctx* src, sa_ctx** out);

void sa_destroy(sa_ctx* ctx);

/* Replaces the Ab closure, sparc_ldpc.py:143-144 (-> block_sub_fht.Ax
 * :120-126): out[b] = A beta[b] for B codewords.  beta: B x (L*M), out: B x n. */
int sa_Ab(sa_ctx* ctx, int B, const double* beta, double* out);

/* Replaces the Az closure, sparc_ldpc.py:145-146 (-> block_sub_fht.Ay
 * :128-134): out[b] = A^T z[b].  z: B x n, out: B x (L*M). */
int sa_Az(sa_ctx* ctx, int B, const double* z, double* out);

/* Replaces amp(y, sigma_n, Pl, L, M, T, Ab, Az, beta) (sparc_ldpc.py:189-222)
 * and amp_test (ldpc/amp_test.py:14-50) for B independent codewords sharing
 * the operator: y: B x n; Pl: L section powers; beta0: B x (L*M) or NULL for
 * the zero start; beta_out: B x (L*M); iters_out (may be NULL): per codeword
 * the loop index at which the exact tau == last_tau stop fired, or T when
 * the loop ran to completion.  sigma_n is not an argument: the reference
 * never reads it. */
int sa_amp(sa_ctx* ctx, int B, const double* y, const double* Pl, int T,
           const double* beta0, double* beta_out, int* iters_out, int flags);

/* ---- device-resident path (bench / Monte-Carlo harness) ----------------
 * sa_reserve sizes the device workspace for B codewords and T iterations
 * (it discards staged data when it has to grow) and builds the tables a
 * decode of B codewords needs that are built lazily (the batched kernel's
 * bank-aware tables, once per operator); sa_stage copies y (and Pl, and optionally beta0) into the context's device
 * buffers; sa_run decodes the staged batch asynchronously on the context's
 * stream (replayed hipGraph); sa_wait blocks until it is done; sa_fetch
 * copies the results back.  sa_run_event_ms returns the device time of the
 * last sa_run measured with HIP events on the context's stream: from the start
 * of its graph to the end of the graph's last kernel (with the fused tail, see
 * sa_decide_async, the section decisions lie inside that span and the last
 * residual update, deferred, outside it).
 *
 * Decode lanes.  A context holds two lanes, each a stream plus everything one
 * decode mutates (y, z, both beta buffers, the partials, tau, iters, the
 * captured graphs); the tables, the power arrays and the sa_decide_async ring
 * are shared.  A small-batch decode (Hadamard backend, fewer than 4 codewords
 * or no batched kernel, graph mode, no SA_FLAG_BETA0, no SA_PLAN_NO_LANES)
 * issued while the previous step is still outstanding (its decode in flight,
 * or decisions queued by sa_decide_async and not yet collected) takes the lane
 * the previous sa_run did not take, so sa_run(k + 1) overlaps sa_run(k) on the
 * chip when the caller collects one step behind (sa_decide_async /
 * sa_decide_collect); every other run, a lone decode (sa_run, sa_wait)
 * among them, stays on the lane of the previous one and is the single-lane
 * decode.  The second lane is created at the first run that takes it; at
 * L = M = 512, n = 4608, one codeword, binary32 it costs about 4.7 MB of
 * partials, 2 x 1 MB of beta and the small buffers (sa_info's byte count
 * includes it).  Batched, dense, matrix, host-operator, eager and NO_LANES
 * contexts never get a second stream or workspace.  What holds:
 *  - each sa_run decodes the inputs staged most recently before it; without an
 *    sa_stage since the previous run it decodes the same y again.  sa_stage
 *    does not wait for a decode in flight: y goes into the lane the next
 *    run is expected to take, on that lane's stream (a run that finds its lane's y
 *    older than the latest staged one copies it over on the device first).
 *    beta0 and the SA_FLAG_BETA0 run stay on the lane of the previous run;
 *  - sa_decide_async, sa_decide, sa_fetch, sa_fetch_z, sa_run_event_ms and the
 *    glue calls (sa_llr, ...) refer to the most recent sa_run and are ordered
 *    behind it on its lane's stream;
 *  - sa_wait, sa_destroy, sa_reserve when it grows the workspace and a changed
 *    Pl wait for every lane; an sa_stage whose Pl equals the staged one writes
 *    nothing to the device;
 *  - results are bit-identical to a single-lane context's. */
int sa_reserve(sa_ctx* ctx, int B, int T);
int sa_stage(sa_ctx* ctx, int B, const double* y, const double* Pl, const double* beta0);
/* Per-codeword power allocations Pl [B][L] (Hadamard backend) for the next
 * sa_run of up to B codewords: c_{b,l} = sqrt(n Pl_{b,l}), P_b = sum_l Pl_{b,l}
 * (sparc_ldpc.py:190,214).  Sections with Pl = 0 keep beta = 0 and drop out
 * of A beta, so this is the reference's shortened-operator decode
 * (sparc_transforms_shorter, amp_exit.py:113-116) as a per-codeword section
 * mask.  The binary64 glue kernels (sa_llr, ...) keep the c_l of the last
 * sa_stage Pl; a later sa_stage with Pl returns to one allocation. */
int sa_stage_power_batch(sa_ctx* ctx, int B, const double* Pl);
int sa_run(sa_ctx* ctx, int B, int T, int flags);
int sa_wait(sa_ctx* ctx);
int sa_fetch(sa_ctx* ctx, int B, double* beta_out, int* iters_out);
/* The residual z of the last decode's final iteration, B x n (diagnostics).
 * A one-codeword decode with the early stop off leaves its last residual
 * update undone (nothing of the decode, its estimate or its decisions reads
 * z_T); this call, and any call that changes what the update reads (a new y,
 * a new power allocation), launches it first, and the lane's next sa_run drops it. */
int sa_fetch_z(sa_ctx* ctx, int B, double* z_out);
/* The staged y, B x n, widened to binary64: what the next sa_run would read
 * (sa_stage's, or what sa_encode, sa_hard_cancel with dst or sa_cancel left
 * as this context's input).  With two lanes live, the current lane's y is
 * first brought up to the latest staged one, as a run does; no kernel other
 * than the binary32 widening is launched and no layout changes. */
int sa_fetch_y(sa_ctx* ctx, int B, double* y_out);
double sa_run_event_ms(sa_ctx* ctx);

/* Per-kernel device time of one EAGER decode of the staged batch (every
 * launch bracketed by HIP events on the context's stream).  out[13]:
 * {mean ms, launches} for kernel kinds 0 section (k_sec), 1 row (k_row),
 * 2 dense A^T z (fp32 GEMV; int8 MFMA GEMM for B >= 4), 3 dense denoiser,
 * 4 dense A beta (GEMV; int8 MFMA GEMM for B >= 4), 5 int8 digit-plane
 * quantisation of z / beta0; out[12] = total ms of the sequence.  Leaves the
 * decode's results in place like sa_run. */
int sa_profile(sa_ctx* ctx, int B, int T, int flags, double* out);
/* Number of kernel kinds K of sa_profile / sa_profile_rep: `out` holds 2 K + 1
 * doubles (K = 6 since SA_VERSION 0.2: size buffers from this, not a constant). */
int sa_profile_kinds(void);
/* The same with every bracketed launch issued `rep` (1..1024) times back to
 * back between its events: mean = elapsed / rep, i.e. the launch's duration
 * plus the same-stream kernel boundary, without the event packets' dispatch
 * overhead.  The results left in place are then those of repeated
 * launches (not a decode); re-run sa_run before fetching. */
int sa_profile_rep(sa_ctx* ctx, int B, int T, int flags, int rep, double* out);
/* The same eager decode with every loop kernel launched once through
 * hipExtLaunchKernel with a start / stop event pair bound to the kernel's own
 * dispatch: {mean ms, launches} per kind is the kernels' execution time in
 * the decode's order (what a rocprofv3 kernel trace records), with no marker
 * packets between the launches.  Leaves the decode's results in place. */
int sa_profile_dispatch(sa_ctx* ctx, int B, int T, int flags, double* out);

/* Per-codeword section decisions (sparc_ldpc.py:452-455: argmax per
 * section, first index on ties) of the last sa_run / sa_amp, computed on
 * device: idx_out is B x L. */
int sa_decide(sa_ctx* ctx, int B, int32_t* idx_out);

/* The same decision, pipelined: sa_decide_async enqueues the argmax and the
 * copy of its B x L indices into slot `slot` (0 .. SA_DECIDE_SLOTS-1) of a
 * context-owned pinned host ring behind the work already on the stream and
 * returns at once; sa_decide_collect waits for that slot's copy only and
 * hands its indices to the caller (idx_out: B x L).  A decoder loop queues
 * decode k + 1 before it collects the decisions of decode k, so the device
 * never waits on the host.
 *
 * Fused tail.  A one-codeword decode on the pair / triple / quad section
 * kernels with k_row2, SA_FLAG_NO_EARLY_STOP, T > 0 and M a power of two takes
 * the decisions in its last section launch (the argmax of the estimate that
 * launch stores, the same rule) and writes them into a pinned buffer of its
 * lane: sa_decide_async then enqueues nothing, the slot remembers the lane, and
 * sa_decide_collect waits for the end of that decode (the event
 * sa_run_event_ms reads) and copies from the lane.  A later sa_run on that lane
 * first moves uncollected decisions into the slot, on the lane's stream.  Any
 * number of slots may be queued before the first collect; each yields its own
 * step's decisions.  SA_PLAN_NO_FUSED_TAIL keeps the separate argmax launch. */
enum { SA_DECIDE_SLOTS = 4 };
int sa_decide_async(sa_ctx* ctx, int B, int slot);
int sa_decide_collect(sa_ctx* ctx, int B, int slot, int32_t* idx_out);

/* ---- SPARC <-> LDPC glue of the joint decoder (sparc_ldpc.py:359-712) ---
 * Binary64 kernels on the staged batch; llr / app arrays are [B][ns*log2 M]
 * (the LDPC bits of sections l0 .. l0+ns-1, MSB first) and may be device
 * pointers shared with libldpc_bp.so (flag SA_PTR_DEVICE). */

/* Encoder (sparc_ldpc.py:436-446): y[b] = A beta(idx[b]) + noise[b] staged as
 * the decode input, beta(idx) one-hot with c_l = sqrt(n Pl_l) at column
 * idx[b][l] of section l.  idx: B x L; noise: B x n or NULL.  Needs Pl staged
 * (sa_stage(ctx, B, NULL, Pl, NULL)). */
int sa_encode(sa_ctx* ctx, int B, const int32_t* idx, const double* noise);

/* The encoder from message bits that are on the device already (the reps
 * lb_joint_draw of libldpc_bp.so draws): d_bits [B][L log2 M] bytes, section l
 * taking bits [l log2 M, (l + 1) log2 M) MSB first (bits2indices,
 * sparc_ldpc.py:317), d_noise [B][n] binary64 or NULL; both device pointers on
 * the context's device, their producer finished.  Forms idx on the device and
 * stages y exactly as sa_encode stages it from the same idx and noise (the
 * same kernel), bit for bit.  idx_out: B x L on the host, or NULL.  M not a
 * power of two: SA_ERR_UNSUPPORTED; d_bits NULL or B <= 0: SA_ERR_ARG.  Needs
 * Pl staged.  Blocking. */
int sa_encode_bits(sa_ctx* ctx, int B, const uint8_t* d_bits, const double* d_noise, int32_t* idx_out);

/* Hard re-initialisation (sparc_ldpc.py:831-838): stage the one-hot beta0
 * with c_l at idx[b][l] (B x L) for the next sa_run(..., SA_FLAG_BETA0). */
int sa_stage_onehot(sa_ctx* ctx, int B, const int32_t* idx);

/* The same with amplitude scale * c_l, idx -1 = an all-zero section: the 0/1
 * start beta_0 = beta / sqrt(n P / L) with its first L_zero sections zeroed of
 * the amp_test.py reps loop (amp_test.py:202-204; scale = 1 / sqrt(n P / L)). */
int sa_stage_onehot_scaled(sa_ctx* ctx, int B, const int32_t* idx, double scale);

/* sp2bp + LLR (sparc_ldpc.py:470-479, :257-281) of sections [l0, l0+ns) of
 * the current beta: llr = nan_to_num(log(1-p) - log(p)), p the bitwise
 * posterior of beta_l / c_l (binary64 c_l; an entry equal to c_l in the
 * context's precision counts as posterior 1, a decided section). */
int sa_llr(sa_ctx* ctx, int B, int l0, int ns, double* llr, int flags);

/* sa_llr with a choice of form and a clip on the magnitude.
 *   mode  SA_LLR_REFERENCE: the expression above (sa_llr is this with no clip).
 *         SA_LLR_TWO_SIDED: llr = nan_to_num(log(p0) - log(p1)), p1 the p above
 *         and p0 the same ordered sum over the entries whose bit is clear.
 *         Neither term is 1 - (a rounded sum): on a binary32 beta the
 *         reference form is noise from |llr| = 16 and 0 (NaN) where p > 1.
 *   clip  +inf or 0: none, +-inf -> +-DBL_MAX.  Finite > 0: the result is
 *         bounded to [-clip, clip], +-inf -> +-clip; NaN -> 0 either way.
 * An unknown mode, or a negative or NaN clip: SA_ERR_ARG, nothing is written. */
enum { SA_LLR_REFERENCE = 0, SA_LLR_TWO_SIDED = 1 };
int sa_llr_ex(sa_ctx* ctx, int B, int l0, int ns, double* llr, int flags, int mode, double clip);

/* Soft exchange (sparc_ldpc.py:683-698): beta0 := beta with sections
 * [l0, l0+ns) replaced by c_l * bp2sp(1/(1+exp(app))), staged for the next
 * sa_run(..., SA_FLAG_BETA0); the staged y is kept. */
int sa_soft_beta0(sa_ctx* ctx, int B, int l0, int ns, const double* app, int flags);

/* Hard exchange (sparc_ldpc.py:486-524): idx = bits2indices(app < 0) for
 * sections [l0, l0+ns) (idx_out: B x ns, may be NULL); if dst is given (a
 * context over the same n, e.g. sa_subset of the kept sections), stages
 * y - A beta_hard(idx) as dst's input y. */
int sa_hard_cancel(sa_ctx* ctx, int B, int l0, int ns, const double* app, int flags, sa_ctx* dst,
                   int32_t* idx_out);

/* Threshold decisions (amp_exit.py:56-105): for sections [l0, l0+ns) the
 * bp2sp of the LLRs `app` ([B][ns*log2 M]); idx_out[b][s] = the entry whose
 * normalised probability exceeds `threshold` if exactly one does, else -1. */
int sa_threshold(sa_ctx* ctx, int B, int l0, int ns, const double* app, int flags, double threshold,
                 int32_t* idx_out);

/* Hard cancellation of decided sections (amp_exit.py:107-109): stages
 * y - A beta(idx) as dst's input y, idx [B][L] with -1 for sections that are
 * not cancelled; dst is a context over the same n (e.g. sa_subset of the
 * undecided sections). */
int sa_cancel(sa_ctx* ctx, int B, const int32_t* idx, sa_ctx* dst);

/* The same with beta(idx) at amplitude scale * c_l: y - Ab(beta_0) of the
 * amp_test.py reps loop's hard initialisation (amp_test.py:207-210), where
 * beta_0 carries 1 = c_l / sqrt(n P / L) at the decided sections. */
int sa_cancel_scaled(sa_ctx* ctx, int B, const int32_t* idx, double scale, sa_ctx* dst);

/* ---- host-operator AMP (SA_BACKEND_HOST context; sa_create with ordering
 * NULL) ------------------------------------------------------------------
 * The reference's amp() takes ANY pair of callables (sparc_ldpc.py:189,196,
 * 213,220).  For operators that are not this library's, the caller applies
 * Ab / Az itself and the loop's other steps run on the device:
 *   sa_host_init(B, T, y, Pl, beta0, Ab(beta0))  z = y - Ab(beta0) (:192-200; both NULL: zero start)
 *   for t < T:
 *     sa_host_tau(t, stopped)        tau_t = sqrt(sum z^2 / n), stopped[b] = (tau_t == tau_{t-1}) (:203-209)
 *     if every codeword stopped: done
 *     sa_fetch_z -> the caller computes Az(z)
 *     sa_host_eta(t, Az(z))          beta = eta(beta + Az(z)) (:213-219)
 *     sa_fetch -> the caller computes Ab(beta)
 *     sa_host_residual(t, Ab(beta))  z = y - Ab(beta) + z / tau^2 (P - sum beta^2 / n) (:220)
 * Stopped codewords keep beta and z.  flags: SA_FLAG_NO_EARLY_STOP. */
int sa_host_init(sa_ctx* ctx, int B, int T, const double* y, const double* Pl, const double* beta0,
                 const double* ab0);
int sa_host_tau(sa_ctx* ctx, int B, int t, int flags, int* stopped);
int sa_host_eta(sa_ctx* ctx, int B, int t, int flags, const double* az);
int sa_host_residual(sa_ctx* ctx, int B, int t, int flags, const double* ab);

/* Monte-Carlo rep stream (BASELINE configs[3]: amp_test.py:183-246, the BER
 * sweeps of sparc_ldpc.py:1217-1245 / 1318-1323).
 *
 * sa_draw_reps: on the host cores, rep i drawn as NumPy's
 * RandomState(seeds[i]).randint(0, M, L) (idx_out [count][L]) followed by
 * .randn(n) * sigma (noise_out [count][n]), bit for bit NumPy's legacy
 * generator (MT19937, masked bounded integers, polar Gaussian); threads <= 0:
 * every hardware thread.
 *
 * sa_mc_stage copies `nreps` reps (section indices [nreps][L], noise
 * [nreps][n], fp64) to the device.  sa_mc_run decodes them through B slots
 * (4 <= B <= 1024) of the batched decode with per-slot refill: each slot runs
 * its own iteration index, and when its exact-tau stop fires or T iterations
 * are done its section decisions go to dec_out [nreps][L] and its stop index
 * (T when the loop ran out) to iters_out [nreps], and the next rep is encoded
 * into the slot (y = A beta(idx) + noise) on the device; errs_out [nreps]
 * receives each rep's bit errors (the popcounts of decision ^ index summed
 * over its sections, sparc_ldpc.py:462); any output may be NULL.  Every rep's
 * decisions and stop index equal those of sa_encode + sa_run(early stop) +
 * sa_decide on any batch holding it.  Needs one staged power allocation
 * (sa_stage Pl) and the batched codeword-interleaved Hadamard decode
 * (sa_plan: k_secb + k_rowc), else SA_ERR_UNSUPPORTED; ms_out: the device
 * time of the whole stream (events), or NULL. */
int sa_draw_reps(const uint32_t* seeds, int count, int L, int M, int n, double sigma, int32_t* idx_out,
                 double* noise_out, int threads);
int sa_mc_stage(sa_ctx* ctx, int nreps, const int32_t* idx, const double* noise);
int sa_mc_run(sa_ctx* ctx, int B, int T, int flags, int32_t* dec_out, int32_t* iters_out, int32_t* errs_out,
              double* ms_out);
/* sa_mc_draw stages `nreps` reps drawn on the device from their seeds: rep i
 * is sa_draw_reps' rep of seeds[i] at sigma[i] (one sigma per rep, so the
 * points of a sweep share a stream), NumPy's legacy generator run by one
 * workgroup per rep.  Only the seeds and sigmas go up.  The section indices
 * are bit for bit the host's; the noise is the host's up to the device
 * library's log against the C library's (both within an ulp: a few values in
 * a thousand differ, by under 2^-49 relative).  M must be a power of two
 * (randint(0, M) then rejects no draw), else SA_ERR_UNSUPPORTED.  Afterwards
 * sa_mc_run decodes the reps as after sa_mc_stage.  ms_out: the device time of
 * the draw (events), or NULL.  Blocking.
 *
 * sa_mc_fetch_draws reads the first `nreps` staged reps back, whichever call
 * staged them: idx_out [nreps][L], noise_out [nreps][n]; either may be NULL. */
int sa_mc_draw(sa_ctx* ctx, int nreps, const uint32_t* seeds, const double* sigma, double* ms_out);
int sa_mc_fetch_draws(sa_ctx* ctx, int nreps, int32_t* idx_out, double* noise_out);
/* The design's row sub-sampling table (sparc_ldpc.py:107-117): NumPy's
 * RandomState(seed) shuffling arange(1, w) once per section, cumulatively,
 * the first n of each kept, w = 2^ceil(log2(max(M+1, n+1))); out [L][n]. */
int sa_make_ordering(int L, int M, int n, uint32_t seed, uint32_t* out);

/* State evolution (SE) of the AMP decoder: the scalar recursion that predicts
 * a decode's effective noise variance tau_t^2 and its section error rate,
 * iteration by iteration, without a codeword.  Context-free like sa_draw_reps;
 * binary64 on the device.  For B allocations Pl [B][L] (P_b = sum_l Pl_{b,l}),
 * section size M, code length n and noise sigma [B]:
 *   tau_0^2 = sigma^2 + P,  c_l = sqrt(n Pl_l),  a = c_l / tau_t,
 *   E_l = E[ e^(a^2 + a U_1) / (e^(a^2 + a U_1) + sum_{j >= 2} e^(a U_j)) ],  U_j i.i.d. N(0, 1),
 *   x_{t+1} = sum_l (Pl_l / P) E_l,  tau_{t+1}^2 = sigma^2 + P (1 - x_{t+1}),
 * the decoder's section softmax (sparc_ldpc.py:213-219) applied to
 * s = c e_true + tau U; a (section, sample) pair is missed when
 * a^2 + a U_1 < max_{j >= 2} a U_j.  The expectation is the mean over S rows
 * of M Gaussians: row s = RandomState(seeds[s]).randn(M) drawn on the device
 * (NumPy's legacy generator, as sa_mc_draw), or the caller's U [S][M]; exactly
 * one of seeds and U is given.  The same S rows serve every section, every
 * iteration and every allocation of the call (common random numbers), so a
 * call is deterministic (the same inputs give the same bits, and an
 * allocation's results do not depend on the rest of the batch) and
 * allocations are compared on the same noise.  Sections of an allocation whose
 * powers are equal bit for bit are computed once.  All T iterations are queued
 * on one stream; the call waits once and copies back once.
 *   tau2_out [B][T+1], x_out [B][T], miss_out [B][T]: the missed (section,
 *   sample) pairs of iteration t, out of L * S; sec_out [B][L] or NULL: E_l of
 *   the last iteration; ms_out or NULL: device time of the draw and the
 *   iterations (events).
 * SA_ERR_ARG (sa_last_error names the argument; nothing is written): B < 1,
 * L < 1, M < 2, n < 1, T < 1, S < 1, a sigma that is not finite and > 0, a Pl
 * that is negative or not finite, P = 0, both or neither of seeds and U.
 * SA_ERR_UNSUPPORTED: M > SA_SE_MAX_M, the largest row a workgroup holds (M
 * need not be a power of two); S > 2^24.  SA_ERR_NO_DEVICE as elsewhere.
 *
 * sa_se_draws: the rows the seeded path uses, U_out [S][M]: NumPy's up to the
 * device library's log against the C library's (about one value in a
 * hundred differs, by under 2^-49 relative). */
enum { SA_SE_MAX_M = 4096 };
int sa_se(int device, int B, int L, int M, int n, const double* Pl, const double* sigma, int T, int S,
          const uint32_t* seeds, const double* U, double* tau2_out, double* x_out, int64_t* miss_out,
          double* sec_out, double* ms_out);
int sa_se_draws(int device, int S, int M, const uint32_t* seeds, double* U_out);

/* ---- spatially coupled SPARCs: base-matrix AMP ----
 * A coupled design over a Hadamard-backend context `parent` of L sections of
 * M columns and n rows: A[i, j] = sqrt(W[r(i), c(j)]) * At[i, j], At the
 * parent's +-1/sqrt(n) operator, W an R x C base matrix (row-major, entries
 * >= 0 and finite, a positive entry in every row and every column), row block
 * r(i) = i / (n / R), column block c(l) = l / (L / C) of section l.  The
 * decoder tracks one effective-noise level phi_r per row block and one
 * tau_c^2 per column block; beta = 0, z = y, then for t < T
 *   phi_r = sum_{i in r} z_i^2 / (n / R);  stop (index t) if t > 0 and every
 *           phi_r equals the previous iteration's bit for bit: beta, z kept
 *   1 / tau_c^2 = (1 / R) sum_r W[r, c] / phi_r
 *   u_j = beta_j c_l / tau_c^2 + c_l sum_i A[i, j] z_i / phi_r(i),  c_l = sqrt(n Pl_l)
 *   beta_j = c_l exp(u_j - max) / sum_section exp(...)
 *   psi_c = P_c - sum_{j in c} beta_j^2 / n,  gamma_r = sum_c W[r, c] psi_c,  P_c = sum_{l in c} Pl_l
 *   z_i = y_i - (A beta)_i + z_i gamma_r(i) / phi_r(i)
 * which at R = C = 1, W = [[1]] is sa_amp's loop (sparc_ldpc.py:189-222).
 *
 * sa_sc_create: the coupled context borrows the parent's device tables and
 * precision; the parent must outlive it.  It has its own stream and buffers.
 *   SA_ERR_ARG: R or C < 1, W NULL, R does not divide n, C does not divide L,
 *   a negative or non-finite entry, a row or column of W without a positive entry.
 *   SA_ERR_UNSUPPORTED: R or C above SA_SC_MAX_BLOCKS; M not a power of two; a
 *   parent that is not a Hadamard-backend context; n too large for z to fit
 *   the section kernel's LDS image.
 * sa_last_error names the argument; *out is not written on a refusal.
 *
 * sa_sc_Ab / sa_sc_Az: out[b] = A beta[b] (B x n) / A^T z[b] (B x L*M).
 *
 * sa_sc_amp decodes B codewords y (B x n) with section powers Pl [L]:
 * beta_out B x (L*M); iters_out [B] (may be NULL) the stop index, T when the
 * loop ran out; phi_out [B][T][R] (may be NULL) the phi_r of every iteration
 * that ran, rows from a codeword's stop index on zero.  flags:
 * SA_FLAG_NO_EARLY_STOP.  sa_sc_event_ms: the device time of the last
 * sa_sc_amp's iterations (events around the loop's launches).
 *
 * sa_sc_mc: one call on the device for B Monte-Carlo reps: encodes
 * y = A beta(idx) + noise (idx B x L, noise B x n binary64 or NULL; the
 * kernels of sa_sc_Ab, the noise added in binary64), decodes, takes each
 * section's argmax (first index on ties) into dec_out [B][L], the stop
 * indices into iters_out [B] and each rep's bit errors (popcounts of
 * decision ^ index summed over its sections, as sa_mc_run counts them) into
 * errs_out [B]; any output may be NULL; ms_out: the device time of encoder,
 * decode and decisions (events), or NULL.
 *
 * sa_sc_amp_ex / sa_sc_mc_ex (since SA_VERSION 0.5):
 * the same calls with an opt-in tolerance stop and frozen column blocks.
 * stop_tol, freeze_tol >= 0 are taken in the context's precision; per codeword
 * taul_c is the tau_c^2 at which block c's beta was last computed.
 *   stop (index t) if t > 0 and |phi_r - phi_r^(t-1)| <= stop_tol * phi_r^(t-1)
 *     for every r (stop_tol = 0: bit equality, the rule above;
 *     SA_FLAG_NO_EARLY_STOP still disables it);
 *   tau_c^2 = R / sum_r W[r, c] / phi_r; block c is live at t if t = 0, or
 *     freeze_tol == 0 (off), or |tau_c^2 - taul_c| > freeze_tol * taul_c; for
 *     live blocks taul_c = tau_c^2;
 *   u and beta are computed for live blocks only: a frozen block's beta, psi_c
 *     and A beta stay as its last live iteration left them; the psi, gamma and
 *     z steps are unchanged.  A frozen block is live again by the same test
 *     whenever its tau_c^2 has drifted: nothing is sticky.
 * live_out [B][T][C] bytes (may be NULL): 1 where block c was live in
 * iteration t, rows from a codeword's stop index on zero.  With both
 * tolerances 0 the calls are sa_sc_amp / sa_sc_mc, bit for bit, and launch the
 * same kernels (live_out is then 1 in front of the stop index).
 *   SA_ERR_ARG: a negative, NaN or infinite stop_tol or freeze_tol (named in
 *   sa_last_error); no output is written on a refusal. */
enum { SA_SC_MAX_BLOCKS = 64 };
typedef struct sa_sc sa_sc;
int sa_sc_create(sa_ctx* parent, int R, int C, const double* W, sa_sc** out);
void sa_sc_destroy(sa_sc* sc);
int sa_sc_Ab(sa_sc* sc, int B, const double* beta, double* out);  /* A beta,  B x n    */
int sa_sc_Az(sa_sc* sc, int B, const double* z, double* out);     /* A^T z,   B x L*M  */
int sa_sc_amp(sa_sc* sc, int B, const double* y, const double* Pl, int T, double* beta_out,
              int* iters_out, double* phi_out, int flags);
double sa_sc_event_ms(sa_sc* sc);
int sa_sc_mc(sa_sc* sc, int B, const int32_t* idx, const double* noise, const double* Pl, int T,
             int flags, int32_t* dec_out, int32_t* iters_out, int32_t* errs_out, double* ms_out);
int sa_sc_amp_ex(sa_sc* sc, int B, const double* y, const double* Pl, int T, double stop_tol,
                 double freeze_tol, double* beta_out, int* iters_out, double* phi_out,
                 unsigned char* live_out, int flags);
int sa_sc_mc_ex(sa_sc* sc, int B, const int32_t* idx, const double* noise, const double* Pl, int T,
                double stop_tol, double freeze_tol, int flags, int32_t* dec_out, int32_t* iters_out,
                int32_t* errs_out, unsigned char* live_out, double* ms_out);

/* ---- coupled AMP from a beta_0, the staged coupled context and the SPARC <->
 * LDPC glue on it (since SA_VERSION 0.6) ----
 * The beta_0 start is the uncoupled decoder's (sparc_ldpc.py:192-200) on the
 * coupled design: beta = beta_0, z = y - A beta_0, no Onsager term at the
 * start, then the loop above unchanged (iteration 0's u reads beta = beta_0).
 * It composes with stop_tol / freeze_tol; at t = 0 every block is live.
 *
 * sa_sc_amp_start is sa_sc_amp_ex with a start beta0 [B][L*M]; with beta0 NULL
 * it is that call, launch for launch.
 *
 * The staged calls keep y, beta and the traces on the device between calls, as
 * sa_reserve ... sa_fetch do for a sa_ctx:
 *   sa_sc_reserve       sizes the workspace for B codewords and T iterations
 *                       (growing it drops whatever was staged);
 *   sa_sc_stage_power   stages the section powers Pl [L];
 *   sa_sc_stage         stages y [B][n] and, where given, beta0 [B][L*M];
 *   sa_sc_encode        stages y = A beta(idx) + noise (idx [B][L] in [0, M),
 *                       noise [B][n] binary64 or NULL; sa_sc_mc's encoder);
 *   sa_sc_encode_bits   the same from device pointers: message bits [B][L log2 M]
 *                       bytes, MSB first per section, and noise [B][n] binary64
 *                       or NULL; idx_out [B][L] (host, may be NULL) receives the indices;
 *   sa_sc_run           queues a decode of the staged y on the context's stream
 *                       and returns; flags SA_FLAG_NO_EARLY_STOP, SA_FLAG_BETA0
 *                       (start from the beta on the device: staged, written by
 *                       the glue below, or left by the last run); the staged y
 *                       survives any number of runs;
 *   sa_sc_wait          waits for the stream;
 *   sa_sc_fetch         beta_out [B][L*M], iters_out [B], phi_out [B][T][R] of
 *                       the last run (each may be NULL);
 *   sa_sc_decide        each section's argmax (first index on ties), idx_out [B][L].
 * The glue works on the context's beta with the kernels, semantics and flags
 * (SA_PTR_DEVICE included) of its sa_ctx namesakes: sa_sc_llr is sa_llr_ex,
 * sa_sc_soft_beta0 is sa_soft_beta0, sa_sc_hard_indices is sa_hard_cancel
 * without a dst, sa_sc_stage_onehot is sa_stage_onehot.  The protected
 * sections are [l0, l0 + ns); any l0 >= 0 is legal, inside a column block too.
 * The one-call entry points above overwrite the workspace: after one of them
 * nothing is staged.
 *   SA_ERR_ARG (sa_last_error names it; no output and nothing staged is
 *   touched): B outside [1, 65535] or above the reserved batch, T above the
 *   reserved T, a run with nothing staged ("nothing staged"), with B above the
 *   staged batch or without staged powers, SA_FLAG_BETA0 or sa_sc_llr with no
 *   beta on the device, l0 < 0, ns < 1, l0 + ns > L, an index outside [0, M),
 *   a NULL argument that must not be, unknown flags or LLR mode, a bad
 *   tolerance or clip.  SA_ERR_UNSUPPORTED: M < 2. */
int sa_sc_amp_start(sa_sc* sc, int B, const double* y, const double* Pl, int T, const double* beta0,
                    double stop_tol, double freeze_tol, double* beta_out, int* iters_out,
                    double* phi_out, unsigned char* live_out, int flags);
int sa_sc_reserve(sa_sc* sc, int B, int T);
int sa_sc_stage_power(sa_sc* sc, const double* Pl);
int sa_sc_stage(sa_sc* sc, int B, const double* y, const double* beta0);
int sa_sc_encode(sa_sc* sc, int B, const int32_t* idx, const double* noise);
int sa_sc_encode_bits(sa_sc* sc, int B, const uint8_t* d_bits, const double* d_noise, int32_t* idx_out);
int sa_sc_run(sa_sc* sc, int B, int T, double stop_tol, double freeze_tol, int flags);
int sa_sc_wait(sa_sc* sc);
int sa_sc_fetch(sa_sc* sc, int B, double* beta_out, int* iters_out, double* phi_out);
int sa_sc_decide(sa_sc* sc, int B, int32_t* idx_out);
int sa_sc_llr(sa_sc* sc, int B, int l0, int ns, double* llr, int flags, int mode, double clip);
int sa_sc_soft_beta0(sa_sc* sc, int B, int l0, int ns, const double* app, int flags);
int sa_sc_hard_indices(sa_sc* sc, int B, int l0, int ns, const double* app, int flags, int32_t* idx_out);
int sa_sc_stage_onehot(sa_sc* sc, int B, const int32_t* idx);

/* ---- coupled state evolution ----
 * The scalar recursion that predicts a coupled decode, iteration by
 * iteration, without a codeword: the per-row-block phi_r, the
 * per-column-block tau_c^2 and section error rate.  Context-free like sa_se;
 * binary64 on the device.  A batch of B configurations shares L and M; n, R,
 * C [B], the base matrices W (row-major, back to back), Pl [B][L] and sigma
 * [B] are per configuration.  With c_l = sqrt(n Pl_l), P_c = sum_{l in c} Pl_l
 * (l in order) and the rows U of sa_se (exactly one of seeds and U):
 *   psi_c^0 = P_c
 *   phi_r^t = sigma^2 + sum_c W[r, c] psi_c^t                  (c in order)
 *   1 / tau_c^2^t = (1 / R) sum_r W[r, c] / phi_r^t             (r in order)
 *   a = c_l / tau_c(l)^t,  E_l as in sa_se,  a pair missed as in sa_se
 *   x_c^t = sum_{l in c} (Pl_l / P_c) E_l,  psi_c^{t+1} = P_c (1 - x_c^t)
 * the decoder's steps 1, 3, 5 and 6 applied to s = c e_true + tau_c U; at
 * R = C = 1, W = [[1]] it is sa_se's recursion with tau^2 = phi.  Sections of
 * one configuration and one column block whose powers are equal bit for bit
 * are computed once.  For t >= 1 a column block whose tau_c^2 has the bits it
 * had at t - 1 is not recomputed (E is a function of tau^2 and U alone, so
 * the results are the same bits); flags = SA_SCSE_NO_SKIP recomputes it.  All
 * T iterations are queued on one stream; the call waits once and copies back
 * once.  A configuration's results do not depend on the rest of the batch.
 *   phi_out [B][T+1][Rmax], tau2_out, x_out, miss_out [B][T][Cmax] (the missed
 *   (section, sample) pairs of block c at t, out of (L / C) S), zero beyond a
 *   configuration's own R and C; stop_out [B]: the predicted stop index, the
 *   first t >= 1 at which every phi_r^t equals phi_r^{t-1} bit for bit (the
 *   decoder's stopping rule), or T; sec_out [B][L] or NULL: E_l of the last
 *   iteration; ms_out or NULL: device time of the draw and the iterations.
 * SA_ERR_ARG (sa_last_error names the argument and the configuration; nothing
 * is written): B, L, T, S < 1, M < 2, n, R or C < 1, R does not divide n, C
 * does not divide L, a negative or non-finite entry of W, a row or column of W
 * without a positive entry, a sigma that is not finite and > 0, a Pl that is
 * negative or not finite, P_c = 0, Rmax or Cmax below the batch's largest,
 * both or neither of seeds and U, unknown flags.  SA_ERR_UNSUPPORTED: R or C
 * above SA_SC_MAX_BLOCKS, M > SA_SE_MAX_M (M need not be a power of two: SE
 * never gathers), S > 2^24. */
enum { SA_SCSE_NO_SKIP = 1 };
int sa_sc_se(int device, int B, int L, int M, const int* n, const int* R, const int* C, const double* W,
             const double* Pl, const double* sigma, int T, int S, const uint32_t* seeds, const double* U,
             int Rmax, int Cmax, int flags, double* phi_out, double* tau2_out, double* x_out,
             int64_t* miss_out, int* stop_out, double* sec_out, double* ms_out);

/* Introspection. */
/* The kernels a decode of B codewords runs: out8 = {section path (sa_sec_path),
 * Ab partials per codeword, row splits, codewords per batched workgroup,
 * z^2 partials, w, row kernel (sa_row_kernel), number of CUs}. */
typedef enum sa_sec_path {
  SA_SEC_K_SEC = 0,    /* k_sec: one wave per section, row splits */
  SA_SEC_K_SEC2 = 1,   /* k_sec2: two waves per section */
  SA_SEC_K_SECB = 2,   /* k_secb: the batched kernel */
  SA_SEC_DENSE = 3,    /* dense fp32 GEMVs */
  SA_SEC_K_SEC4 = 4,   /* k_sec4: four waves per section, pairs of sections */
  SA_SEC_K_SEC43 = 5,  /* k_sec43: four waves per section, triples of sections */
  SA_SEC_DENSE_I8 = 6, /* dense int8 MFMA GEMMs */
  SA_SEC_MATRIX = 7,   /* caller-matrix f32 / f64 MFMA GEMMs */
  SA_SEC_K_SECG = 8,   /* k_secg: z from global memory, 32-bit bucket entries (n past the LDS image or >= 65535) */
  SA_SEC_K_SEC44 = 9   /* k_sec44: four waves per section, quads of sections (1024-thread workgroups) */
} sa_sec_path;
typedef enum sa_row_kernel {
  SA_ROW_K_ROW = 0,     /* k_row: 64-row blocks */
  SA_ROW_K_ROW2 = 1,    /* k_row2: 32-row blocks */
  SA_ROW_K_ROWV16 = 2,  /* k_rowv, 16-byte rows */
  SA_ROW_K_ROWV8 = 3,   /* k_rowv, 8-byte rows */
  SA_ROW_K_ROW2_16 = 4, /* k_row2: 16-row blocks */
  SA_ROW_K_ROWC = 5     /* k_rowc: codeword-interleaved rows behind k_secb */
} sa_row_kernel;
int sa_plan(sa_ctx* ctx, int B, int64_t* out8);
/* The batched section kernel's work order for B codewords (k_secb, B >= 4):
 * out4 = {section groups, sections per workgroup, section groups per XCD per
 * pass, passes per XCD}; SA_ERR_ARG when a decode of B does not run k_secb. */
int sa_plan_batched(sa_ctx* ctx, int B, int64_t* out4);
int sa_info(const sa_ctx* ctx, int64_t* out8); /* L, M, n, w, backend, precision, device, bytes */
int sa_device_count(void);
const char* sa_last_error(void);
const char* sa_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPARC_AMP_H */
