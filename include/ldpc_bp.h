/* ldpc_bp.h — C ABI of the MI355X (gfx950) LDPC belief-propagation decoder.
 *
 * Replaces the reference's native LDPC decoder ldpc/src/c_ldpc.c, bound by
 * ctypes in ldpc/py/ldpc.py:855-930 (code.decode).  Two layers:
 *
 *  1. Reference-signature entry points (sumprod, sumprod2, minsum, Lxor,
 *     Lxfb): same names, argument lists and meaning as c_ldpc.c:32, 138, 339,
 *     234, 294, so `ct.CDLL(".../libldpc_bp.so")` can stand in for
 *     `ct.CDLL('./bin/c_ldpc.so')` (ldpc.py:859) unchanged.  They decode one
 *     word on the GPU (the graph is uploaded once and cached by content).
 *     Return: iteration count (0..200) as the reference, or a negative
 *     LB_ERR_* code (the reference returns -1 when calloc fails, c_ldpc.c:40-42).
 *
 *  2. A context API for batches of B words sharing one graph (Monte-Carlo),
 *     with device-resident buffers for the joint SPARC/LDPC pipeline.
 *
 * All arithmetic is IEEE binary64 in the reference's per-node operation order
 * (the layered decoders also run in binary32 on request, LB_F32, and layered
 * min-sum on saturating integers of settable widths, LB_FIXED).
 * Graph arrays follow ldpc.py:694-786: vdeg[Nv], cdeg[Nc], intrlv[Nmsg]
 * (message index, in check-node order, of each variable-node port).
 */
#ifndef LDPC_BP_H
#define LDPC_BP_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  LB_OK = 0,
  LB_ERR_ARG = -1,         /* bad argument (reference: NameError / assert) */
  LB_ERR_HIP = -2,         /* HIP runtime failure */
  LB_ERR_NOMEM = -3,       /* device allocation failed (c_ldpc.c:40-42 returns -1) */
  LB_ERR_GRAPH = -4,       /* degrees do not sum to Nmsg, or intrlv is not a permutation */
  LB_ERR_UNSUPPORTED = -5, /* check degree > 32 or variable degree > 255; a flag on a type it does not exist for */
  LB_ERR_NO_DEVICE = -6    /* no HIP device: there is no CPU fallback */
};

/* 3, 4: the layered schedule (see lb_set_layers) with sumprod2's / minsum's check rule */
enum { LB_SUMPROD2 = 0, LB_SUMPROD = 1, LB_MINSUM = 2, LB_LAYERED_SUMPROD2 = 3, LB_LAYERED_MINSUM = 4 };
/* Precision flag, OR-ed into algo: LB_LAYERED_SUMPROD2 | LB_F32 and
 * LB_LAYERED_MINSUM | LB_F32 decode in binary32 (see "binary32" below).  On a
 * flooding type it is LB_ERR_UNSUPPORTED. */
#define LB_F32 0x100
/* Arithmetic flag, OR-ed into algo: LB_LAYERED_MINSUM | LB_FIXED decodes on
 * integers of settable widths (see "fixed point" below).  On any other type it
 * is LB_ERR_UNSUPPORTED; together with LB_F32 it is LB_ERR_ARG. */
#define LB_FIXED 0x400

#define LB_MAX_ITCOUNT 200 /* c_ldpc.c:7 */

typedef struct lb_ctx lb_ctx;

/* ---- reference-signature drop-ins (c_ldpc.c) ---------------------------- */
int sumprod(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg,
            double* app);                                      /* c_ldpc.c:32  */
int sumprod2(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg,
             double* app);                                     /* c_ldpc.c:138 */
int minsum(double* ch, long* vdeg, long* cdeg, long* intrlv, int Nv, int Nc, int Nmsg,
           double* app, double correction_factor);             /* c_ldpc.c:339 */
double Lxor(double L1, double L2, int corr_flag);              /* c_ldpc.c:234; NaN on failure */
double Lxfb(double* L, long dc, int corr_flag);                /* c_ldpc.c:294; NaN on failure */

/* ---- batched context API ---------------------------------------------------- */
/* Upload a graph (host arrays as above) to `device`. */
int lb_create(lb_ctx** out, const long* vdeg, const long* cdeg, const long* intrlv, int Nv, int Nc,
              int Nmsg, int device);
void lb_destroy(lb_ctx* ctx);

/* Decode B words: ch[B][Nv] channel LLRs -> app[B][Nv] a-posteriori LLRs and
 * iters[B] (the reference's return value per word).  Host pointers; blocking.
 * max_iter = 0 (here and in lb_decode_device, lb_run, lb_mc_run and
 * lb_mc_run_seeds) runs no iteration: app = ch, the variable phase on zero
 * messages (the uncoded hard decision), and iters = 0 for every word.
 * max_iter < 0 is LB_ERR_ARG. */
int lb_decode(lb_ctx* ctx, int B, const double* ch, double* app, int* iters, int algo,
              double corr_factor, int max_iter);

/* Device-resident form: d_ch / d_app / d_iters are device pointers on the
 * context's device; queued on the context's stream, returns without waiting
 * (the tail is sized on the device, see lb_set_tail). */
int lb_decode_device(lb_ctx* ctx, int B, const double* d_ch, double* d_app, int* d_iters, int algo,
                     double corr_factor, int max_iter);

/* Device buffers of the context sized for B words (ch, app: B x Nv doubles;
 * iters: B ints), for handing LLRs to / from other device code (the SPARC
 * glue of libsparc_amp.so) without a host round trip.  lb_run / lb_fetch
 * operate on them. */
int lb_buffers(lb_ctx* ctx, int B, double** d_ch, double** d_app, int** d_iters);

/* Measurement helpers: stage B words into the context's device buffers, run
 * (asynchronously), wait, fetch; lb_run_event_ms = device time of the last run. */
int lb_stage(lb_ctx* ctx, int B, const double* ch);
int lb_run(lb_ctx* ctx, int B, int algo, double corr_factor, int max_iter);
int lb_wait(lb_ctx* ctx);
int lb_fetch(lb_ctx* ctx, int B, double* app, int* iters);
double lb_run_event_ms(lb_ctx* ctx);

/* out[0..9] = Nv, Nc, Nmsg, max vdeg, max cdeg, messages in LDS (1/0),
 *             threads per workgroup, device, the check degree of the
 *             straight-line check kernel of a check-regular code (0: the
 *             general kernel), and the first tail iteration (0: off) */
int lb_info(lb_ctx* ctx, long long* out);

/* Tail launches: a decode runs its first `tail_at` iterations one workgroup
 * per word; the words still running after that are spread over several
 * workgroups each, two launches per iteration (bit-identical results).
 * lb_decode (blocking) reads back the number of words left once and sizes
 * the tail for them, issuing iterations until a read-back shows every word
 * done; lb_run / lb_decode_device never wait: every iteration up to
 * max_iter is queued, sized from the previous tail's word count, and a
 * launch past the last running word returns at once.  tail_at < 0: the
 * default chosen at lb_create (8, or the environment's LDPC_BP_TAIL); 0: off.
 * Needs variable degrees <= 12 (LB_ERR_UNSUPPORTED otherwise).  The layered
 * decoders take no part in the tail launches: they ignore tail_at. */
int lb_set_tail(lb_ctx* ctx, int tail_at);

/* ---- layered schedule (row-layered / turbo-decoding message passing) ---------- */
/* algo = LB_LAYERED_SUMPROD2 / LB_LAYERED_MINSUM, wherever algo is taken
 * (lb_decode, lb_decode_device, lb_run, lb_mc_run, lb_mc_run_seeds), decodes
 * with the layered schedule: layer l is the consecutive checks first_check[l] ..
 * first_check[l+1] - 1 (for a quasi-cyclic code its protograph rows,
 * first_check = 0, z, 2z, .., Nc).  With app = ch and r = 0 (one message per
 * edge, in check order), a sweep takes the layers in order; per layer, for
 * each check and each of its edges e on variable v: q[e] = app[v] - r[e]; the
 * check rule on the check's q gives its new r (Lxfb with the correction
 * terms, or Lxfb without them times corr_factor); app[v] = q[e] + r[e].
 * Before each sweep the stop test: every check has an even number of
 * variables with app < 0 and none with app == 0 or NaN.  iters = i: the test
 * passed after i sweeps (0: the channel word is a codeword already);
 * max_iter: it had not passed before the last sweep.  One launch, one
 * workgroup per word; lb_run and lb_decode_device never wait.
 *
 * lb_set_layers checks on the host, before anything is uploaded or changed,
 * that first_check[0..nlayers] increases strictly from 0 to Nc and that no
 * variable occurs twice in a layer (the checks of a layer are then independent
 * and the result does not depend on the order they are taken in): otherwise
 * LB_ERR_GRAPH, with a message naming the layer and the variable, and the
 * context is left as it was.  A layered algo on a context without layers is
 * LB_ERR_ARG.
 *
 * lb_layer_info: out[0..3] = nlayers (0: none set), the largest layer's
 * checks, where the messages live (2: r and app in LDS, 1: app in LDS and r in
 * HBM, 0: both in HBM) and threads per workgroup.  r and app live in LDS when
 * they fit, and the workgroup has a thread per edge of the largest layer (at
 * most 1024; 768 for check-regular codes of degree 20).
 *
 * Measurement switches, read from the environment by lb_set_layers:
 * LDPC_BP_LAYERED_LDS = 1 / 0 keeps r / r and app in HBM although they would
 * fit; LDPC_BP_LAYERED_THREADS = the threads per workgroup;
 * LDPC_BP_LAYERED_F32_RESIDENT = 1 pads a binary32 workgroup's LDS so that it
 * has its CU alone (the results are the same bits either way). */
int lb_set_layers(lb_ctx* ctx, int nlayers, const int* first_check);
int lb_layer_info(lb_ctx* ctx, long long* out);

/* binary32: algo = LB_LAYERED_SUMPROD2 | LB_F32 or LB_LAYERED_MINSUM | LB_F32,
 * wherever algo is taken, runs the same schedule with app, r, q, every Lxor
 * and corr_factor held and rounded in binary32.  ch, app and iters keep their
 * types and layouts: the kernel loads ch32 = (float)clip(ch, -2^100, 2^100)
 * (NaN stays NaN, the sign of zero is kept; with variable degrees <= 255 |app|
 * then stays below 2^108, so saturated inputs up to +-DBL_MAX or +-inf never
 * meet as inf - inf) and stores app = (double)app32.  Layered minsum is the
 * same IEEE operations as its statement in NumPy, bit for bit; layered
 * sumprod2 evaluates log(1 + exp(-x)) with the hardware's binary32 exp2 and
 * log2.  The stop test, the meaning of iters and max_iter = 0 (app = ch,
 * unclamped) are the binary64 decoders'.  r and app live in LDS when
 * (Nmsg + Nv) * 4 bytes fit, app alone when Nv * 4 bytes fit; r in HBM is kept
 * in the context's message slices as floats.  LB_F32 on a flooding type is
 * LB_ERR_UNSUPPORTED (binary32 exists for the layered types only); on a
 * context without layers the layered types are LB_ERR_ARG in either precision.
 *
 * lb_layer_info_ex: precision 0 (binary64) or 1 (binary32); out[0..7] =
 * nlayers, the largest layer's checks, where the messages live (2 / 1 / 0 as
 * lb_layer_info's out[2]), threads per workgroup, dynamic LDS bytes,
 * workgroups resident per CU of the sumprod2 and of the minsum instance (the
 * runtime's occupancy figure at that thread count and LDS size; 0 before
 * lb_set_layers), and the bytes per message (8 / 4). */
int lb_layer_info_ex(lb_ctx* ctx, int precision, long long* out);

/* fixed point: algo = LB_LAYERED_MINSUM | LB_FIXED, wherever algo is taken
 * (lb_decode, lb_decode_device, lb_run, lb_mc_run, lb_mc_run_seeds,
 * lb_mc_stream_seeds), runs layered normalised min-sum on saturating integers,
 * the decoder a receiver builds (tests/ldpc_fixed_ref.py is its statement; the
 * kernel equals it bit for bit).  frac_bits F in 0..8, msg_bits MB in 2..8,
 * app_bits AB in MB..16; rmax = 2^(MB-1) - 1, amax = 2^(AB-1) - 1,
 * alpha = rint(16 corr_factor), which must lie in 1..16 (LB_ERR_ARG otherwise,
 * and for a NaN).
 *   app[v] = clip(rint(ch[v] 2^F), -rmax, rmax)   half to even; NaN -> 0; +-inf saturate; -0.0 -> 0
 *   r[e] = 0; per sweep, after the layered decoders' stop test (every check even
 *   in app < 0, no app == 0), per layer, per check, per edge e on variable v:
 *     q[e]   = clip(app[v] - r[e], -amax, amax)
 *     mag, neg = the minimum of |q| and the xor of (q < 0) over the check's other
 *                edges (a check of degree 1: mag = amax)
 *     m      = min((alpha mag + 8) >> 4, rmax);  r[e] = neg ? -m : m
 *     app[v] = clip(q[e] + r[e], -amax, amax)
 * ch, app and iters keep their types and layouts: app = (double)int 2^-F, so a
 * zero is +0.  iters and max_iter mean what they mean for the other layered
 * decoders; max_iter = 0 leaves app = ch, unquantised.  lb_set_tail does not
 * apply.  app (int16) and r (int8) live in LDS for the whole decode, one
 * workgroup per word, a group of lanes per check and one barrier per layer;
 * there are no HBM layouts (no code this project builds needs them): when
 * 2 Nv + Nmsg bytes do not fit a workgroup's LDS the call is LB_ERR_UNSUPPORTED.
 * Errors leave app, iters and the context as they were: no layers set,
 * alpha out of range, LB_FIXED | LB_F32: LB_ERR_ARG; LB_FIXED on another type
 * than LB_LAYERED_MINSUM, or an image that does not fit: LB_ERR_UNSUPPORTED.
 *
 * lb_set_fixed sets the widths for the decodes that follow (any time between
 * decodes; out of range: LB_ERR_ARG and the context unchanged; never called:
 * 2, 6, 8).  lb_fixed_info: out[0..7] = frac_bits, msg_bits, app_bits, threads
 * per workgroup, lanes per check, dynamic LDS bytes (2 Nv + Nmsg rounded up to
 * 16), workgroups resident per CU (the runtime's occupancy figure) and whether
 * the image fits (1 / 0); the last five are 0 before lb_set_layers.
 *
 * Measurement and test switches, read from the environment by lb_set_layers and
 * lb_set_fixed: LDPC_BP_FIXED_LANES = the lanes per check (1, 2, 4, 8 or 16),
 * LDPC_BP_FIXED_THREADS = the threads per workgroup (a multiple of 64 up to
 * 1024).  The results are the same bits for every setting. */
int lb_set_fixed(lb_ctx* ctx, int frac_bits, int msg_bits, int app_bits);
int lb_fixed_info(lb_ctx* ctx, long long* out);

/* ---- LDPC-only Monte-Carlo (sim_ldpc sparc_ldpc.py:1064-1124, ldpc_awgn.py, ldpc_bsc.py) ---- */
/* Block s is its seed: RandomState(seeds[i]) draws randint(0, 2, K) into
 * u[i][K] (bits as bytes; skipped when K == 0, u may then be NULL) and then
 * randn(N) (kind 0) or random_sample(N) (kind 1) into w[i][N], bit for bit
 * NumPy's legacy generator, over at most `threads` host threads (<= 0: the
 * host's, at most 16).  Host arrays; needs no device. */
int lb_draw_blocks(const unsigned int* seeds, int nblk, int K, int N, int kind, unsigned char* u, double* w,
                   int threads);

/* The quasi-cyclic encoder of the context's code: proto[Mp][Np] base matrix of
 * shifts (-1: no block, as ldpc.py:26-663), lifting size z, Np z = Nv and
 * Mp z = Nc.  Mp == 0: no encoder (the all-zero word).  LB_ERR_ARG when the
 * shifts of column Np - Mp do not reduce to a single offset (ldpc.py:815-822;
 * checked on the host before anything else). */
int lb_mc_set_code(lb_ctx* ctx, const int* proto, int Mp, int Np, int z);

/* x[B][Nv] = the systematic codewords of u[B][Nv - Nc] (bits as bytes), encoded
 * on the device.  Host pointers; blocking. */
int lb_encode(lb_ctx* ctx, int B, const unsigned char* u, unsigned char* x);

/* nblk blocks, `batch` at a time: encode u[nblk][Nv - Nc] (NULL: the all-zero
 * word), channel LLRs from w[nblk][Nv] on the device, decode, count.
 *   kind 0 (AWGN, a = sigma): ch = (2 / sigma^2) ((1 - 2 x) + sigma w)
 *   kind 1 (BSC, a = p, u NULL): ch = -log((1 - p) / p) where w < p, + elsewhere
 * errs[nblk] = sum((app < 0) != x) over the Nv bits, iters[nblk] = the
 * decoder's iteration counts.  Host pointers; blocking; lb_run_event_ms gives
 * the device time of the whole run. */
int lb_mc_run(lb_ctx* ctx, int nblk, const unsigned char* u, const double* w, double a, int kind, int batch,
              int algo, double corr_factor, int max_iter, int* errs, int* iters);

/* lb_mc_run with every batch's bits and noise drawn on the device from the
 * blocks' seeds (NumPy's legacy generator, one workgroup per block), on the
 * context's stream in front of the encoder: only the seeds go up.  K: the
 * bits drawn per block, Nv - Nc (encoded; needs lb_mc_set_code) or 0 (the
 * all-zero word, no randint).  The bits and the random_sample values (kind 1)
 * are bit for bit lb_draw_blocks'; the randn values (kind 0) are its values up
 * to the device library's log against the C library's (both within an ulp: a
 * few values in a thousand differ, by under 2^-49 relative).
 *
 * lb_draw_blocks_device: the same kernel with the arrays copied back, the
 * device twin of lb_draw_blocks (u[nblk][K], w[nblk][N], host arrays; any K
 * and N).  Blocking. */
int lb_mc_run_seeds(lb_ctx* ctx, int nblk, const unsigned int* seeds, int K, double a, int kind, int batch,
                    int algo, double corr_factor, int max_iter, int* errs, int* iters);
int lb_draw_blocks_device(lb_ctx* ctx, const unsigned int* seeds, int nblk, int K, int N, int kind,
                          unsigned char* u, double* w);

/* One operating point as a stream (opt-in; layered decoders only).  The blocks
 * of lb_mc_run_seeds (same seeds, K, a, kind: the same draws, code words and
 * channel values), in chunks of `chunk` blocks over two lanes (two streams,
 * each with its own buffers).  Per chunk: the draw and the encoder / channel
 * kernels over the whole chunk, then one persistent kernel of `slots`
 * workgroups.  Each workgroup takes the chunk's next block by a ticket, decodes
 * it with the layered decoder's arithmetic (per block the same errs and iters
 * as lb_mc_run_seeds, bit for bit) and counts its bit errors itself, until the
 * chunk is out of tickets; no workgroup waits for another.  Chunk k + 1's
 * workgroups take the CUs that chunk k's last blocks leave, so a block that
 * runs to max_iter holds one CU, not the launch.  Device memory for the
 * decoder grows with `slots`, not with `chunk`.
 *
 * min_errors > 0: the stopping rule of a Monte-Carlo point, blocks in seed
 * order until min_errors of them have errs > 0 (or nblk).  n* = the blocks
 * that rule consumes.  The host consumes chunk k - 2 before it queues chunk k
 * (at most two chunks in flight) and queues nothing once the rule is met; on
 * the device a block is skipped when the block errors of the consumed chunks,
 * of the chunk before and of its own chunk's finished blocks reach
 * min_errors: all of them lie at smaller seed indices, so only blocks from n*
 * on are ever skipped.  Blocks below n* are always decoded; which blocks from
 * n* on are decoded depends on timing.  min_errors <= 0: every block is decoded.
 *
 * errs[nblk], iters[nblk] in seed order; iters = -1 (and errs = 0) marks a
 * block that was not decoded.  out[0..3] = n* (nblk when the rule is off or
 * never met), the blocks decoded, the slots per lane used, the chunks queued.
 * slots <= 0: the workgroups the device holds at once (the instance's
 * residency on a CU times the CU count); at most the chunk's blocks are used.
 * algo: a flooding type is LB_ERR_UNSUPPORTED.  No layers set, chunk <= 0, or
 * K / a / kind that lb_mc_run_seeds refuses: LB_ERR_ARG, and the context is
 * left as it was.  max_iter = 0 as in lb_mc_run_seeds (errs of the channel's
 * hard decision, iters = 0).  Host pointers; blocking; lb_run_event_ms gives
 * the device time of the whole call, both lanes. */
int lb_mc_stream_seeds(lb_ctx* ctx, int nblk, const unsigned int* seeds, int K, double a, int kind, int chunk,
                       int slots, int min_errors, int algo, double corr_factor, int max_iter, int* errs,
                       int* iters, long long* out);

/* The reps of the joint SPARC + LDPC simulators (sparc_ldpc.py:419-446 /
 * :606-634) drawn and encoded on the device, one workgroup per seed.  For
 * RandomState(seeds[i]): randint(0, 2, K) are the protected bits (output word
 * k & 1), randint(0, 2, U) the unprotected bits (word (K + j) & 1; U = 0 draws
 * nothing), randn(n) * sigma the noise (from word K + U on, no cached value).
 * The protected bits are then encoded (the encoder of lb_encode).  Two buffers
 * of the context receive the reps and stay valid until its next lb_joint_draw:
 *   *d_bits   [nrep][U + Nv] bytes: the U unprotected bits, then the codeword
 *   *d_noise  [nrep][n] binary64
 * device pointers for sa_encode_bits (include/sparc_amp.h).  The bits are bit
 * for bit NumPy's and ldpc.encode_batch's; the noise is NumPy's up to the
 * device library's log, as in lb_mc_run_seeds.  Blocking (a consumer on another
 * stream needs no event); ms_out (or NULL): the device time of the draw and the
 * encoder (events).  LB_ERR_ARG, and nothing is touched: K != Nv - Nc, no
 * encoder set (lb_mc_set_code), U < 0, n <= 0, sigma not finite, nrep <= 0.
 * A rep whose randn runs into the chunk cap: LB_ERR_HIP, as in lb_mc_run_seeds.
 *
 * lb_joint_fetch copies the first nrep reps of the last lb_joint_draw back:
 * bits_out [nrep][U + Nv], noise_out [nrep][n], host arrays; either may be NULL. */
int lb_joint_draw(lb_ctx* ctx, int nrep, const unsigned int* seeds, int K, int U, int n, double sigma,
                  unsigned char** d_bits, double** d_noise, double* ms_out);
int lb_joint_fetch(lb_ctx* ctx, int nrep, unsigned char* bits_out, double* noise_out);

int lb_device_count(void);
const char* lb_last_error(void);
const char* lb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_BP_H */
