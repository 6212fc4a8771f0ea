// sparc_amp.hip — MI355X (gfx950) SPARC AMP decoder: kernels + C ABI.
//
// Hot path of Spimp/sparc_ldpc: the amp() loop of ldpc/sparc_ldpc.py:189-222
// over the sub-sampled Walsh-Hadamard design operator of
// ldpc/sparc_ldpc.py:32-147.  See DESIGN.md for the derivation; in short, for
// M a power of two and w = 2^ceil(log2(max(M+1, n+1))) the block of section l
// factorises as
//     A_l[r, c] = sgn(o >> log2 M) * H_M[o & (M-1), c] / sqrt(n),
//     o = ordering[l, r],  sgn(h) = (-1)^popcount(h),
// because the reference keeps the LAST M columns (w-M+c, :68/:77) of the
// natural-order Hadamard H_w, whose high index bits are all ones.  So
//     Az_l = H_M v_l / sqrt(n),  v_l[k] = sum_h sgn(h) z[inv_l[h*M + k]]
//     Ab[r] = sum_l sgn(o_lr >> log2 M) (H_M beta_l)[o_lr & (M-1)] / sqrt(n)
// with inv_l the inverse of ordering row l (sentinel n -> a zero slot).
// Per section that is one M-point FWHT (in registers + cross-lane shuffles,
// one wavefront per section) plus gathers from LDS, instead of the
// reference's w-point FWHT; no n x (L*M) matrix is ever formed.
//
// A second backend materialises the fp32 n x (L*M) matrix and streams it as
// a GEMV pair (the HBM-roofline formulation of BASELINE.json's north_star).
//
// One AMP iteration = two launches (section kernel, row kernel) replayed from
// a hipGraph captured once per (B, T, flags).  All reductions are in a fixed
// order, so results are bitwise reproducible run to run.

// 0.3: sa_profile / sa_profile_rep write 2 * sa_profile_kinds() + 1 doubles (13 since 0.2)
// 0.4: sa_profile_dispatch (dispatch-bound event pairs), sa_decide_async / sa_decide_collect
#define SA_VERSION "sparc_amp 0.6 gfx950"

#include "sa_host.h"

namespace sa {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

template <typename src_t, typename dst_t>
__global__ void k_convert(const src_t* s, dst_t* d, size_t N) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < N;
       i += (size_t)gridDim.x * blockDim.x)
    d[i] = (dst_t)s[i];
}

// Word fill used inside captured sequences instead of hipMemsetAsync (keeps
// the graphs made of kernel nodes only).
__global__ void k_fill32(uint32_t* p, uint32_t v, size_t nw) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// Fused path: the final residual of a codeword lies in the buffer of parity
// iters[b] (z double-buffered); bring it home to z (one codeword).
template <typename real>
__global__ void k_beta_final(real* beta, const real* beta2, const int* it, size_t LM) {
  const int b = blockIdx.y;
  if (!(it[b] & 1)) return;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < LM; i += (size_t)gridDim.x * blockDim.x)
    beta[(size_t)b * LM + i] = beta2[(size_t)b * LM + i];
}

__global__ void k_iters_final(int* it, int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && it[b] < 0) it[b] = T;
}


// Fused decisions of a lane moved into a ring slot (both pinned and device-mapped)
__global__ void k_copy32(const int32_t* s, int32_t* d, size_t N) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x)
    d[i] = s[i];
}

int dev_alloc(sa_ctx* c, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(SA_ERR_NOMEM, "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
  }
  c->bytes += bytes;
  return SA_OK;
}

void dev_free(void* p) {
  if (p) (void)hipFree(p);
}

// ---- decode lanes (sa_host.h: sa_lane) ---------------------------------------

int sync_all(sa_ctx* c) {
  for (auto& l : c->lane)
    if (l.stream) HIP_TRY(hipStreamSynchronize(l.stream));
  return SA_OK;
}

// Before stream s writes lane k's d_y: the other lane's copy of it must have read it.
static int y_wait_reader(sa_ctx* c, int k, hipStream_t s) {
  sa_lane& o = c->lane[1 - k];
  if (c->lanes_on && o.y_read) {
    HIP_TRY(hipStreamWaitEvent(s, o.y_ev, 0));
    o.y_read = false;
  }
  return SA_OK;
}

int y_begin_write(sa_ctx* c, int k, hipStream_t s, int B) {
  if (c->lane[k].row_B) {  // a deferred row step reads the y about to go
    sa_lane& l = c->lane[k];
    if (int rc = row_flush(c, k)) return rc;
    if (s != l.stream) {
      HIP_TRY(hipEventRecord(l.y_ev, l.stream));  // (still behind the lane's last y write)
      HIP_TRY(hipStreamWaitEvent(s, l.y_ev, 0));
    }
  }
  if (!c->lanes_on) return SA_OK;
  if (B < c->Bcap) {  // the rows past B keep the latest staged values
    if (int rc = y_sync(c, k)) return rc;
    if (s != c->lane[k].stream) HIP_TRY(hipStreamWaitEvent(s, c->lane[k].y_ev, 0));
  }
  return y_wait_reader(c, k, s);
}

int y_mark(sa_ctx* c, int k) {
  sa_lane& l = c->lane[k];
  l.y_ver = ++c->y_ver;
  c->y_lane = k;  // (y_read stays: the event recorded here lies behind the lane's earlier copy too)
  if (l.y_ev) HIP_TRY(hipEventRecord(l.y_ev, l.stream));
  return SA_OK;
}

int y_sync(sa_ctx* c, int k) {
  sa_lane& l = c->lane[k];
  if (!c->lanes_on || l.y_ver == c->y_ver) return SA_OK;
  sa_lane& src = c->lane[c->y_lane];
  if (int rcf = row_flush(c, k)) return rcf;  // a deferred row step reads the y about to go
  HIP_TRY(hipStreamWaitEvent(l.stream, src.y_ev, 0));
  if (int rc = y_wait_reader(c, k, l.stream)) return rc;
  HIP_TRY(hipMemcpyAsync(l.d_y, src.d_y, (size_t)c->Bcap * c->n * rsz(c), hipMemcpyDeviceToDevice, l.stream));
  HIP_TRY(hipEventRecord(l.y_ev, l.stream));
  l.y_ver = c->y_ver;
  l.y_read = true;
  return SA_OK;
}

// A lane's stream and events (lane 0: with the context; lane 1: at its first use).
static int lane_open(sa_lane& l) {
  if (!l.stream) HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
  if (!l.ev0) HIP_TRY(hipEventCreate(&l.ev0));
  if (!l.ev1) HIP_TRY(hipEventCreate(&l.ev1));
  if (!l.y_ev) HIP_TRY(hipEventCreateWithFlags(&l.y_ev, hipEventDisableTiming));
  return SA_OK;
}

static int beta2_alloc(sa_ctx* c, sa_lane& l, size_t nB) {
  int rc = dev_alloc(c, &l.d_beta2, nB * c->L * c->M * rsz(c));
  if (!rc) l.beta2_cap = (int)nB;
  return rc;
}

// A lane's decode buffers for nB codewords and T iterations.  What differs
// between the lanes: nBp, the codewords d_z and d_abp are padded to (lane 0:
// whole chunks of the interleaved batched layout); Gmax, the most Ab / beta^2
// partials per codeword of any kernel the lane runs; and whether d_beta2 comes
// now or with the first run that needs it (ensure_beta2).
static int lane_alloc(sa_ctx* c, sa_lane& l, size_t nB, size_t nBp, int T, int Gmax, bool beta2) {
  const size_t s = rsz(c), LM = (size_t)c->L * c->M;
  int rc;
  if ((rc = dev_alloc(c, &l.d_y, nB * c->n * s))) return rc;
  if ((rc = dev_alloc(c, &l.d_z, nBp * c->n * s))) return rc;
  if ((rc = dev_alloc(c, &l.d_beta, nB * LM * s))) return rc;
  // rows padded to 32: the row-block-major layout of the pair / triple kernels (SecArgs::pt)
  if ((rc = dev_alloc(c, &l.d_abp, nBp * Gmax * ((size_t)c->NZ16 * kRow2Rows) * s))) return rc;
  if ((rc = dev_alloc(c, &l.d_zzp, nB * c->NZh * s))) return rc;
  // tau and, behind it (256-byte aligned), the beta^2 partials in one allocation:
  // k_row2 reaches the partials at a 32-bit offset from the tau it is handed
  const size_t tau_bytes = (nB * (T + 1) * s + 255) / 256 * 256;
  if ((rc = dev_alloc(c, &l.d_tau, tau_bytes + nB * Gmax * s))) return rc;
  l.d_bbp = static_cast<char*>(l.d_tau) + tau_bytes;
  if ((rc = dev_alloc(c, (void**)&l.d_iters, nB * sizeof(int)))) return rc;
  // the fused tail's decisions: written by the last section launch, read by the host behind ev1
  if (hipHostMalloc((void**)&l.h_dec, nB * c->L * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
      hipHostGetDevicePointer((void**)&l.d_dec, l.h_dec, 0) != hipSuccess) {
    if (l.h_dec) (void)hipHostFree(l.h_dec);
    l.h_dec = l.d_dec = nullptr;
    return fail(SA_ERR_NOMEM, "hipHostMalloc(lane decisions) failed");
  }
  return beta2 ? beta2_alloc(c, l, nB) : SA_OK;
}

static void lane_free(sa_lane& l) {
  void** bufs[] = {&l.d_y, &l.d_z, &l.d_beta, &l.d_beta2, &l.d_abp, &l.d_zzp, &l.d_tau, (void**)&l.d_iters};
  for (void** p : bufs) {
    dev_free(*p);
    *p = nullptr;
  }
  l.d_bbp = nullptr;  // inside d_tau's allocation
  l.beta2_cap = 0;
  if (l.h_dec) (void)hipHostFree(l.h_dec);
  l.h_dec = l.d_dec = nullptr;
  tail_begin(l);
}

// Lane k's buffers are about to go (every lane waited for): decisions that a
// queued slot still expects in the lane's h_dec move into the ring.
static void dec_rescue(sa_ctx* c, int k) {
  for (int s = 0; s < SA_DECIDE_SLOTS; ++s)
    if (c->dec_B[s] != 0 && c->dec_lane[s] == k && c->h_dec && c->lane[k].h_dec) {
      std::memcpy(c->h_dec + (size_t)s * c->dec_cap, c->lane[k].h_dec, (size_t)c->dec_B[s] * c->L * sizeof(int32_t));
      c->dec_lane[s] = -1;  // (dec_ev[s]: recorded long ago or never; waiting for it returns at once)
    }
}

// Before a run re-records lane k's ev1 (and may overwrite its h_dec): decisions
// a queued slot still expects there move into the slot on the lane's stream,
// behind the run that wrote them, and the slot waits on its own event again.
static int dec_spill(sa_ctx* c, int k) {
  sa_lane& l = c->lane[k];
  for (int s = 0; s < SA_DECIDE_SLOTS; ++s)
    if (c->dec_B[s] != 0 && c->dec_lane[s] == k) {
      const size_t N = (size_t)c->dec_B[s] * c->L;
      k_copy32<<<(int)std::min<size_t>((N + 255) / 256, 1024), 256, 0, l.stream>>>(l.d_dec, c->d_dec + (size_t)s * c->dec_cap, N);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(c->dec_ev[s], l.stream));
      c->dec_lane[s] = -1;
    }
  return SA_OK;
}

static void stage_free(sa_lane& l) {
  dev_free(l.d_stage);
  l.d_stage = nullptr;
  l.stage_cap = 0;
}

// Lane 1's stream, events and buffers for the small-batch path (no batched-
// layout padding or partials: a lane never runs the batched kernels).
static int lane_create(sa_ctx* c) {
  sa_lane& l = c->lane[1];  // (lane 0 is current while lane 1 is off)
  if (int rco = lane_open(l)) return rco;
  const int Gmax = std::max(c->G, std::max(c->G2, c->G3));
  if (int rc = lane_alloc(c, l, c->Bcap, c->Bcap, c->Tcap, Gmax, true)) return rc;
  // the staging buffer the caller's uploads / fetches have needed so far: the
  // lane's first stage allocates nothing
  if (int rc = ensure_stage(c, l, c->lane[0].stage_cap)) return rc;
  l.y_ver = 0;  // older than any staged y: copied before the lane's first run
  l.y_read = false;
  c->lanes_on = true;
  return SA_OK;
}

// The caller is pipelining: something of the previous step is still
// outstanding when the next one is issued (its decode in flight, or decisions
// queued by sa_decide_async and not collected yet).  Only then does a run take
// the other lane: a lone decode (run, wait) stays where its buffers and its
// graph are, exactly the single-lane path.
static bool pipelining(const sa_ctx* c) {
  for (int k = 0; k < SA_DECIDE_SLOTS; ++k)
    if (c->dec_B[k] != 0) return true;
  return c->at().ev1 && hipEventQuery(c->at().ev1) == hipErrorNotReady;
}

// Whether a run of B codewords may rotate lanes at all (the plan, the backend, the batch).
static bool lane_shape(const sa_ctx* c, int B) {
  return c->backend == SA_BACKEND_HADAMARD && !use_batched(*c, B) && !(c->plan & (SA_PLAN_EAGER | SA_PLAN_NO_LANES));
}

void graphs_clear(GraphMap& m) {
  for (auto& kv : m) (void)hipGraphExecDestroy(kv.second);
  m.clear();
}

int lanes_release(sa_ctx* c) {
  int rc = sync_all(c);
  if (!c->lanes_on) return rc;
  if (!rc) dec_rescue(c, 1);
  lane_switch(c, 0);
  sa_lane &l0 = c->lane[0], &l = c->lane[1];
  if (!rc) rc = y_sync(c, 0);  // the staged y stays with lane 0
  if (!rc && l0.stream && hipStreamSynchronize(l0.stream) != hipSuccess)
    rc = fail(SA_ERR_HIP, "lanes_release: sync failed");
  graphs_clear(l.graphs);
  lane_free(l);
  stage_free(l);
  l.y_read = false;
  l0.y_read = false;
  l0.y_ver = c->y_ver;
  c->y_lane = 0;
  c->lanes_on = false;
  return rc;
}

void drop_graphs(sa_ctx* c) {
  for (auto& l : c->lane) graphs_clear(l.graphs);
  graphs_clear(c->mc_graphs);  // sa_mc_run's
}

// Lane 0's decode buffers and the buffers every lane shares.
void free_workspace(sa_ctx* c) {
  lane_free(c->lane[0]);
  void** bufs[] = {&c->d_out, &c->d_azp, &c->d_cb, &c->d_Pb, (void**)&c->d_stop, (void**)&c->d_idx};
  for (void** p : bufs) {
    dev_free(*p);
    *p = nullptr;
  }
  c->Bcap = c->Tcap = 0;
  c->h_Plb.clear();  // d_cb / d_Pb went
  if (c->pb_on) {  // the per-codeword powers went with the workspace
    c->pb_on = false;
    c->power_set = c->shared_power;
  }
}


int ensure_fgemm(sa_ctx* c, int B);

int ensure_workspace(sa_ctx* c, int B, int T) {
  if (c->backend == SA_BACKEND_DENSE) {
    int rc8 = ensure_i8(c, B > c->Bcap ? B : c->Bcap);
    if (rc8) return rc8;
  }
  if (c->backend == SA_BACKEND_MATRIX) {
    int rcf = ensure_fgemm(c, B > c->Bcap ? B : c->Bcap);
    if (rcf) return rcf;
  }
  if (B <= c->Bcap && T <= c->Tcap) return SA_OK;
  if (int rcl = lanes_release(c)) return rcl;  // waits for every lane; lane 1 returns at the next eligible run
  drop_graphs(c);
  const size_t nB = B > c->Bcap ? B : c->Bcap;
  const int nT = T > c->Tcap ? T : c->Tcap;
  dec_rescue(c, 0);  // (lanes_release waited for every lane)
  free_workspace(c);
  const size_t s = rsz(c), LM = (size_t)c->L * c->M;
  int Gmax = c->G > c->KS ? c->G : c->KS;
  if (c->backend == SA_BACKEND_DENSE && Gmax < kI8MaxS) Gmax = kI8MaxS;
  if (c->backend == SA_BACKEND_MATRIX && Gmax < kFMaxS) Gmax = kFMaxS;
  if (c->Gb > Gmax) Gmax = c->Gb;
  if (c->G2 > Gmax) Gmax = c->G2;
  if (c->G3 > Gmax) Gmax = c->G3;
  int rc;
  const size_t nBp = (nB + 3) / 4 * 4;  // whole chunks of the interleaved batched layout
  if ((rc = lane_alloc(c, c->lane[0], nB, nBp, nT, Gmax, false))) return rc;
  if ((rc = dev_alloc(c, &c->d_out, nB * (LM > (size_t)c->n ? LM : (size_t)c->n) * s))) return rc;
  if ((rc = dev_alloc(c, (void**)&c->d_stop, nB * sizeof(int)))) return rc;
  if ((rc = dev_alloc(c, (void**)&c->d_idx, nB * c->L * sizeof(int32_t)))) return rc;
  if ((rc = dev_alloc(c, &c->d_cb, nB * c->L * s))) return rc;
  if ((rc = dev_alloc(c, &c->d_Pb, nB * s))) return rc;
  if (is_dense(*c))
    if ((rc = dev_alloc(c, &c->d_azp, nB * c->RS * c->lda * s))) return rc;
  if (c->backend == SA_BACKEND_HOST)  // the caller's A^T z, one partial per codeword
    if ((rc = dev_alloc(c, &c->d_azp, nB * c->lda * s))) return rc;
  c->Bcap = (int)nB;
  c->Tcap = nT;
  return SA_OK;
}

int ensure_stage(sa_ctx* c, sa_lane& l, size_t count) {
  if (count <= l.stage_cap) return SA_OK;
  HIP_TRY(hipStreamSynchronize(l.stream));
  stage_free(l);
  int rc = dev_alloc(c, (void**)&l.d_stage, count * sizeof(double));
  if (rc) return rc;
  l.stage_cap = count;
  return SA_OK;
}

// k_convert's grid for count values: 256 per block, at least one block, at most 4096
static int convert_blocks(size_t count) { return (int)std::min<size_t>(std::max<size_t>((count + 255) / 256, 1), 4096); }

// Host fp64 -> device `real` buffer (through the fp64 staging buffer).
int upload(sa_ctx* c, sa_lane& l, void* dst, const double* src, size_t count) {
  if (c->prec == SA_PREC_F64) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * 8, hipMemcpyHostToDevice, l.stream));
    return SA_OK;
  }
  int rc = ensure_stage(c, l, count);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(l.d_stage, src, count * 8, hipMemcpyHostToDevice, l.stream));
  k_convert<double, float><<<convert_blocks(count), 256, 0, l.stream>>>(l.d_stage, (float*)dst, count);
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

int download(sa_ctx* c, sa_lane& l, double* dst, const void* src, size_t count) {
  if (c->prec == SA_PREC_F64) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * 8, hipMemcpyDeviceToHost, l.stream));
    return SA_OK;
  }
  int rc = ensure_stage(c, l, count);
  if (rc) return rc;
  k_convert<float, double><<<convert_blocks(count), 256, 0, l.stream>>>((const float*)src, l.d_stage, count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, l.d_stage, count * 8, hipMemcpyDeviceToHost, l.stream));
  return SA_OK;
}



// ---- composite sequences (all asynchronous on the current lane's stream) ----

// Ab of the batch staged in d_beta -> d_out  (B x n)
template <typename real>
int seq_ab(sa_ctx* c, int B) {
  const Plan p = plan_for(c, B);
  if (p.dense()) return dense_ab<real>(c, p, B);
  if (int rc = launch_sec<real>(c, p, B, SEC_AB, 0, 0)) return rc;
  return launch_row<real>(c, p, B, ROW_ABOUT, 0, 0, c->G, c->G);
}

// Az of the batch staged in d_z -> d_out  (B x L*M)
template <typename real>
int seq_az(sa_ctx* c, int B) {
  const Plan p = plan_for(c, B);
  if (p.dense()) return dense_az<real>(c, p, B);
  return launch_sec<real>(c, p, B, SEC_AZ, 0, 0);
}

// One launch of a decode (sa_seq.h: Step) on the current lane: side 0 / 1 of
// the estimate is d_beta / d_beta2, the decisions go to the lane's d_dec.
template <typename real>
int launch_step(sa_ctx* c, const Plan& p, int B, const Step& s) {
  sa_lane& ln = c->at();
  void* const side[2] = {ln.d_beta, ln.d_beta2};
  switch (s.kind) {
    case ST_FILL_ITERS:
      k_fill32<<<(B + 255) / 256, 256, 0, ln.stream>>>((uint32_t*)ln.d_iters, 0xffffffffu, (size_t)B);
      break;
    case ST_ZERO_BETA: {
      const size_t nw = (size_t)B * c->L * c->M * rsz(c) / 4;
      k_fill32<<<(int)std::min<size_t>((nw + 255) / 256, 8192), 256, 0, ln.stream>>>((uint32_t*)ln.d_beta, 0u, nw);
      break;
    }
    case ST_DENSE_START: return dense_start<real>(c, p, B);
    case ST_SEC_AB: return launch_sec<real>(c, p, B, SEC_AB, 0, 0);
    case ST_ROW: return launch_row<real>(c, p, B, s.mode, s.t, s.es, s.G, s.Gb, s.itset);
    case ST_SEC: return launch_sec<real>(c, p, B, SEC_AMP, s.t, s.es, side[s.rd], side[s.wr]);
    case ST_SEC_MW:
      return launch_sec2<real>(c, p, B, s.t, s.es, side[s.rd], side[s.wr], s.bzero, s.decide ? ln.d_dec : nullptr, s.itset);
    case ST_SEC_B: return launch_secb<real>(c, p, B, s.t, s.es);
    case ST_DENSE_ITER: return dense_iter<real>(c, p, B, s.t, s.es);
    case ST_ITERS_FINAL:
      k_iters_final<<<(B + 255) / 256, 256, 0, ln.stream>>>(ln.d_iters, B, s.itset);
      break;
    case ST_BETA_FINAL: {
      const size_t LM = (size_t)c->L * c->M;
      k_beta_final<real><<<dim3((unsigned)std::min<size_t>((LM + 255) / 256, 4096), B), 256, 0, ln.stream>>>(
          (real*)ln.d_beta, (const real*)ln.d_beta2, ln.d_iters, LM);
      break;
    }
  }
  HIP_TRY(hipGetLastError());
  return SA_OK;
}

// Whole AMP decode q (sa_seq.h: decode_seq) of the staged batch on the current
// lane: y in d_y, beta0 in d_beta.
template <typename real>
int seq_amp(sa_ctx* c, const Plan& p, int B, const DecodeSeq& q) {
  return for_each_step(q, [&](const Step& s) { return launch_step<real>(c, p, B, s); });
}

int row_flush(sa_ctx* c, int k) {
  int B, T;
  if (!tail_take_row(c->lane[k], &B, &T)) return SA_OK;
  const int keep = c->cur;
  const Plan p = plan_for(c, B);  // the run's own: (context, B) decide it
  const Step row = deferred_row(p, T);
  lane_switch(c, k);  // the launchers address the current lane
  const int rc = c->prec == SA_PREC_F64 ? launch_step<double>(c, p, B, row) : launch_step<float>(c, p, B, row);
  lane_switch(c, keep);
  return rc;
}

int ensure_beta2(sa_ctx* c, int B) {
  if (is_dense(*c) || use_batched(*c, B) || c->at().beta2_cap >= c->Bcap) return SA_OK;
  if (int rcl = lanes_release(c)) return rcl;
  // lane 0 has none yet (lane 1 is created with its own; a grown workspace drops lane 0's)
  if (int rc = beta2_alloc(c, c->lane[0], c->Bcap)) return rc;
  drop_graphs(c);  // captured graphs hold the old pointer
  return SA_OK;
}

template <typename real>
int run_graph(sa_ctx* c, int B, int T, int flags, int has_b0) {
  int rc0 = ensure_beta2(c, B);
  if (!rc0 && use_batched(*c, B)) rc0 = ensure_invb(c);  // before any capture: it uploads
  if (rc0) return rc0;
  // Decode lanes: a small-batch graph decode without beta0, issued while the
  // previous step is outstanding, takes the lane the previous run did not, so
  // consecutive decodes overlap on the chip; every other run stays on the
  // current lane.  Lane 1 appears at the first such run.
  if (lane_shape(c, B) && !c->prof && !has_b0 && pipelining(c)) {
    if (!c->lanes_on)
      if (int rcl = lane_create(c)) return rcl;
    lane_switch(c, 1 - c->cur);
  } else if (use_batched(*c, B)) {
    lane_switch(c, 0);  // lane 1's buffers hold no batched layout (no chunk padding, no k_secb partials)
  }
  {
    sa_lane& l = c->at();  // the run's lane: cur is settled
    int rb, rt;
    (void)tail_take_row(l, &rb, &rt);  // dropped, before y_sync would flush it
    if (int rcd = dec_spill(c, c->cur)) return rcd;
    tail_begin(l);
  }
  if (int rcy = y_sync(c)) return rcy;  // a lane whose y is older than the latest staged one
  sa_lane& ln = c->at();
  const Plan p = plan_for(c, B);  // the kernels of this decode and their partial counts
  const DecodeSeq q = decode_seq(*c, p, T, flags, has_b0 != 0, c->prof != nullptr);
  hipGraphExec_t graph = nullptr;  // stays null: eager launches instead of the captured graph
  if (!(c->plan & SA_PLAN_EAGER)) {
    // the power-allocation mode selects the captured kernel arguments (c, P arrays)
    const auto key = std::make_tuple(B, T, flags | (c->pb_on ? 0x10000 : 0), has_b0);
    auto it = ln.graphs.find(key);
    if (it == ln.graphs.end()) {
      hipGraphExec_t ex = nullptr;
      if (int rc = capture_graph(ln.stream, [&] { return seq_amp<real>(c, p, B, q); }, &ex)) return rc;
      it = ln.graphs.emplace(key, ex).first;
    }
    graph = it->second;
  }
  HIP_TRY(hipEventRecord(ln.ev0, ln.stream));
  if (graph) {
    HIP_TRY(hipGraphLaunch(graph, ln.stream));
  } else if (int rc = seq_amp<real>(c, p, B, q)) {
    return rc;
  }
  HIP_TRY(hipEventRecord(ln.ev1, ln.stream));
  tail_issued(c, B, q);
  c->last_B = B;
  c->last_T = T;
  return SA_OK;
}

int check_ctx(const sa_ctx* c) {
  if (!c) return fail(SA_ERR_ARG, "null context");
  return SA_OK;
}

// Entry points that read the Hadamard design's tables (the row-parallel
// encoder and cancellation: one table entry per section and row).
int check_tables(const sa_ctx* c, const char* what) {
  if (!c) return fail(SA_ERR_ARG, "null context");
  if (c->backend != SA_BACKEND_HADAMARD && c->backend != SA_BACKEND_DENSE)
    return fail(SA_ERR_UNSUPPORTED, std::string(what) + ": needs a design built from an ordering "
                                                        "(use sa_Ab for a caller's matrix)");
  return SA_OK;
}

// Entry points that apply the design operator on the device: not on a
// host-operator context (SA_BACKEND_HOST holds no operator).
int check_op(const sa_ctx* c, const char* what) {
  if (!c) return fail(SA_ERR_ARG, "null context");
  if (c->backend == SA_BACKEND_HOST)
    return fail(SA_ERR_UNSUPPORTED, std::string(what) + ": a host-operator context has no device operator");
  return SA_OK;
}

// The caller's section vectors [B][L][Mu] <-> the device's padded layout
// [B][L][M] (a padded section's dead leading columns zero); identity when M
// is the caller's.
int upload_sections(sa_ctx* c, void* dst, const double* src, int B) {
  const size_t LM = (size_t)c->L * c->M;
  if (c->dead == 0) return upload(c, dst, src, (size_t)B * LM);
  std::vector<double> pad((size_t)B * LM, 0.0);
  for (size_t bl = 0; bl < (size_t)B * c->L; ++bl)
    std::memcpy(pad.data() + bl * c->M + c->dead, src + bl * c->Mu, (size_t)c->Mu * sizeof(double));
  int rc = upload(c, dst, pad.data(), pad.size());
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));  // pad is a host temporary
  return SA_OK;
}

int download_sections(sa_ctx* c, double* dst, const void* src, int B) {
  const size_t LM = (size_t)c->L * c->M;
  if (c->dead == 0) return download(c, dst, src, (size_t)B * LM);
  std::vector<double> pad((size_t)B * LM);
  int rc = download(c, pad.data(), src, pad.size());
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  for (size_t bl = 0; bl < (size_t)B * c->L; ++bl)
    std::memcpy(dst + bl * c->Mu, pad.data() + bl * c->M + c->dead, (size_t)c->Mu * sizeof(double));
  return SA_OK;
}

int set_power(sa_ctx* c, const double* Pl) {
  if (!Pl) return fail(SA_ERR_ARG, "Pl is NULL");
  std::vector<double> cl(c->L);
  double P = 0;
  for (int l = 0; l < c->L; ++l) {
    if (!(Pl[l] >= 0)) return fail(SA_ERR_ARG, "Pl must be non-negative");
    cl[l] = std::sqrt((double)c->n * Pl[l]);  // np.sqrt(n*Pl), sparc_ldpc.py:214
    P += Pl[l];                                // np.sum(Pl), sparc_ldpc.py:190
  }
  // (a deferred row step reads P as its decode did: before any change of mode or value)
  for (int k = 0; k < sa_ctx::kLanes; ++k)
    if (int rcf = row_flush(c, k)) return rcf;
  // A decode in flight on either lane reads d_c / d_P1: an unchanged Pl (a
  // caller passing it with every stage) writes nothing, a new one waits for
  // every lane first.
  const bool same = c->h_Pl.size() == (size_t)c->L && std::memcmp(c->h_Pl.data(), Pl, (size_t)c->L * 8) == 0;
  if (same) {
    c->pb_on = false;
    c->shared_power = true;
    c->power_set = true;
    return SA_OK;
  }
  if (int rcs = sync_all(c)) return rcs;
  c->h_Pl.clear();
  c->P = P;
  c->cmax = 0;
  for (int l = 0; l < c->L; ++l) c->cmax = cl[l] > c->cmax ? cl[l] : c->cmax;
  int rc = upload(c, c->d_c, cl.data(), c->L);
  if (!rc) rc = upload(c, c->d_P1, &P, 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_cd, cl.data(), (size_t)c->L * 8, hipMemcpyHostToDevice, c->at().stream));
  HIP_TRY(hipStreamSynchronize(c->at().stream));  // cl is a host temporary
  c->pb_on = false;  // back to one allocation (graphs are keyed on the mode)
  c->shared_power = true;
  c->power_set = true;
  if (c->d_bfix && (rc = i8_set_bfix(c))) return rc;
  c->h_Pl.assign(Pl, Pl + c->L);
  return SA_OK;
}

// Per-codeword power allocations Pl [B][L] for the next runs of B' <= B
// codewords (c_{b,l} = sqrt(n Pl_{b,l}), P_b = sum_l Pl_{b,l}).  A section with
// Pl = 0 has c = 0, so its estimate stays exactly 0 (beta = c e / S) and it
// adds nothing to A beta or to sum(beta^2): AMP over the remaining sections
// with the same n, i.e. the reference's sparc_transforms_shorter decode
// (amp_exit.py:113-116) as a mask, per codeword, in one batch.
int set_power_batch(sa_ctx* c, int B, const double* Pl) {
  if (!Pl) return fail(SA_ERR_ARG, "Pl is NULL");
  if (is_dense(*c)) return fail(SA_ERR_UNSUPPORTED, "per-codeword power: Hadamard backend only");
  const size_t L = (size_t)c->L;
  for (int k = 0; k < sa_ctx::kLanes; ++k)
    if (int rcf = row_flush(c, k)) return rcf;
  // as set_power: unchanged allocations write nothing, new ones wait for every lane
  if (c->h_Plb.size() == (size_t)B * L && std::memcmp(c->h_Plb.data(), Pl, (size_t)B * L * 8) == 0) {
    c->pb_on = true;
    c->power_set = true;
    return SA_OK;
  }
  if (int rcs = sync_all(c)) return rcs;
  c->h_Plb.clear();
  std::vector<double> cb((size_t)B * L), Pb(B);
  for (int b = 0; b < B; ++b) {
    double P = 0;
    for (size_t l = 0; l < L; ++l) {
      const double p = Pl[(size_t)b * L + l];
      if (!(p >= 0)) return fail(SA_ERR_ARG, "Pl must be non-negative");
      cb[(size_t)b * L + l] = std::sqrt((double)c->n * p);
      P += p;
    }
    Pb[b] = P;
  }
  int rc = upload(c, c->d_cb, cb.data(), (size_t)B * L);
  if (!rc) rc = upload(c, c->d_Pb, Pb.data(), (size_t)B);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  c->pb_on = true;
  c->power_set = true;
  c->h_Plb.assign(Pl, Pl + (size_t)B * L);
  return SA_OK;
}

// Every section-kernel instantiation may use the full 160 KB LDS, the MFMA
// GEMMs their staging buffers (once per process).
int set_lds_limits() {
  static int done = 0;
  if (done) return SA_OK;
  if (!secb_no_static_lds())
    return fail(SA_ERR_HIP, "k_secb has static LDS: absolute LDS addressing in gather_step4 is invalid");
  hipError_t e = sec_lds_attrs();
  if (e == hipSuccess) e = secb_lds_attrs();
  if (e == hipSuccess) e = dense_lds_attrs();
  if (e == hipSuccess) e = mc_lds_attrs();
  if (e != hipSuccess) return fail(SA_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
  done = 1;
  return SA_OK;
}

int create_impl(sa_ctx** out, int L, int M, int n, const uint32_t* ordering, int backend, int prec,
                int device, int plan, const sa_ctx* share) {
  if (!out) return fail(SA_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (L <= 0 || M <= 0 || n <= 0) return fail(SA_ERR_ARG, "L, M, n must be positive");
  if (backend != SA_BACKEND_HADAMARD && backend != SA_BACKEND_DENSE && backend != SA_BACKEND_HOST &&
      backend != SA_BACKEND_MATRIX)
    return fail(SA_ERR_ARG, "unknown backend");
  if (!ordering && backend != SA_BACKEND_HOST && backend != SA_BACKEND_MATRIX)
    return fail(SA_ERR_ARG, "ordering is NULL");
  if (prec != SA_PREC_F32 && prec != SA_PREC_F64) return fail(SA_ERR_ARG, "unknown precision");
  if (plan & ~SA_PLAN_ALL) return fail(SA_ERR_ARG, "unknown plan option bits");
  if (backend == SA_BACKEND_DENSE && prec != SA_PREC_F32)
    return fail(SA_ERR_UNSUPPORTED, "dense backend streams an fp32 matrix (precision must be F32)");
  std::string err;
  if (int rcl = shape_limits(M, n, backend, err)) return fail(rcl, err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SA_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(SA_ERR_ARG, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  int n_cus = Shape().n_cus;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      n_cus = prop.multiProcessorCount;
  }

  sa_ctx* c = new sa_ctx();
  if (int rcs = shape_for(*c, L, M, n, backend, prec, plan, n_cus, err)) {  // every shape number (sa_shape.h)
    delete c;
    return fail(rcs, err);
  }
  c->device = device;
  if (ordering) c->ordering.assign(ordering, ordering + (size_t)L * n);
  const size_t s = rsz(c);
  if (lane_open(c->lane[0]) != SA_OK) {
    delete c;
    return fail(SA_ERR_HIP, "stream/event creation failed");
  }
  int rc = SA_OK;
  if (backend == SA_BACKEND_DENSE) {
    c->RS = 8;
    c->KS = 8;
    rc = build_tables(c);  // validates the ordering (distinct values in [1, w))
    if (!rc) rc = build_dense(c);
  } else if (backend == SA_BACKEND_HOST) {
    c->lda = (size_t)L * M;  // no operator on the device: the caller's products are uploaded
  } else if (backend == SA_BACKEND_MATRIX) {
    // the caller's matrix, uploaded by sa_create_matrix (sa_dense.hip)
    c->RS = 8;
    c->KS = 8;
    rc = matrix_init(c);
  } else if (share) {  // sa_create_twin: the same tables, read-only, borrowed
    c->tab = share->tab;
    c->borrowed = true;
  } else {
    rc = build_tables(c);
  }
  if (!rc) rc = dev_alloc(c, &c->d_c, (size_t)L * s);
  if (!rc) rc = dev_alloc(c, (void**)&c->d_cd, (size_t)L * 8);
  if (!rc) rc = dev_alloc(c, &c->d_P1, s);
  if (rc) {
    sa_destroy(c);
    return rc;
  }
  if ((rc = set_lds_limits())) {
    sa_destroy(c);
    return rc;
  }
  *out = c;
  return SA_OK;
}

}  // namespace sa

using namespace sa;

extern "C" {

int sa_create(sa_ctx** out, int L, int M, int n, const uint32_t* ordering, int backend, int precision,
              int device) {
  return create_impl(out, L, M, n, ordering, backend, precision, device, SA_PLAN_DEFAULT);
}

int sa_create_ex(sa_ctx** out, int L, int M, int n, const uint32_t* ordering, int backend, int precision,
                 int device, int plan) {
  return create_impl(out, L, M, n, ordering, backend, precision, device, plan);
}


int sa_subset(const sa_ctx* parent, const int64_t* sections, int Ls, sa_ctx** out) {
  if (int rc0 = check_tables(parent, "sa_subset")) return rc0;
  if (!sections || Ls <= 0) return fail(SA_ERR_ARG, "empty section subset");
  std::vector<uint32_t> ord((size_t)Ls * parent->n);
  for (int i = 0; i < Ls; ++i) {
    int64_t s = sections[i];
    if (s < 0) s += parent->L;  // numpy negative indexing
    if (s < 0 || s >= parent->L) return fail(SA_ERR_ARG, "section index out of range");
    std::memcpy(ord.data() + (size_t)i * parent->n, parent->ordering.data() + (size_t)s * parent->n,
                (size_t)parent->n * 4);
  }
  return create_impl(out, Ls, parent->Mu, parent->n, ord.data(), parent->backend, parent->prec, parent->device,
                     parent->plan);
}

int sa_create_twin(sa_ctx* src, sa_ctx** out) {
  if (!out) return fail(SA_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (check_ctx(src)) return SA_ERR_ARG;
  if (src->backend != SA_BACKEND_HADAMARD)
    return fail(SA_ERR_UNSUPPORTED, "sa_create_twin: Hadamard-backend contexts only");
  HIP_TRY(hipSetDevice(src->device));
  // the lazily built batched-kernel tables first, so that both contexts use them
  if (int rc = ensure_invb(src)) return rc;
  return create_impl(out, src->L, src->Mu, src->n, src->ordering.data(), src->backend, src->prec, src->device,
                     src->plan, src);
}

void sa_destroy(sa_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)lanes_release(c);  // waits for every lane; lane 0 is current from here
  drop_graphs(c);
  free_workspace(c);
  mc_release(c);
  if (!c->borrowed) tables_free(c->tab);
  dev_free(c->d_A);
  dev_free(c->d_AT); dev_free(c->d_xz); dev_free(c->d_xb);
  dev_free(c->d_A8); dev_free(c->d_AT8); dev_free(c->d_zq); dev_free(c->d_bq);
  dev_free(c->d_zsc); dev_free(c->d_bsc0); dev_free(c->d_bfix);
  dev_free(c->d_c);
  dev_free(c->d_cd);
  dev_free(c->d_P1);
  for (auto& e : c->dec_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->h_dec) (void)hipHostFree(c->h_dec);
  for (auto& l : c->lane) {
    stage_free(l);
    if (l.y_ev) (void)hipEventDestroy(l.y_ev);
    if (l.ev0) (void)hipEventDestroy(l.ev0);
    if (l.ev1) (void)hipEventDestroy(l.ev1);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  delete c;
}

int sa_Ab(sa_ctx* c, int B, const double* beta, double* out) {
  if (int rc0 = check_op(c, "sa_Ab")) return rc0;
  if (B <= 0 || !beta || !out) return fail(SA_ERR_ARG, "sa_Ab: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, c->Tcap > 0 ? c->Tcap : 1);
  if (rc) return rc;
  if ((rc = tail_settle(c))) return rc;  // d_beta and the partials change
  if ((rc = upload_sections(c, c->at().d_beta, beta, B))) return rc;
  rc = c->prec == SA_PREC_F64 ? seq_ab<double>(c, B) : seq_ab<float>(c, B);
  if (rc) return rc;
  if ((rc = download(c, out, c->d_out, (size_t)B * c->n))) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

int sa_Az(sa_ctx* c, int B, const double* z, double* out) {
  if (int rc0 = check_op(c, "sa_Az")) return rc0;
  if (B <= 0 || !z || !out) return fail(SA_ERR_ARG, "sa_Az: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, c->Tcap > 0 ? c->Tcap : 1);
  if (rc) return rc;
  if ((rc = row_flush(c, c->cur))) return rc;  // in stream order in front of the new z, as the decode's last row step was
  if ((rc = upload(c, c->at().d_z, z, (size_t)B * c->n))) return rc;
  c->zil_last = false;  // d_z holds [B][n] now
  if (c->prec == SA_PREC_F64) {
    rc = seq_az<double>(c, B);
  } else {
    rc = seq_az<float>(c, B);
  }
  if (rc) return rc;
  if ((rc = download_sections(c, out, c->d_out, B))) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

int sa_reserve(sa_ctx* c, int B, int T) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || T < 0) return fail(SA_ERR_ARG, "sa_reserve: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, T > 0 ? T : 1);
  // the batched kernel's tables (built once per operator) now, not at the first decode
  if (!rc && c->backend == SA_BACKEND_HADAMARD && use_batched(*c, B)) rc = ensure_invb(c);
  return rc;
}

int sa_stage(sa_ctx* c, int B, const double* y, const double* Pl, const double* beta0) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0) return fail(SA_ERR_ARG, "sa_stage: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, c->Tcap > 0 ? c->Tcap : 1);
  if (rc) return rc;
  if (Pl && (rc = set_power(c, Pl))) return rc;
  if (y) {  // NULL: keep the staged y
    // Into the lane the next run will take, on that lane's stream: a decode in
    // flight on the current lane is not waited for.  (A run that takes another
    // lane after all copies y over first: y_sync.)  With beta0 the next run is
    // a beta0 run, which stays on the current lane.
    const bool rotate = c->lanes_on && !beta0 && lane_shape(c, B) && pipelining(c);
    const int k = rotate ? 1 - c->cur : c->cur;
    sa_lane& l = c->lane[k];
    rc = y_begin_write(c, k, l.stream, B);
    if (!rc) rc = upload(c, l, l.d_y, y, (size_t)B * c->n);
    if (!rc) rc = y_mark(c, k);
    if (rc) return rc;
  }
  if (beta0) {
    tail_beta_rewritten(c->at());
    if ((rc = upload_sections(c, c->at().d_beta, beta0, B))) return rc;
  }
  return SA_OK;
}

int sa_stage_power_batch(sa_ctx* c, int B, const double* Pl) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0) return fail(SA_ERR_ARG, "sa_stage_power_batch: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, c->Tcap > 0 ? c->Tcap : 1);
  if (rc) return rc;
  return set_power_batch(c, B, Pl);
}

int sa_run(sa_ctx* c, int B, int T, int flags) {
  if (int rc0 = check_op(c, "sa_run")) return rc0;
  if (B <= 0 || T < 0) return fail(SA_ERR_ARG, "sa_run: bad arguments");
  if (!c->power_set) return fail(SA_ERR_ARG, "sa_run: power allocation not staged");
  if (B > c->Bcap) return fail(SA_ERR_ARG, "sa_run: batch larger than the staged batch");
  HIP_TRY(hipSetDevice(c->device));
  if (T > c->Tcap) {
    // growing T reallocates the workspace; keep the staged inputs
    return fail(SA_ERR_ARG, "sa_run: T larger than the workspace (call sa_reserve first)");
  }
  const int has_b0 = (flags & SA_FLAG_BETA0) ? 1 : 0;
  return c->prec == SA_PREC_F64 ? run_graph<double>(c, B, T, flags & 0xff, has_b0)
                                : run_graph<float>(c, B, T, flags & 0xff, has_b0);
}

int sa_wait(sa_ctx* c) {
  if (check_ctx(c)) return SA_ERR_ARG;
  HIP_TRY(hipSetDevice(c->device));
  return sync_all(c);  // every lane
}

double sa_run_event_ms(sa_ctx* c) {
  if (!c) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, c->at().ev0, c->at().ev1) != hipSuccess) return -1.0;
  return ms;
}

int sa_fetch_z(sa_ctx* c, int B, double* z_out) {
  if (check_ctx(c) || !z_out) return fail(SA_ERR_ARG, "sa_fetch_z: bad arguments");
  if (B <= 0 || B > c->Bcap) return fail(SA_ERR_ARG, "sa_fetch_z: bad batch");
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = row_flush(c, c->cur))) return rc;  // z_T of a fused-tail decode: its last row step runs now
  if (c->zil_last) {  // [NC][n][CB] -> [B][n]
    const int CB = 16 / (int)rsz(c), NC = (B + CB - 1) / CB;
    std::vector<double> il((size_t)NC * CB * c->n);
    if ((rc = download(c, il.data(), c->at().d_z, il.size()))) return rc;
    HIP_TRY(hipStreamSynchronize(c->at().stream));
    for (int b = 0; b < B; ++b)
      for (int r = 0; r < c->n; ++r) z_out[(size_t)b * c->n + r] = il[((size_t)(b / CB) * c->n + r) * CB + b % CB];
    return SA_OK;
  }
  if ((rc = download(c, z_out, c->at().d_z, (size_t)B * c->n))) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

int sa_fetch_y(sa_ctx* c, int B, double* y_out) {
  if (check_ctx(c) || !y_out) return fail(SA_ERR_ARG, "sa_fetch_y: bad arguments");
  if (B <= 0 || B > c->Bcap) return fail(SA_ERR_ARG, "sa_fetch_y: bad batch");
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = y_sync(c))) return rc;  // the y the next run would read, wherever it was staged
  if ((rc = download(c, y_out, c->at().d_y, (size_t)B * c->n))) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

int sa_fetch(sa_ctx* c, int B, double* beta_out, int* iters_out) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || B > c->Bcap) return fail(SA_ERR_ARG, "sa_fetch: bad batch");
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (beta_out && (rc = download_sections(c, beta_out, c->at().d_beta, B))) return rc;
  const sa_lane& ln = c->at();
  if (iters_out) HIP_TRY(hipMemcpyAsync(iters_out, ln.d_iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, ln.stream));
  HIP_TRY(hipStreamSynchronize(ln.stream));
  return SA_OK;
}

int sa_amp(sa_ctx* c, int B, const double* y, const double* Pl, int T, const double* beta0, double* beta_out,
           int* iters_out, int flags) {
  if (int rc0 = check_op(c, "sa_amp")) return rc0;
  if (B <= 0 || T < 0 || !y || !Pl || !beta_out) return fail(SA_ERR_ARG, "sa_amp: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_workspace(c, B, T > 0 ? T : 1);
  if (rc) return rc;
  if ((rc = sa_stage(c, B, y, Pl, beta0))) return rc;
  if (T == 0) {
    // the loop body never runs: beta is beta0 (or zeros)
    tail_beta_rewritten(c->at());
    if (!beta0) HIP_TRY(hipMemsetAsync(c->at().d_beta, 0, (size_t)B * c->L * c->M * rsz(c), c->at().stream));
    HIP_TRY(hipMemsetAsync(c->at().d_iters, 0, (size_t)B * sizeof(int), c->at().stream));
  } else {
    if ((rc = sa_run(c, B, T, (flags & 0xff) | (beta0 ? SA_FLAG_BETA0 : 0)))) return rc;
  }
  return sa_fetch(c, B, beta_out, iters_out);
}

int sa_profile(sa_ctx* c, int B, int T, int flags, double* out) { return sa_profile_rep(c, B, T, flags, 1, out); }

int sa_profile_kinds(void) { return K_NKINDS; }

extern "C++" {
namespace {
int profile_impl(sa_ctx* c, int B, int T, int flags, int rep, bool dispatch, double* out) {
  if (int rc0 = check_op(c, "sa_profile")) return rc0;
  if (B <= 0 || T <= 0 || !out || B > c->Bcap || T > c->Tcap || !c->power_set || rep < 1 || rep > 1024)
    return fail(SA_ERR_ARG, "sa_profile: bad arguments (reserve and stage first)");
  HIP_TRY(hipSetDevice(c->device));
  if (int rcs = sync_all(c)) return rcs;  // the profiled decode has the chip to itself (it stays on the current lane)
  if (int rcb = ensure_beta2(c, B)) return rcb;
  if (use_batched(*c, B)) lane_switch(c, 0);  // as sa_run
  tail_begin(c->at());
  if (int rcy = y_sync(c)) return rcy;
  if (use_batched(*c, B))
    if (int rci = ensure_invb(c)) return rci;
  Prof prof;
  prof.rep = rep;
  prof.dispatch = dispatch;
  c->prof = &prof;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, c->at().stream));
  const Plan p = plan_for(c, B);
  const DecodeSeq q = decode_seq(*c, p, T, flags & 0xff, (flags & SA_FLAG_BETA0) != 0, true);  // never a fused tail
  int rc = c->prec == SA_PREC_F64 ? seq_amp<double>(c, p, B, q) : seq_amp<float>(c, p, B, q);
  tail_issued(c, B, q);
  c->prof = nullptr;
  (void)hipEventRecord(e1, c->at().stream);
  hipError_t e = hipStreamSynchronize(c->at().stream);
  if (rc == SA_OK && e != hipSuccess) rc = fail(SA_ERR_HIP, std::string("sa_profile: ") + hipGetErrorString(e));
  double sum[K_NKINDS] = {0}, cnt[K_NKINDS] = {0};
  if (rc == SA_OK) {
    for (auto& ev : prof.ev) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, std::get<1>(ev), std::get<2>(ev)) == hipSuccess) {
        sum[std::get<0>(ev)] += ms / rep;
        cnt[std::get<0>(ev)] += 1;
      }
    }
    float tot = 0.f;
    (void)hipEventElapsedTime(&tot, e0, e1);
    for (int k = 0; k < K_NKINDS; ++k) {
      out[2 * k] = cnt[k] > 0 ? sum[k] / cnt[k] : 0.0;
      out[2 * k + 1] = cnt[k];
    }
    out[2 * K_NKINDS] = tot;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}
}  // namespace
}  // extern "C++"

int sa_profile_rep(sa_ctx* c, int B, int T, int flags, int rep, double* out) {
  return profile_impl(c, B, T, flags, rep, false, out);
}

int sa_profile_dispatch(sa_ctx* c, int B, int T, int flags, double* out) {
  return profile_impl(c, B, T, flags, 1, true, out);
}


int sa_decide(sa_ctx* c, int B, int32_t* idx_out) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || B > c->Bcap || !idx_out) return fail(SA_ERR_ARG, "sa_decide: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  if (c->at().fused_B >= B) {  // the last section launch decided
    HIP_TRY(hipStreamSynchronize(c->at().stream));
    std::memcpy(idx_out, c->at().h_dec, (size_t)B * c->L * sizeof(int32_t));
    return SA_OK;
  }
  if (int rc = launch_decide(c, B, c->d_idx)) return rc;
  HIP_TRY(hipMemcpyAsync(idx_out, c->d_idx, (size_t)B * c->L * sizeof(int32_t), hipMemcpyDeviceToHost, c->at().stream));
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

int sa_decide_async(sa_ctx* c, int B, int slot) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (B <= 0 || B > c->Bcap || slot < 0 || slot >= SA_DECIDE_SLOTS)
    return fail(SA_ERR_ARG, "sa_decide_async: bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  const size_t per = (size_t)c->Bcap * c->L;  // one slot holds a whole staged batch
  if (!c->h_dec || c->dec_cap < per) {
    // a larger staged batch regrows the ring: refused while another slot still
    // holds decisions not collected (they would be dropped)
    for (int k = 0; k < SA_DECIDE_SLOTS; ++k)
      if (c->h_dec && c->dec_B[k] != 0)
        return fail(SA_ERR_ARG, "sa_decide_async: the staged batch grew while slot " + std::to_string(k) +
                                    " holds decisions not yet collected (sa_decide_collect them first)");
    if (int rcs = sync_all(c)) return rcs;  // either lane's k_decide may still write the old ring
    if (c->h_dec) (void)hipHostFree(c->h_dec);
    c->h_dec = nullptr;
    c->d_dec = nullptr;
    c->dec_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&c->h_dec, per * SA_DECIDE_SLOTS * sizeof(int32_t), hipHostMallocDefault));
    HIP_TRY(hipHostGetDevicePointer((void**)&c->d_dec, c->h_dec, 0));
    c->dec_cap = per;
    for (int k = 0; k < SA_DECIDE_SLOTS; ++k) {
      if (!c->dec_ev[k]) HIP_TRY(hipEventCreateWithFlags(&c->dec_ev[k], hipEventDisableTiming));
      c->dec_B[k] = 0;
      c->dec_lane[k] = -1;
    }
  }
  if (c->at().fused_B >= B) {
    // the run's last section launch wrote them into its lane's pinned buffer,
    // marked by the lane's ev1: nothing to enqueue, the slot remembers the lane
    c->dec_lane[slot] = c->cur;
    c->dec_B[slot] = B;
    return SA_OK;
  }
  c->dec_lane[slot] = -1;
  // k_decide writes the indices straight into the slot (the pinned ring is
  // mapped into the device's address space: no copy behind the kernel); the
  // host reads them after the event recorded behind it
  if (int rc = launch_decide(c, B, c->d_dec + (size_t)slot * c->dec_cap)) return rc;
  HIP_TRY(hipEventRecord(c->dec_ev[slot], c->at().stream));
  c->dec_B[slot] = B;
  return SA_OK;
}

int sa_decide_collect(sa_ctx* c, int B, int slot, int32_t* idx_out) {
  if (check_ctx(c)) return SA_ERR_ARG;
  if (slot < 0 || slot >= SA_DECIDE_SLOTS || !idx_out || !c->h_dec || c->dec_B[slot] != B || B <= 0)
    return fail(SA_ERR_ARG, "sa_decide_collect: no decision of this batch queued in the slot");
  HIP_TRY(hipSetDevice(c->device));
  if (const int k = c->dec_lane[slot]; k >= 0) {  // fused decisions, still in their lane
    HIP_TRY(hipEventSynchronize(c->lane[k].ev1));
    std::memcpy(idx_out, c->lane[k].h_dec, (size_t)B * c->L * sizeof(int32_t));
    c->dec_B[slot] = 0;
    c->dec_lane[slot] = -1;
    return SA_OK;
  }
  HIP_TRY(hipEventSynchronize(c->dec_ev[slot]));
  std::memcpy(idx_out, c->h_dec + (size_t)slot * c->dec_cap, (size_t)B * c->L * sizeof(int32_t));
  c->dec_B[slot] = 0;
  return SA_OK;
}


int sa_plan(sa_ctx* c, int B, int64_t* o) {
  if (check_ctx(c) || !o || B <= 0) return fail(SA_ERR_ARG, "sa_plan: bad arguments");
  const Plan p = plan_for(c, B);
  o[0] = p.sec;
  o[1] = p.G;
  o[2] = (p.sec == SA_SEC_K_SEC || p.sec == SA_SEC_K_SECG) ? p.rs : 1;  // the loop's k_sec / k_secg launches
  o[3] = p.CB;
  o[4] = p.nz;
  o[5] = c->w;
  o[6] = p.row;
  o[7] = c->n_cus;
  return SA_OK;
}

int sa_plan_batched(sa_ctx* c, int B, int64_t* o) {
  if (check_ctx(c) || !o || B <= 0) return fail(SA_ERR_ARG, "sa_plan_batched: bad arguments");
  if (is_dense(*c) || !use_batched(*c, B)) return fail(SA_ERR_ARG, "sa_plan_batched: this batch does not run k_secb");
  const SecbOrder so = secb_order(*c, B);
  o[0] = c->Gb;
  o[1] = c->WB;
  o[2] = so.gp;
  o[3] = so.passes;
  return SA_OK;
}

int sa_info(const sa_ctx* c, int64_t* o) {
  if (check_ctx(c) || !o) return fail(SA_ERR_ARG, "sa_info: bad arguments");
  o[0] = c->L; o[1] = c->Mu; o[2] = c->n; o[3] = c->w; o[4] = c->backend; o[5] = c->prec;
  o[6] = c->device; o[7] = (int64_t)c->bytes;
  return SA_OK;
}

int sa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* sa_last_error(void) { return g_err.c_str(); }

const char* sa_version(void) { return SA_VERSION; }

#ifdef SA_STAMPS
int sa_debug_stamps(unsigned long long* out) {
  // each unit keeps its own stamp buffer; the stamped kernel's is the non-zero one
  HIP_TRY(hipDeviceSynchronize());
  std::memset(out, 0, sizeof(unsigned long long) * 16 * 16);
  HIP_TRY(stamps_add_sec(out));
  HIP_TRY(stamps_add_secb(out));
  return SA_OK;
}
#endif

}  // extern "C"