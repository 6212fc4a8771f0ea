// ldpc_mc.hip — the LDPC-only Monte-Carlo simulators (sim_ldpc,
// sparc_ldpc.py:1064-1124; ldpc/py/ldpc_awgn.py:60-123; ldpc/ldpc_bsc.py:63-113)
// around the belief-propagation decoder of ldpc_bp.hip:
//
//  * lb_draw_blocks: block s draws RandomState(s).randint(0, 2, K) and then
//    .randn(N) (or .random_sample(N)), restated natively on the host cores
//    (legacy_mt.h), bit for bit the same values, over several threads.  Needs
//    no device.
//  * k_mc_prep: one workgroup per word.  The quasi-cyclic systematic encoder
//    of ldpc.py:790-850 on the word's bits in LDS (systematic syndromes, first
//    parity block, dual-diagonal recursion), then the channel LLRs
//    ch = (2 / sigma^2) ((1 - 2 x) + sigma w) (AWGN) or +-log((1 - p) / p)
//    (BSC) in the host's operation order, no contraction: the same bits as
//    the NumPy expression.
//  * lb::launch (ldpc_bp.hip), unchanged, queued without waiting.
//  * k_mc_count: one workgroup per word, sum((app < 0) != x) over the N bits
//    and the word's iteration count: two ints per word return to the host.
//  * lb_mc_run: the blocks in batches; the next batch's bits and noise go up
//    on a second stream through a second pinned staging buffer while the
//    current batch is encoded, decoded and counted.
//  * lb_mc_run_seeds / lb_draw_blocks_device: the blocks drawn on the device
//    from their seeds (k_mc_draw_blocks, legacy_mt_dev.h: one workgroup per
//    block) on the context's stream, in front of k_mc_prep; only the seeds go
//    up, through no staging buffer and no second stream.
//  * lb_mc_stream_seeds: one operating point as a stream (opt-in, layered
//    decoders).  The blocks in chunks over two lanes (the context's stream and
//    `copy`, each lane with its own bits, noise, code words and channel LLRs):
//    per chunk k_mc_draw_blocks and k_mc_prep over the whole chunk, unchanged,
//    then one persistent kernel (k_bpls / k_bpls32, ldpc_bp.hip) of `slots`
//    workgroups that take the chunk's blocks by ticket, decode them with the
//    layered decoder's arithmetic and count their bit errors themselves, then
//    an asynchronous copy of the chunk's two ints per block and an event.
//    Chunk k + 1's workgroups take the CUs chunk k's last blocks leave.  The
//    host consumes chunk k - 2 in seed order before it queues chunk k (two
//    chunks in flight) and stops queuing once min_errors block errors are
//    reached; the kernel skips blocks that are provably behind the stopping
//    block.  Decoder memory grows with the slots, not with the chunk.
//  * lb_joint_draw: the reps of the joint SPARC + LDPC simulators drawn on the
//    device from their seeds (k_joint_draw: protected bits, unprotected bits,
//    scaled noise, in the reference's order) and their protected bits encoded
//    by k_mc_prep (encode only) behind the unprotected bits of the message.
//    The message bits and the noise stay on the device for libsparc_amp.so
//    (sa_encode_bits); lb_joint_fetch copies them back.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "ldpc_bp_int.h"
#include "legacy_mt.h"
#include "legacy_mt_dev.h"

#pragma clang fp contract(off)

struct lb_mc {
  int Mp = 0, Np = 0, z = 0;  // base matrix shape and lifting size; Mp == 0: no encoder
  int off = 0;                // the single offset column Kp's shifts reduce to
  int* d_proto = nullptr;     // [Mp][Np] shifts mod z, -1: no block
  int cap = 0;                // words the device staging buffers (d_u, d_w, d_x) hold
  int hcap = 0;               // words the pinned staging buffers hold
  uint32_t* d_seeds = nullptr;  // lb_mc_run_seeds: the blocks' seeds [capSeeds]
  int* d_err = nullptr;         // the device generator's error flag
  int capSeeds = 0;
  uint8_t* h_u[2] = {nullptr, nullptr};  // pinned staging, two batches
  double* h_w[2] = {nullptr, nullptr};
  uint8_t* d_u[2] = {nullptr, nullptr};
  double* d_w[2] = {nullptr, nullptr};
  uint8_t* d_x = nullptr;     // [cap][Nv] codeword bits
  int* d_res = nullptr;       // [2][capRes] bit errors, iterations
  int* h_res = nullptr;       // pinned
  int capRes = 0;
  hipStream_t copy = nullptr;
  hipEvent_t ev_up[2] = {nullptr, nullptr};    // staging buffer i has landed on the device
  hipEvent_t ev_prep[2] = {nullptr, nullptr};  // k_mc_prep has read device buffer i
  // lb_mc_stream_seeds: lane 0 on the context's stream, lane 1 on `copy`; lane i draws into
  // d_u[i] / d_w[i] and keeps its own codeword bits, channel LLRs and per-slot decoder slices
  struct Lane {
    uint8_t* x = nullptr;     // [capChunk][Nv]
    double* ch = nullptr;     // [capChunk][Nv]
    double* app = nullptr;    // [capSlots][Nv]
    double* msg = nullptr;    // [capSlots][Nmsg]
    int* it = nullptr;        // [capSlots]
    hipEvent_t done = nullptr;  // the lane's last chunk has landed in h_res
  } lane[2];
  int capChunk = 0, capSlots = 0;
  int* d_ctr = nullptr;       // a call's tickets [nchunks], then its block-error counters [nchunks + 1] (the first
                              // stays 0); room for capCtr chunks
  int capCtr = 0;
  hipEvent_t ev_go = nullptr, ev_join = nullptr;  // the seeds and counters are up; lane 1 is through
  // lb_joint_draw: the reps' protected bits [jrep][K], message bits [jrep][jU + Nv] (unprotected bits, then the
  // codeword) and noise [jrep][jn]; capacities in elements, jrep == 0: nothing drawn
  uint8_t *j_u = nullptr, *j_bits = nullptr;
  double* j_noise = nullptr;
  size_t capJu = 0, capJbits = 0, capJnoise = 0;
  int jrep = 0, jU = 0, jn = 0;
};

namespace {

using lb::fail;

constexpr int kPrepThreads = 256, kCountThreads = 256;
constexpr size_t kPrepLdsBytes = 64 * 1024;

struct PrepArgs {
  const uint8_t* u;  // [B][K] information bits (encoder only)
  const double* w;   // [B][N] randn (kind 0) or random_sample (kind 1) values
  double* ch;        // [B][N]
  uint8_t* x;        // codeword bits, word b at x + b * ldx (ldx = N: [B][N])
  const int* proto;  // [Mp][Np]
  int Mp, Np, z, off, N, K, ldx;
  int kind;          // 0: AWGN, 1: BSC, -1: encode only
  double c0, a;      // AWGN: 2 / sigma^2, sigma; BSC: log((1 - p) / p), p
};

// ldpc.py:790-850 (ldpc.encode_batch) per word; np.roll(v, -s)[i] = v[(i + s) mod z]
__global__ void __launch_bounds__(kPrepThreads) k_mc_prep(PrepArgs a) {
  extern __shared__ uint8_t lds_bits[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int z = a.z, Np = a.Np, Mp = a.Mp, Kp = Np - Mp, N = a.N;
  uint8_t* xs = lds_bits;      // [N] the word
  uint8_t* ps = lds_bits + N;  // [Mp][z] systematic syndromes
  if (Mp > 0) {
    const uint8_t* u = a.u + (size_t)b * a.K;
    for (int i = tid; i < a.K; i += nt) xs[i] = u[i];
    __syncthreads();
    for (int e = tid; e < Mp * z; e += nt) {
      const int j = e / z, i = e % z;
      uint8_t acc = 0;
      for (int k = 0; k < Kp; ++k) {
        const int s = a.proto[j * Np + k];
        if (s >= 0) acc ^= xs[k * z + (i + s) % z];
      }
      ps[e] = acc;
    }
    __syncthreads();
    // first parity block: the XOR of all p_j rolled by the surviving offset
    for (int i = tid; i < z; i += nt) {
      const int src = (i + z - a.off) % z;
      uint8_t acc = 0;
      for (int j = 0; j < Mp; ++j) acc ^= ps[j * z + src];
      xs[Kp * z + i] = acc;
    }
    __syncthreads();
    // dual-diagonal recursion: parity block j + 1 from row j
    for (int j = 0; j < Mp - 1; ++j) {
      for (int i = tid; i < z; i += nt) {
        uint8_t acc = ps[j * z + i];
        for (int k = 0; k <= j; ++k) {
          const int s = a.proto[j * Np + Kp + k];
          if (s >= 0) acc ^= xs[(Kp + k) * z + (i + s) % z];
        }
        xs[(Kp + j + 1) * z + i] = acc;
      }
      __syncthreads();
    }
  }
  uint8_t* xo = a.x + (size_t)b * a.ldx;
  if (a.kind < 0) {
    for (int n = tid; n < N; n += nt) xo[n] = xs[n];
    return;
  }
  const double* w = a.w + (size_t)b * N;
  double* ch = a.ch + (size_t)b * N;
  for (int n = tid; n < N; n += nt) {
    const uint8_t bit = Mp > 0 ? xs[n] : (uint8_t)0;
    xo[n] = bit;
    if (a.kind == 0)
      ch[n] = a.c0 * ((1.0 - 2.0 * (double)bit) + a.a * w[n]);
    else
      ch[n] = w[n] < a.a ? -a.c0 : a.c0;
  }
}

__global__ void __launch_bounds__(kCountThreads) k_mc_count(const double* app, const uint8_t* x, const int* it,
                                                             int N, int* errs, int* iters) {
  __shared__ int part[kCountThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* ap = app + (size_t)b * N;
  const uint8_t* xb = x + (size_t)b * N;
  int cnt = 0;
  for (int n = tid; n < N; n += kCountThreads) cnt += ((ap[n] < 0.0) != (xb[n] != 0)) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int k = 0; k < kCountThreads / 64; ++k) s += part[k];
    errs[b] = s;
    iters[b] = it[b];
  }
}

// the C library's pow / log, as the Python expressions 2.0 / sigma**2 and
// log((1 - p) / p) call them (not folded at compile time)
double (*volatile libm_pow)(double, double) = static_cast<double (*)(double, double)>(::pow);
double (*volatile libm_log)(double) = static_cast<double (*)(double)>(::log);

// Rep-for-rep lb_draw_blocks on the device (legacy_mt_dev.h): block b draws
// RandomState(seeds[b]).randint(0, 2, K) into u[b] (word k & 1), then randn(N)
// (kind 0) or random_sample(N) (kind 1) into w[b].  A block whose randn runs
// into the chunk cap sets *err.
__global__ void __launch_bounds__(legacy_rng_dev::kThreads) k_mc_draw_blocks(const uint32_t* __restrict__ seeds,
                                                                             int K, int N, int kind,
                                                                             uint8_t* __restrict__ u,
                                                                             double* __restrict__ w, int max_chunks,
                                                                             int* err) {
  __shared__ legacy_rng_dev::State st;
  const int b = blockIdx.x;
  legacy_rng_dev::seed_state(st, seeds[b]);
  int have = 0;
  uint8_t* ub = u + (size_t)b * K;
  legacy_rng_dev::draw_masked(st, have, K, 1u, [&](int k, uint32_t v) { ub[k] = (uint8_t)v; });
  double* wb = w + (size_t)b * N;
  if (kind == 0) {
    const bool ok = legacy_rng_dev::draw_randn(st, have, K, N, false, 1.0, wb, max_chunks);
    if (!ok && threadIdx.x == 0) *err = 1;
  } else {
    legacy_rng_dev::draw_samples(st, have, K, N, wb);
  }
}

// A rep of the joint SPARC + LDPC simulators (sparc_ldpc.py:419-446 / :606-634), one workgroup per seed:
// RandomState(seeds[b]).randint(0, 2, K) into u[b] (the protected bits, word k & 1), randint(0, 2, U) into
// bits[b][0 .. U) (the unprotected bits, word (K + j) & 1; bits[b] is ldb bytes, the encoder fills the rest),
// then randn(n) * sigma from word K + U on into noise[b].  A rep whose randn runs into the chunk cap sets *err.
__global__ void __launch_bounds__(legacy_rng_dev::kThreads) k_joint_draw(const uint32_t* __restrict__ seeds, int K,
                                                                         int U, int n, double sigma,
                                                                         uint8_t* __restrict__ u,
                                                                         uint8_t* __restrict__ bits, int ldb,
                                                                         double* __restrict__ noise, int max_chunks,
                                                                         int* err) {
  __shared__ legacy_rng_dev::State st;
  const int b = blockIdx.x;
  legacy_rng_dev::seed_state(st, seeds[b]);
  int have = 0;
  uint8_t* ub = u + (size_t)b * K;
  legacy_rng_dev::draw_masked(st, have, K, 1u, [&](int k, uint32_t v) { ub[k] = (uint8_t)v; });
  uint8_t* mb = bits + (size_t)b * ldb;
  legacy_rng_dev::draw_masked_from(st, have, K, U, 1u, [&](int j, uint32_t v) { mb[j] = (uint8_t)v; });
  const bool ok = legacy_rng_dev::draw_randn(st, have, K + U, n, true, sigma, noise + (size_t)b * n, max_chunks);
  if (!ok && threadIdx.x == 0) *err = 1;
}

void free_pinned(lb_mc* m) {
  for (int i = 0; i < 2; ++i) {
    if (m->h_u[i]) (void)hipHostFree(m->h_u[i]);
    if (m->h_w[i]) (void)hipHostFree(m->h_w[i]);
    m->h_u[i] = nullptr;
    m->h_w[i] = nullptr;
  }
  m->hcap = 0;
}

void free_staging(lb_mc* m) {
  free_pinned(m);
  for (int i = 0; i < 2; ++i) {
    (void)hipFree(m->d_u[i]);
    (void)hipFree(m->d_w[i]);
    m->d_u[i] = nullptr;
    m->d_w[i] = nullptr;
  }
  (void)hipFree(m->d_x);
  m->d_x = nullptr;
  m->cap = 0;
}

int ensure_state(lb_ctx* c) {
  if (c->mc) return LB_OK;
  lb_mc* m = new lb_mc;
  c->mc = m;  // released with the context whatever fails below
  if (hipStreamCreateWithFlags(&m->copy, hipStreamNonBlocking) != hipSuccess) {
    m->copy = nullptr;
    return fail(LB_ERR_HIP, "stream creation failed");
  }
  for (hipEvent_t* e : {&m->ev_up[0], &m->ev_up[1], &m->ev_prep[0], &m->ev_prep[1]})
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
      *e = nullptr;
      return fail(LB_ERR_HIP, "hipEventCreate failed");
    }
  return LB_OK;
}

// staging for `B` words: two pinned and two device buffers of bits and noise, the codeword bits
int ensure_staging(lb_ctx* c, int B, bool pinned = true) {
  lb_mc* m = c->mc;
  const size_t K = (size_t)(c->Nv - c->Nc), N = (size_t)c->Nv;
  int rc;
  if (B > m->cap) {
    free_staging(m);
    for (int i = 0; i < 2; ++i) {
      if (K > 0 && (rc = lb::dev_alloc((void**)&m->d_u[i], B * K))) return rc;
      if ((rc = lb::dev_alloc((void**)&m->d_w[i], B * N * sizeof(double)))) return rc;
    }
    if ((rc = lb::dev_alloc((void**)&m->d_x, B * N))) return rc;
    m->cap = B;
  }
  if (pinned && B > m->hcap) {  // (the device-draw path stages nothing through the host)
    free_pinned(m);
    for (int i = 0; i < 2; ++i) {
      if (K > 0 && hipHostMalloc((void**)&m->h_u[i], B * K, hipHostMallocDefault) != hipSuccess) {
        m->h_u[i] = nullptr;
        return fail(LB_ERR_NOMEM, "hipHostMalloc failed");
      }
      if (hipHostMalloc((void**)&m->h_w[i], B * N * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        m->h_w[i] = nullptr;
        return fail(LB_ERR_NOMEM, "hipHostMalloc failed");
      }
    }
    m->hcap = B;
  }
  return LB_OK;
}

// the seeds of lb_mc_run_seeds and the generator's error flag
int ensure_seeds(lb_mc* m, int nblk) {
  int rc;
  if (!m->d_err && (rc = lb::dev_alloc((void**)&m->d_err, sizeof(int)))) return rc;
  if (nblk <= m->capSeeds) return LB_OK;
  (void)hipFree(m->d_seeds);
  m->d_seeds = nullptr;
  m->capSeeds = 0;
  if ((rc = lb::dev_alloc((void**)&m->d_seeds, (size_t)nblk * sizeof(uint32_t)))) return rc;
  m->capSeeds = nblk;
  return LB_OK;
}

void free_joint(lb_mc* m) {
  (void)hipFree(m->j_u);
  (void)hipFree(m->j_bits);
  (void)hipFree(m->j_noise);
  m->j_u = m->j_bits = nullptr;
  m->j_noise = nullptr;
  m->capJu = m->capJbits = m->capJnoise = 0;
  m->jrep = 0;
}

// lb_joint_draw's buffers for nrep reps of U unprotected bits and n noise values; each grows on its own
int ensure_joint(lb_ctx* c, int nrep, int U, int n) {
  lb_mc* m = c->mc;
  const size_t nu = (size_t)nrep * (c->Nv - c->Nc), nb = (size_t)nrep * ((size_t)U + c->Nv), nn = (size_t)nrep * n;
  int rc;
  m->jrep = 0;  // until the draw has succeeded
  if (nu > m->capJu) {
    (void)hipFree(m->j_u);
    m->j_u = nullptr;
    m->capJu = 0;
    if ((rc = lb::dev_alloc((void**)&m->j_u, nu))) return rc;
    m->capJu = nu;
  }
  if (nb > m->capJbits) {
    (void)hipFree(m->j_bits);
    m->j_bits = nullptr;
    m->capJbits = 0;
    if ((rc = lb::dev_alloc((void**)&m->j_bits, nb))) return rc;
    m->capJbits = nb;
  }
  if (nn > m->capJnoise) {
    (void)hipFree(m->j_noise);
    m->j_noise = nullptr;
    m->capJnoise = 0;
    if ((rc = lb::dev_alloc((void**)&m->j_noise, nn * sizeof(double)))) return rc;
    m->capJnoise = nn;
  }
  return LB_OK;
}

int ensure_results(lb_mc* m, int nblk) {
  if (nblk <= m->capRes) return LB_OK;
  (void)hipFree(m->d_res);
  if (m->h_res) (void)hipHostFree(m->h_res);
  m->d_res = m->h_res = nullptr;
  m->capRes = 0;
  int rc;
  if ((rc = lb::dev_alloc((void**)&m->d_res, (size_t)2 * nblk * sizeof(int)))) return rc;
  if (hipHostMalloc((void**)&m->h_res, (size_t)2 * nblk * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    m->h_res = nullptr;
    return fail(LB_ERR_NOMEM, "hipHostMalloc failed");
  }
  m->capRes = nblk;
  return LB_OK;
}

void free_stream(lb_mc* m) {
  for (lb_mc::Lane& l : m->lane) {
    (void)hipFree(l.x);
    (void)hipFree(l.ch);
    (void)hipFree(l.app);
    (void)hipFree(l.msg);
    (void)hipFree(l.it);
    l.x = nullptr;
    l.ch = l.app = l.msg = nullptr;
    l.it = nullptr;
  }
  m->capChunk = m->capSlots = 0;
}

// the lanes of lb_mc_stream_seeds for chunks of `chunk` blocks in `slots` slots, `nchunks` counters
int ensure_stream(lb_ctx* c, int chunk, int slots, int nchunks, bool msg) {
  lb_mc* m = c->mc;
  const size_t N = (size_t)c->Nv;
  int rc;
  for (hipEvent_t* e : {&m->lane[0].done, &m->lane[1].done, &m->ev_go, &m->ev_join})
    if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
      *e = nullptr;
      return fail(LB_ERR_HIP, "hipEventCreate failed");
    }
  msg = msg || m->lane[0].msg;
  if (chunk > m->capChunk || slots > m->capSlots || (msg && !m->lane[0].msg)) {
    chunk = std::max(chunk, m->capChunk);
    slots = std::max(slots, m->capSlots);
    free_stream(m);
    for (lb_mc::Lane& l : m->lane) {
      if ((rc = lb::dev_alloc((void**)&l.x, chunk * N))) return rc;
      if ((rc = lb::dev_alloc((void**)&l.ch, chunk * N * sizeof(double)))) return rc;
      if ((rc = lb::dev_alloc((void**)&l.app, slots * N * sizeof(double)))) return rc;
      if (msg && (rc = lb::dev_alloc((void**)&l.msg, (size_t)slots * c->Nmsg * sizeof(double)))) return rc;
      if ((rc = lb::dev_alloc((void**)&l.it, (size_t)slots * sizeof(int)))) return rc;
    }
    m->capChunk = chunk;
    m->capSlots = slots;
  }
  if (nchunks > m->capCtr) {
    (void)hipFree(m->d_ctr);
    m->d_ctr = nullptr;
    m->capCtr = 0;
    if ((rc = lb::dev_alloc((void**)&m->d_ctr, ((size_t)2 * nchunks + 1) * sizeof(int)))) return rc;
    m->capCtr = nchunks;
  }
  return LB_OK;
}

// what ldpc.encode_batch checks (ldpc.py:815-822): the shifts of column Kp,
// counted mod 2 by their value mod z, leave exactly one offset
int surviving_offset(const int* proto, int Mp, int Np, int z, int* off) {
  const int Kp = Np - Mp;
  std::vector<int> par(z, 0);
  for (int j = 0; j < Mp; ++j) {
    const int s = proto[j * Np + Kp];
    if (s >= 0) par[s % z] ^= 1;
  }
  int n = 0;
  for (int i = 0; i < z; ++i)
    if (par[i]) {
      *off = i;
      ++n;
    }
  return n == 1 ? LB_OK : LB_ERR_ARG;
}

void fill_prep(PrepArgs& p, const lb_ctx* c, bool enc) {
  const lb_mc* m = c->mc;
  p.proto = m->d_proto;
  p.Mp = enc ? m->Mp : 0;
  p.Np = enc ? m->Np : 0;
  p.z = enc ? m->z : 1;
  p.off = m->off;
  p.N = c->Nv;
  p.K = c->Nv - c->Nc;
  p.ldx = c->Nv;
}

size_t prep_lds(const PrepArgs& p) { return p.Mp > 0 ? (size_t)(p.Np + p.Mp) * p.z : 0; }

}  // namespace

namespace lb {

void mc_release(lb_ctx* c) {
  lb_mc* m = c->mc;
  if (!m) return;
  (void)hipSetDevice(c->dev);
  free_staging(m);
  free_stream(m);
  free_joint(m);
  (void)hipFree(m->d_ctr);
  for (hipEvent_t e : {m->lane[0].done, m->lane[1].done, m->ev_go, m->ev_join})
    if (e) (void)hipEventDestroy(e);
  (void)hipFree(m->d_proto);
  (void)hipFree(m->d_res);
  (void)hipFree(m->d_seeds);
  (void)hipFree(m->d_err);
  if (m->h_res) (void)hipHostFree(m->h_res);
  for (hipEvent_t e : {m->ev_up[0], m->ev_up[1], m->ev_prep[0], m->ev_prep[1]})
    if (e) (void)hipEventDestroy(e);
  if (m->copy) (void)hipStreamDestroy(m->copy);
  delete m;
  c->mc = nullptr;
}

}  // namespace lb

extern "C" {

int lb_draw_blocks(const uint32_t* seeds, int nblk, int K, int N, int kind, uint8_t* u, double* w, int threads) {
  if (nblk < 0 || K < 0 || N < 0 || (kind != 0 && kind != 1) ||
      (nblk > 0 && (!seeds || (K > 0 && !u) || (N > 0 && !w))))
    return fail(LB_ERR_ARG, "lb_draw_blocks: bad arguments");
  int nt = threads > 0 ? threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  nt = std::max(1, std::min(nt, std::max(1, nblk)));
  auto work = [&](int t0) {
    for (int i = t0; i < nblk; i += nt) {
      legacy_rng::LegacyMT mt(seeds[i]);
      uint8_t* ub = u + (size_t)i * K;
      for (int k = 0; k < K; ++k) ub[k] = (uint8_t)mt.bounded(1u);  // randint(0, 2, K)
      double* wb = w + (size_t)i * N;
      if (kind == 0)
        for (int n = 0; n < N; ++n) wb[n] = mt.gaussian();  // randn(N)
      else
        for (int n = 0; n < N; ++n) wb[n] = mt.next_double();  // random_sample(N)
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  return LB_OK;
}

int lb_mc_set_code(lb_ctx* c, const int* proto, int Mp, int Np, int z) {
  int off = 0;
  if (Mp < 0) return fail(LB_ERR_ARG, "lb_mc_set_code: Mp < 0");
  if (Mp > 0) {
    if (!proto || Np <= Mp || z < 1) return fail(LB_ERR_ARG, "lb_mc_set_code: bad base matrix shape");
    for (int i = 0; i < Mp * Np; ++i)
      if (proto[i] < -1) return fail(LB_ERR_ARG, "lb_mc_set_code: shift below -1");
    if (surviving_offset(proto, Mp, Np, z, &off))
      return fail(LB_ERR_ARG, "lb_mc_set_code: the offsets in column Kp do not add to a single offset");
  }
  if (!c) return fail(LB_ERR_ARG, "lb_mc_set_code: null context");
  if (Mp > 0) {
    if ((long long)Np * z != c->Nv || (long long)Mp * z != c->Nc)
      return fail(LB_ERR_ARG, "lb_mc_set_code: base matrix does not match the context's graph");
    if ((size_t)(Np + Mp) * z > kPrepLdsBytes)
      return fail(LB_ERR_UNSUPPORTED, "lb_mc_set_code: the word does not fit in LDS");
  }
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = ensure_state(c))) return rc;
  lb_mc* m = c->mc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // no encode in flight reads the old table
  (void)hipFree(m->d_proto);
  m->d_proto = nullptr;
  m->Mp = 0;
  if (Mp == 0) return LB_OK;
  std::vector<int> red((size_t)Mp * Np);
  for (int i = 0; i < Mp * Np; ++i) red[i] = proto[i] < 0 ? -1 : proto[i] % z;
  if ((rc = lb::dev_alloc((void**)&m->d_proto, red.size() * sizeof(int)))) return rc;
  HIP_TRY(hipMemcpyAsync(m->d_proto, red.data(), red.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  m->Mp = Mp;
  m->Np = Np;
  m->z = z;
  m->off = off;
  return LB_OK;
}

int lb_encode(lb_ctx* c, int B, const uint8_t* u, uint8_t* x) {
  if (!c) return fail(LB_ERR_ARG, "lb_encode: null context");
  if (B < 0 || (B > 0 && (!u || !x))) return fail(LB_ERR_ARG, "lb_encode: bad arguments");
  if (!c->mc || c->mc->Mp == 0) return fail(LB_ERR_ARG, "lb_encode: no encoder set (lb_mc_set_code)");
  if (B == 0) return LB_OK;
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = ensure_staging(c, B))) return rc;
  lb_mc* m = c->mc;
  const size_t K = (size_t)(c->Nv - c->Nc), N = (size_t)c->Nv;
  std::memcpy(m->h_u[0], u, B * K);
  HIP_TRY(hipMemcpyAsync(m->d_u[0], m->h_u[0], B * K, hipMemcpyHostToDevice, c->stream));
  PrepArgs p{};
  fill_prep(p, c, true);
  p.u = m->d_u[0];
  p.x = m->d_x;
  p.kind = -1;
  hipLaunchKernelGGL(k_mc_prep, dim3(B), dim3(kPrepThreads), prep_lds(p), c->stream, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(x, m->d_x, B * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

int lb_mc_run(lb_ctx* c, int nblk, const uint8_t* u, const double* w, double a, int kind, int batch, int algo,
              double corr, int max_iter, int* errs, int* iters) {
  if (!c) return fail(LB_ERR_ARG, "lb_mc_run: null context");
  if (nblk < 0 || batch <= 0 || (kind != 0 && kind != 1) || (nblk > 0 && (!w || !errs || !iters)))
    return fail(LB_ERR_ARG, "lb_mc_run: bad arguments");
  if (kind == 0 ? !(a > 0.0) : !(a > 0.0 && a < 1.0))
    return fail(LB_ERR_ARG, "lb_mc_run: sigma must be > 0, p in (0, 1)");
  const bool enc = u != nullptr;
  if (enc && kind == 1) return fail(LB_ERR_ARG, "lb_mc_run: the BSC sends the all-zero word (u must be null)");
  if (enc && (!c->mc || c->mc->Mp == 0)) return fail(LB_ERR_ARG, "lb_mc_run: no encoder set (lb_mc_set_code)");
  if (nblk == 0) return LB_OK;
  lb::DecType t;
  int rc;
  if ((rc = lb::resolve(c, algo, corr, max_iter, false, &t))) return rc;
  batch = std::min(batch, nblk);
  HIP_TRY(hipSetDevice(c->dev));
  if ((rc = ensure_state(c))) return rc;
  if ((rc = lb::ensure_io(c, batch))) return rc;
  if ((rc = ensure_staging(c, batch))) return rc;
  lb_mc* m = c->mc;
  if ((rc = ensure_results(m, nblk))) return rc;
  const size_t K = (size_t)(c->Nv - c->Nc), N = (size_t)c->Nv;
  PrepArgs p{};
  fill_prep(p, c, enc);
  p.ch = c->d_ch;
  p.x = m->d_x;
  p.kind = kind;
  p.a = a;
  p.c0 = kind == 0 ? 2.0 / libm_pow(a, 2.0) : libm_log((1.0 - a) / a);
  const int nb = (nblk + batch - 1) / batch;
  // batch j into staging buffer j & 1: the host waits only for that buffer's
  // previous upload (batch j - 2); the upload itself waits for the prep
  // kernel that read the device buffer
  auto stage = [&](int j) -> int {
    const int i = j & 1;
    const size_t b0 = (size_t)j * batch, B = std::min<size_t>(batch, nblk - b0);
    if (j >= 2) HIP_TRY(hipEventSynchronize(m->ev_up[i]));
    if (enc) std::memcpy(m->h_u[i], u + b0 * K, B * K);
    std::memcpy(m->h_w[i], w + b0 * N, B * N * sizeof(double));
    if (j >= 2) HIP_TRY(hipStreamWaitEvent(m->copy, m->ev_prep[i], 0));
    if (enc) HIP_TRY(hipMemcpyAsync(m->d_u[i], m->h_u[i], B * K, hipMemcpyHostToDevice, m->copy));
    HIP_TRY(hipMemcpyAsync(m->d_w[i], m->h_w[i], B * N * sizeof(double), hipMemcpyHostToDevice, m->copy));
    HIP_TRY(hipEventRecord(m->ev_up[i], m->copy));
    return LB_OK;
  };
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  if ((rc = stage(0))) return rc;
  for (int k = 0; k < nb; ++k) {
    const int i = k & 1;
    const int b0 = k * batch, B = std::min(batch, nblk - b0);
    HIP_TRY(hipStreamWaitEvent(c->stream, m->ev_up[i], 0));
    p.u = m->d_u[i];
    p.w = m->d_w[i];
    hipLaunchKernelGGL(k_mc_prep, dim3(B), dim3(kPrepThreads), prep_lds(p), c->stream, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev_prep[i], c->stream));
    if ((rc = lb::launch(c, B, c->d_ch, c->d_app, c->d_it, t, corr, max_iter, false))) return rc;
    hipLaunchKernelGGL(k_mc_count, dim3(B), dim3(kCountThreads), 0, c->stream, c->d_app, m->d_x, c->d_it, (int)N,
                       m->d_res + b0, m->d_res + nblk + b0);
    HIP_TRY(hipGetLastError());
    if (k + 1 < nb && (rc = stage(k + 1))) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipMemcpyAsync(m->h_res, m->d_res, (size_t)2 * nblk * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(errs, m->h_res, (size_t)nblk * sizeof(int));
  std::memcpy(iters, m->h_res + nblk, (size_t)nblk * sizeof(int));
  return LB_OK;
}

// the argument checks of the seeded entries (`who`), in their order; per: the batch or the chunk,
// ptrs: the entry's own pointers are there
static int check_seeded(const std::string& who, lb_ctx* c, int nblk, const uint32_t* seeds, int K, double a, int kind,
                        int per, const int* errs, const int* iters, bool ptrs = true) {
  if (!c) return fail(LB_ERR_ARG, who + ": null context");
  if (nblk < 0 || per <= 0 || (kind != 0 && kind != 1) || !ptrs || (nblk > 0 && (!seeds || !errs || !iters)))
    return fail(LB_ERR_ARG, who + ": bad arguments");
  if (kind == 0 ? !(a > 0.0) : !(a > 0.0 && a < 1.0)) return fail(LB_ERR_ARG, who + ": sigma must be > 0, p in (0, 1)");
  if (K != 0 && K != c->Nv - c->Nc) return fail(LB_ERR_ARG, who + ": K must be Nv - Nc, or 0 for no bits");
  if (K > 0 && kind == 1) return fail(LB_ERR_ARG, who + ": the BSC sends the all-zero word (K must be 0)");
  if (K > 0 && (!c->mc || c->mc->Mp == 0)) return fail(LB_ERR_ARG, who + ": no encoder set (lb_mc_set_code)");
  return LB_OK;
}

int lb_mc_run_seeds(lb_ctx* c, int nblk, const uint32_t* seeds, int K, double a, int kind, int batch, int algo,
                    double corr, int max_iter, int* errs, int* iters) {
  int rc;
  if ((rc = check_seeded("lb_mc_run_seeds", c, nblk, seeds, K, a, kind, batch, errs, iters))) return rc;
  const bool enc = K > 0;
  if (nblk == 0) return LB_OK;
  lb::DecType t;
  if ((rc = lb::resolve(c, algo, corr, max_iter, false, &t))) return rc;
  batch = std::min(batch, nblk);
  HIP_TRY(hipSetDevice(c->dev));
  if ((rc = ensure_state(c))) return rc;
  if ((rc = lb::ensure_io(c, batch))) return rc;
  if ((rc = ensure_staging(c, batch, false))) return rc;
  lb_mc* m = c->mc;
  if ((rc = ensure_results(m, nblk))) return rc;
  if ((rc = ensure_seeds(m, nblk))) return rc;
  const int N = c->Nv;
  PrepArgs p{};
  fill_prep(p, c, enc);
  p.ch = c->d_ch;
  p.x = m->d_x;
  p.kind = kind;
  p.a = a;
  p.c0 = kind == 0 ? 2.0 / libm_pow(a, 2.0) : libm_log((1.0 - a) / a);
  p.u = m->d_u[0];
  p.w = m->d_w[0];
  const int cap = legacy_rng_dev::randn_chunk_cap(N);
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  HIP_TRY(hipMemcpyAsync(m->d_seeds, seeds, (size_t)nblk * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(m->d_err, 0, sizeof(int), c->stream));
  // one stream: a batch's draw follows the prep kernel that read the last one's
  for (int b0 = 0; b0 < nblk; b0 += batch) {
    const int B = std::min(batch, nblk - b0);
    hipLaunchKernelGGL(k_mc_draw_blocks, dim3(B), dim3(legacy_rng_dev::kThreads), 0, c->stream, m->d_seeds + b0, K,
                       N, kind, m->d_u[0], m->d_w[0], cap, m->d_err);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mc_prep, dim3(B), dim3(kPrepThreads), prep_lds(p), c->stream, p);
    HIP_TRY(hipGetLastError());
    if ((rc = lb::launch(c, B, c->d_ch, c->d_app, c->d_it, t, corr, max_iter, false))) return rc;
    hipLaunchKernelGGL(k_mc_count, dim3(B), dim3(kCountThreads), 0, c->stream, c->d_app, m->d_x, c->d_it, N,
                       m->d_res + b0, m->d_res + nblk + b0);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int err = 0;
  HIP_TRY(hipMemcpyAsync(&err, m->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(m->h_res, m->d_res, (size_t)2 * nblk * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (err) return fail(LB_ERR_HIP, "lb_mc_run_seeds: a block's randn ran into the chunk cap");
  std::memcpy(errs, m->h_res, (size_t)nblk * sizeof(int));
  std::memcpy(iters, m->h_res + nblk, (size_t)nblk * sizeof(int));
  return LB_OK;
}

int lb_mc_stream_seeds(lb_ctx* c, int nblk, const uint32_t* seeds, int K, double a, int kind, int chunk, int slots,
                       int min_errors, int algo, double corr, int max_iter, int* errs, int* iters, long long* out) {
  int rc, resident = 1;
  if ((rc = check_seeded("lb_mc_stream_seeds", c, nblk, seeds, K, a, kind, chunk, errs, iters, out != nullptr)))
    return rc;
  const bool enc = K > 0;
  lb::DecType t;
  if ((rc = lb::resolve(c, algo, corr, max_iter, true, &t))) return rc;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (nblk == 0) return LB_OK;
  if ((rc = lb::stream_plan(c, t, &resident))) return rc;
  chunk = std::min(chunk, nblk);
  // a slot beyond the chunk's blocks would find no ticket
  slots = std::min(slots > 0 ? slots : resident * c->ncu, chunk);
  const int nchunks = (nblk + chunk - 1) / chunk;
  if ((rc = ensure_state(c))) return rc;
  if ((rc = ensure_staging(c, chunk, false))) return rc;
  if ((rc = ensure_stream(c, chunk, slots, nchunks, t.hbm))) return rc;
  lb_mc* m = c->mc;
  if ((rc = ensure_results(m, nblk))) return rc;
  if ((rc = ensure_seeds(m, nblk))) return rc;
  const int N = c->Nv;
  PrepArgs p{};
  fill_prep(p, c, enc);
  p.kind = kind;
  p.a = a;
  p.c0 = kind == 0 ? 2.0 / libm_pow(a, 2.0) : libm_log((1.0 - a) / a);
  const int cap = legacy_rng_dev::randn_chunk_cap(N);
  hipStream_t st[2] = {c->stream, m->copy};
  int* ticket = m->d_ctr;           // [nchunks]
  int* ecnt = m->d_ctr + nchunks;   // [nchunks + 1]: chunk k counts in ecnt[k + 1]
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  HIP_TRY(hipMemcpyAsync(m->d_seeds, seeds, (size_t)nblk * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(m->d_err, 0, sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(m->d_ctr, 0, ((size_t)2 * nchunks + 1) * sizeof(int), c->stream));
  HIP_TRY(hipEventRecord(m->ev_go, c->stream));
  HIP_TRY(hipStreamWaitEvent(m->copy, m->ev_go, 0));
  // the sequential rule of harness.ber_point over the blocks that have landed
  int used = 0, nerr = 0, decoded = 0, queued = 0, consumed = 0;
  bool met = false;
  auto consume = [&]() -> int {  // the oldest chunk in flight
    const int k = consumed++;
    HIP_TRY(hipEventSynchronize(m->lane[k & 1].done));
    const int b0 = k * chunk, B = std::min(chunk, nblk - b0);
    for (int j = b0; j < b0 + B; ++j) {
      if (m->h_res[nblk + j] >= 0) ++decoded;
      if (met) continue;
      ++used;
      if (m->h_res[j] > 0) ++nerr;
      met = min_errors > 0 && nerr >= min_errors;
    }
    return LB_OK;
  };
  for (int k = 0; k < nchunks; ++k) {
    if (k >= 2 && (rc = consume())) return rc;  // chunk k - 2: at most two in flight
    if (met) break;
    const int i = k & 1;
    const int b0 = k * chunk, B = std::min(chunk, nblk - b0);
    lb_mc::Lane& l = m->lane[i];
    hipLaunchKernelGGL(k_mc_draw_blocks, dim3(B), dim3(legacy_rng_dev::kThreads), 0, st[i], m->d_seeds + b0, K, N,
                       kind, m->d_u[i], m->d_w[i], cap, m->d_err);
    HIP_TRY(hipGetLastError());
    p.u = m->d_u[i];
    p.w = m->d_w[i];
    p.ch = l.ch;
    p.x = l.x;
    hipLaunchKernelGGL(k_mc_prep, dim3(B), dim3(kPrepThreads), prep_lds(p), st[i], p);
    HIP_TRY(hipGetLastError());
    lb::StreamChunk s;
    s.ch = l.ch;
    s.x = l.x;
    s.app = l.app;
    s.msg = l.msg;
    s.slot_iters = l.it;
    s.errs = m->d_res + b0;
    s.iters = m->d_res + nblk + b0;
    s.ticket = ticket + k;
    s.eprev = ecnt + k;
    s.ecur = ecnt + k + 1;
    s.chunk = B;
    s.base = nerr;  // the block errors of chunks <= k - 2, all consumed above
    s.min_errors = min_errors;
    if ((rc = lb::launch_stream(c, st[i], std::min(slots, B), s, t, corr, max_iter))) return rc;
    HIP_TRY(hipMemcpyAsync(m->h_res + b0, m->d_res + b0, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st[i]));
    HIP_TRY(hipMemcpyAsync(m->h_res + nblk + b0, m->d_res + nblk + b0, (size_t)B * sizeof(int), hipMemcpyDeviceToHost,
                           st[i]));
    HIP_TRY(hipEventRecord(l.done, st[i]));
    ++queued;
  }
  // lane 1 joins the context's stream: the run's time covers both lanes
  HIP_TRY(hipEventRecord(m->ev_join, m->copy));
  HIP_TRY(hipStreamWaitEvent(c->stream, m->ev_join, 0));
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int err = 0;
  HIP_TRY(hipMemcpyAsync(&err, m->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (err) return fail(LB_ERR_HIP, "lb_mc_stream_seeds: a block's randn ran into the chunk cap");
  // the chunks in flight when the loop ended (at most two), in seed order
  while (consumed < queued)
    if ((rc = consume())) return rc;
  const int nq = (int)std::min<long long>(nblk, (long long)queued * chunk);
  std::memcpy(errs, m->h_res, (size_t)nq * sizeof(int));
  std::memcpy(iters, m->h_res + nblk, (size_t)nq * sizeof(int));
  for (int j = nq; j < nblk; ++j) {  // never queued
    errs[j] = 0;
    iters[j] = -1;
  }
  out[0] = used;
  out[1] = decoded;
  out[2] = slots;
  out[3] = queued;
  return LB_OK;
}

int lb_draw_blocks_device(lb_ctx* c, const uint32_t* seeds, int nblk, int K, int N, int kind, uint8_t* u, double* w) {
  if (!c) return fail(LB_ERR_ARG, "lb_draw_blocks_device: null context");
  if (nblk < 0 || K < 0 || N < 0 || K > (1 << 27) || N > (1 << 27) || (kind != 0 && kind != 1) ||
      (nblk > 0 && (!seeds || (K > 0 && !u) || (N > 0 && !w))))
    return fail(LB_ERR_ARG, "lb_draw_blocks_device: bad arguments");
  if (nblk == 0 || (K == 0 && N == 0)) return LB_OK;
  HIP_TRY(hipSetDevice(c->dev));
  struct Bufs {  // this call's own arrays, whatever N and K
    uint32_t* seeds = nullptr;
    uint8_t* u = nullptr;
    double* w = nullptr;
    int* err = nullptr;
    ~Bufs() {
      (void)hipFree(seeds);
      (void)hipFree(u);
      (void)hipFree(w);
      (void)hipFree(err);
    }
  } d;
  int rc;
  if ((rc = lb::dev_alloc((void**)&d.seeds, (size_t)nblk * sizeof(uint32_t)))) return rc;
  if (K > 0 && (rc = lb::dev_alloc((void**)&d.u, (size_t)nblk * K))) return rc;
  if (N > 0 && (rc = lb::dev_alloc((void**)&d.w, (size_t)nblk * N * sizeof(double)))) return rc;
  if ((rc = lb::dev_alloc((void**)&d.err, sizeof(int)))) return rc;
  HIP_TRY(hipMemcpyAsync(d.seeds, seeds, (size_t)nblk * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(d.err, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_mc_draw_blocks, dim3(nblk), dim3(legacy_rng_dev::kThreads), 0, c->stream, d.seeds, K, N, kind,
                     d.u, d.w, legacy_rng_dev::randn_chunk_cap(N), d.err);
  HIP_TRY(hipGetLastError());
  int err = 0;
  HIP_TRY(hipMemcpyAsync(&err, d.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (K > 0) HIP_TRY(hipMemcpyAsync(u, d.u, (size_t)nblk * K, hipMemcpyDeviceToHost, c->stream));
  if (N > 0) HIP_TRY(hipMemcpyAsync(w, d.w, (size_t)nblk * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (err) return fail(LB_ERR_HIP, "lb_draw_blocks_device: a block's randn ran into the chunk cap");
  return LB_OK;
}

int lb_joint_draw(lb_ctx* c, int nrep, const uint32_t* seeds, int K, int U, int n, double sigma, uint8_t** d_bits,
                  double** d_noise, double* ms_out) {
  if (!c) return fail(LB_ERR_ARG, "lb_joint_draw: null context");
  if (nrep <= 0 || !seeds || !d_bits || !d_noise) return fail(LB_ERR_ARG, "lb_joint_draw: bad arguments");
  if (U < 0 || n <= 0 || U > (1 << 27) || n > (1 << 27))
    return fail(LB_ERR_ARG, "lb_joint_draw: U must be in [0, 2^27], n in [1, 2^27]");
  if (!std::isfinite(sigma)) return fail(LB_ERR_ARG, "lb_joint_draw: sigma must be finite");
  if (!c->mc || c->mc->Mp == 0) return fail(LB_ERR_ARG, "lb_joint_draw: no encoder set (lb_mc_set_code)");
  if (K != c->Nv - c->Nc) return fail(LB_ERR_ARG, "lb_joint_draw: K must be Nv - Nc");
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  lb_mc* m = c->mc;
  if ((rc = ensure_joint(c, nrep, U, n))) return rc;
  if ((rc = ensure_seeds(m, nrep))) return rc;
  const int N = c->Nv, ldb = U + N;
  PrepArgs p{};
  fill_prep(p, c, true);
  p.u = m->j_u;
  p.x = m->j_bits + U;  // the codeword behind the rep's unprotected bits
  p.ldx = ldb;
  p.kind = -1;
  HIP_TRY(hipMemcpyAsync(m->d_seeds, seeds, (size_t)nrep * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(m->d_err, 0, sizeof(int), c->stream));
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  hipLaunchKernelGGL(k_joint_draw, dim3(nrep), dim3(legacy_rng_dev::kThreads), 0, c->stream, m->d_seeds, K, U, n,
                     sigma, m->j_u, m->j_bits, ldb, m->j_noise, legacy_rng_dev::randn_chunk_cap(n), m->d_err);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_mc_prep, dim3(nrep), dim3(kPrepThreads), prep_lds(p), c->stream, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int err = 0;
  HIP_TRY(hipMemcpyAsync(&err, m->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (err) return fail(LB_ERR_HIP, "lb_joint_draw: a rep's randn ran into the chunk cap");
  if (ms_out) {
    float ms = -1.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *ms_out = ms;
  }
  m->jrep = nrep;
  m->jU = U;
  m->jn = n;
  *d_bits = m->j_bits;
  *d_noise = m->j_noise;
  return LB_OK;
}

int lb_joint_fetch(lb_ctx* c, int nrep, uint8_t* bits_out, double* noise_out) {
  if (!c) return fail(LB_ERR_ARG, "lb_joint_fetch: null context");
  if (nrep <= 0 || !c->mc || nrep > c->mc->jrep)
    return fail(LB_ERR_ARG, "lb_joint_fetch: nrep outside the drawn reps (lb_joint_draw)");
  HIP_TRY(hipSetDevice(c->dev));
  const lb_mc* m = c->mc;
  if (bits_out)
    HIP_TRY(hipMemcpyAsync(bits_out, m->j_bits, (size_t)nrep * ((size_t)m->jU + c->Nv), hipMemcpyDeviceToHost,
                           c->stream));
  if (noise_out)
    HIP_TRY(hipMemcpyAsync(noise_out, m->j_noise, (size_t)nrep * m->jn * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LB_OK;
}

}  // extern "C"
