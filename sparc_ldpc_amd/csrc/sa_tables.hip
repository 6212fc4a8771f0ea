// sa_tables.hip — the operator tables of a context (sa_tables.h: Tables):
// the builders of sa_tables.h run over the sections on the host's cores, the
// uploads, the batched kernel's tables at their first use (ensure_invb).

#include "sa_host.h"

namespace sa {

void tables_free(Tables& t) {
  void* all[] = {t.inv, t.inv32, t.invb, t.invl, t.hs, t.fwd, t.fwdb, t.fwd2, t.fwd3, t.invp, t.fwd2p};
  for (void* p : all) dev_free(p);
  t = Tables();
}

// Host vector -> a new device buffer, on the context's (non-blocking) stream;
// the caller waits for the stream before the vector goes: a pageable
// hipMemcpy may return once the data is staged, before the DMA lands, and
// the null stream does not order the kernels of a non-blocking stream.
template <typename T>
static int table_upload(sa_ctx* c, T** dst, const std::vector<T>& src) {
  if (int rc = dev_alloc(c, (void**)dst, src.size() * sizeof(T))) return rc;
  HIP_TRY(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->at().stream));
  return SA_OK;
}

// The bucket table inv [L][w] of the context's ordering (T: inv_row), every
// section validated: the first bad entry of the first bad section is reported
template <typename T>
static int fill_inv(const sa_ctx* c, std::vector<T>& inv) {
  const int L = c->L, n = c->n, w = c->w;
  inv.assign((size_t)L * w, (T)n);
  std::vector<std::string> bad((size_t)L);
  parallel_for(L, 1, [&](int l) {
    inv_row(c->ordering.data() + (size_t)l * n, l, n, w, inv.data() + (size_t)l * w, bad[l]);
  });
  for (int l = 0; l < L; ++l)
    if (!bad[l].empty()) return fail(SA_ERR_ORDERING, bad[l]);
  return SA_OK;
}

// The Ab table fwd [G][n][4] (missing sections -> (k 0, +)) and, where asked
// for, the pair / triple tables; sections in blocks of 12 over the host's
// cores (a pair / triple word is filled by one block)
static void fill_fwd(const sa_ctx* c, std::vector<uint16_t>& fwd, std::vector<uint32_t>* fwd2,
                     std::vector<uint32_t>* fwd3) {
  const int L = c->L, n = c->n;
  fwd.assign((size_t)fwd_groups(L) * n * kSpw, 0);
  if (fwd2) fwd2->assign((size_t)((L + 1) / 2) * n, 0);
  if (fwd3) fwd3->assign((size_t)c->G3 * n, 0);
  parallel_for(L, 12, [&](int l) {
    fwd_section(c->ordering.data() + (size_t)l * n, l, n, c->M, fwd.data(), fwd2 ? fwd2->data() : nullptr,
                fwd3 ? fwd3->data() : nullptr);
  });
}

// The host copies of inv and fwd (16-bit operators): kept by build_tables
// until the batched tables are built from them, rebuilt where they went
static const std::vector<uint16_t>& host_inv(sa_ctx* c) {
  if (c->h_inv.size() != (size_t)c->L * c->w) (void)fill_inv(c, c->h_inv);  // (validated when the context was created)
  return c->h_inv;
}
static const std::vector<uint16_t>& host_fwd(sa_ctx* c) {
  if (c->h_fwd.size() != (size_t)fwd_groups(c->L) * c->n * kSpw) fill_fwd(c, c->h_fwd, nullptr, nullptr);
  return c->h_fwd;
}
static void host_drop(sa_ctx* c) {
  std::vector<uint16_t>().swap(c->h_inv);
  std::vector<uint16_t>().swap(c->h_fwd);
}

// The tables every section kernel but k_secb reads; validates the ordering
// (distinct values in [1, w)).  A k_secg operator (Shape::big): the bucket
// table with 32-bit row entries and the 4-section Ab table alone.
int build_tables(sa_ctx* c) {
  Tables& t = c->tab;
  std::vector<uint32_t> inv32, fwd2, fwd3;
  int rc = c->big ? fill_inv(c, inv32) : fill_inv(c, c->h_inv);
  if (rc) return rc;
  fill_fwd(c, c->h_fwd, c->big ? nullptr : &fwd2, c->sec3 ? &fwd3 : nullptr);
  rc = c->big ? table_upload(c, &t.inv32, inv32) : table_upload(c, &t.inv, c->h_inv);
  if (!rc) rc = table_upload(c, &t.fwd, c->h_fwd);
  if (!rc && !c->big) rc = table_upload(c, &t.fwd2, fwd2);
  if (!rc && c->sec3) rc = table_upload(c, &t.fwd3, fwd3);
  // the packed forms of inv and fwd2 for k_sec4 / k_sec44, from the same host copies
  std::vector<uint32_t> invp;
  std::vector<uint64_t> fwd2p;
  if (!rc && c->pack_inv) {
    const size_t per = pack_inv_section_dwords(c->M, c->nhi, c->pack_kh);
    invp.assign((size_t)c->L * per, 0);
    parallel_for(c->L, 1, [&](int l) {
      pack_inv_section(c->M, c->n, c->nhi, c->pack_kh, c->h_inv.data() + (size_t)l * c->w, invp.data() + (size_t)l * per);
    });
    rc = table_upload(c, &t.invp, invp);
  }
  if (!rc && c->pack_fwd) {
    const size_t per = (size_t)pack_fwd_words(c->n) * kPackNT;
    fwd2p.assign((size_t)c->G2 * per, 0);
    parallel_for(c->G2, 1, [&](int g) {
      pack_fwd_pair(c->n, fwd2.data() + (size_t)g * c->n, fwd2p.data() + (size_t)g * per);
    });
    rc = table_upload(c, &t.fwd2p, fwd2p);
  }
  HIP_TRY(hipStreamSynchronize(c->at().stream));  // (also after a failed allocation: the vectors go)
  if (rc) return rc;
  // the host copies stay for the batched tables (ensure_invb)
  if (!(c->backend == SA_BACKEND_HADAMARD && c->CB > 0)) host_drop(c);
  return SA_OK;
}

// The bank-aware bucket table (banked_section), all sections in parallel on
// the host; uploaded into tab.invb, the steps used into tab.hs.
static int build_banked(sa_ctx* c) {
  const int L = c->L, w = c->w;
  const std::vector<int> sets = invb_sets(c->E, c->prec == SA_PREC_F32);
  const uint16_t* inv = host_inv(c).data();
  std::vector<uint16_t> out((size_t)L * w, 0);
  std::vector<uint32_t> hs((size_t)L, 0);
  parallel_for(L, 1, [&](int l) {
    banked_section(c->M, c->n, c->nhi, l, inv + (size_t)l * w, out.data() + (size_t)l * w, sets, 16, 16, hs.data(),
                   invb_kh(*c));
  });
  int rc = table_upload(c, &c->tab.invb, out);
  if (!rc) rc = table_upload(c, &c->tab.hs, hs);
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return rc;
}

// [L][w] bucket table (slot h * M + column) -> [L][nhi][64][E]: lane L's E
// entries of step h contiguous, in register order (columns elem_index<E >= 4>
// of lane L ^ 3 in binary32 (sgn), of L in binary64)
__global__ void k_lane_major(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int L, int nhi, int M,
                             int w, int E, int sgn) {
  const size_t tot = (size_t)L * nhi * 64 * E;
  for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < tot; x += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(x % E);
    size_t t = x / E;
    const int lane = (int)(t % 64);
    t /= 64;
    const int h = (int)(t % nhi), l = (int)(t / nhi);
    const int lp = sgn ? (lane ^ 3) : lane;
    const int e = (i / 4) * 256 + lp * 4 + (i % 4);
    dst[x] = src[(size_t)l * w + (size_t)h * M + e];
  }
}

// k_secb's Ab table (fwdb_group), all section groups in parallel on the host
static int build_fwdb(sa_ctx* c) {
  const int npad = (c->n + 63) & ~63;
  const uint16_t* fwd = host_fwd(c).data();
  std::vector<uint16_t> out((size_t)c->Gb * c->WB * npad, 0);
  const int rowb = c->CB * (int)rsz(c);  // bytes per staged T element
  const bool search = !(c->plan & SA_PLAN_NO_BANKS);
  parallel_for(c->Gb, 1, [&](int g) {
    fwdb_group(c->WB, c->M, c->n, c->L, c->E, rowb, search, g, fwd, npad, out.data());
  });
  if (int rc = table_upload(c, &c->tab.fwdb, out)) return rc;
  HIP_TRY(hipStreamSynchronize(c->at().stream));
  return SA_OK;
}

// The batched kernel's tables, at its first use
int ensure_invb(sa_ctx* c) {
  Tables& t = c->tab;
  // the Ab table first (every k_secb configuration reads it)
  if (c->backend == SA_BACKEND_HADAMARD && c->CB > 0 && !c->big && !t.fwdb) {
    if (c->WB * c->M >= 32768) return fail(SA_ERR_UNSUPPORTED, "k_secb: W * M >= 2^15");
    if (int rc = build_fwdb(c)) return rc;
  }
  if (t.invb_done) return SA_OK;
  t.invb_done = true;
  if (invb_banked(*c))
    if (int rc = build_banked(c)) return rc;
  // the codeword-interleaved k_secb's copy of its bucket table with each
  // lane's E entries of a step contiguous (one 16-byte load per lane and
  // step at E = 8 instead of two 8-byte loads 512 B apart)
  if (secb_rows16(*c) && c->E >= 4 && c->E % 4 == 0) {
    const size_t cnt = (size_t)c->L * c->nhi * 64 * c->E;
    if (int rc = dev_alloc(c, (void**)&t.invl, cnt * 2)) return rc;
    k_lane_major<<<(int)std::min<size_t>((cnt + 255) / 256, 16384), 256, 0, c->at().stream>>>(
        t.invb ? t.invb : t.inv, t.invl, c->L, c->nhi, c->M, c->w, c->E, c->prec == SA_PREC_F32 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->at().stream));
  }
  host_drop(c);  // the host copies have served
  return SA_OK;
}

}  // namespace sa
