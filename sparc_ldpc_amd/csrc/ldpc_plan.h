// ldpc_plan.h — the LDPC decoder's host rules as pure code: what a graph must
// satisfy (check_graph) and the tables built from it (GraphTables), what the
// library decides about a code (GraphPlan, plan_graph), about its layers
// (check_layers, LayerPlan, plan_layers) and about the fixed-point decoder on
// them (FixedPlan, plan_fixed), which decoder type a call resolves to or why it
// is refused (resolve), how a layered type launches (layered_launch) and the
// grids of the tail launches (tail_shape).
// No HIP include: csrc/lb_host_check.cpp runs these rules on a machine without
// a GPU.  lb_ctx (ldpc_bp_int.h) is a GraphPlan, a LayerPlan and a FixedPlan;
// ldpc_bp.hip validates, plans, uploads and launches by them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "ldpc_bp.h"

namespace lb {

// ---- constants --------------------------------------------------------------
constexpr size_t kLdsBytes = 160 * 1024;  // the LDS of a CU; a workgroup's dynamic part may take all but 64 bytes
constexpr int kMaxThreads = 1024;
// DCFIX > 0 instances (lxfb_fixed): at most kFixThreads threads, so that a thread may hold the
// two chains in registers: 3 waves per SIMD
constexpr int kFixThreads = 768;
constexpr int kTailFixThreads = 256, kTailThreads = 128;  // k_bp_tail_chk: the lane-pair form / one thread per check
// first iteration of the tail launches (0: off); LDPC_BP_TAIL overrides
constexpr int kTailAt = 8;
constexpr int kTailChunk = 8;  // tail iterations per stop test

// ---- measurement and test switches ------------------------------------------
// One LDPC_BP_* variable of the environment: whether it is set to a non-empty string, and its atoi
struct Switch {
  bool set = false;
  int v = 0;
};
inline Switch parse_switch(const char* e) { return (e && *e) ? Switch{true, atoi(e)} : Switch{}; }

// The rules below take the switches by value and never read the environment themselves.
struct Switches {
  Switch tail;                  // LDPC_BP_TAIL: the first tail iteration (plan_graph)
  Switch layered_lds;           // LDPC_BP_LAYERED_LDS = 1 / 0 keeps r / r and app out of LDS although they would fit
  Switch layered_threads;       // LDPC_BP_LAYERED_THREADS: the workgroup's threads (a multiple of 64 within the instance's bound)
  Switch layered_f32_resident;  // LDPC_BP_LAYERED_F32_RESIDENT = 1: one binary32 workgroup per CU (padded dynamic LDS),
                                // to time against the two that share a CU at 802.16 5/6 z=192
  Switch fixed_lanes;           // LDPC_BP_FIXED_LANES: lanes per check of the fixed-point decoder (1, 2, 4, 8 or 16)
  Switch fixed_threads;         // LDPC_BP_FIXED_THREADS: its threads per workgroup (a multiple of 64 up to 1024)
};
struct SwitchName {
  const char* name;
  Switch Switches::*field;
};
constexpr SwitchName kSwitchNames[] = {
    {"LDPC_BP_TAIL", &Switches::tail},
    {"LDPC_BP_LAYERED_LDS", &Switches::layered_lds},
    {"LDPC_BP_LAYERED_THREADS", &Switches::layered_threads},
    {"LDPC_BP_LAYERED_F32_RESIDENT", &Switches::layered_f32_resident},
    {"LDPC_BP_FIXED_LANES", &Switches::fixed_lanes},
    {"LDPC_BP_FIXED_THREADS", &Switches::fixed_threads},
};
// every getenv of the decode side (lb_create, lb_set_layers, and lb_set_fixed on a context with layers)
inline Switches read_switches() {
  Switches s;
  for (const SwitchName& n : kSwitchNames) s.*n.field = parse_switch(getenv(n.name));
  return s;
}

// a rule's refusal: the message into err, the LB_ERR_* code back
inline int refuse(std::string& err, int code, const std::string& msg) {
  err = msg;
  return code;
}

// ---- the graph ----------------------------------------------------------------
// Check degree classes of the kernel instances: the unrolled length DCMAX of lxfb, and the
// fixed-point kernels' edges over a group's lanes (20 is the 802.16 5/6 codes' degree and keeps
// their lanes at 10 edges, not 16)
constexpr int dc_class(int maxdc) { return maxdc <= 8 ? 8 : maxdc <= 16 ? 16 : 32; }
constexpr int dc_class_fixed(int maxdc) { return maxdc <= 16 ? dc_class(maxdc) : maxdc <= 20 ? 20 : 32; }
constexpr int edges_per_lane(int dcmax, int g) { return (dcmax + g - 1) / g; }

// What lb_create decides about a code, after check_graph
struct GraphPlan {
  int Nv = 0, Nc = 0, Nmsg = 0, maxdv = 0, maxdc = 0, mindc = 0;
  int dcmax = 0;       // dc_class(maxdc)
  bool lds = false;    // flooding: the messages (one binary64 per edge) live in LDS
  int nt = 0;          // flooding: threads per workgroup
  bool fixed = false;  // check-regular with a straight-line check kernel (lxfb_fixed)
  // tail launches (k_bp_tail): variable-degree class (ports in fours, 0: no tail), the first tail
  // iteration (lb_set_tail) and the one chosen at lb_create (kTailAt or LDPC_BP_TAIL)
  int nq = 0, tail_at = 0, tail_default = 0;
};

// lb_create's validation (the reference trusts its own prepare_decoder).  LB_OK with the degrees'
// summary in g (Nv .. mindc), or the code with its message in err.
inline int check_graph(const long* vdeg, const long* cdeg, const long* intrlv, int Nv, int Nc, int Nmsg, GraphPlan& g,
                       std::string& err) {
  if (!vdeg || !cdeg || !intrlv || Nv <= 0 || Nc <= 0 || Nmsg <= 0) return refuse(err, LB_ERR_ARG, "empty or null graph");
  long sv = 0, sc = 0;
  int maxdv = 0, maxdc = 0, mindc = 1 << 30;
  for (int j = 0; j < Nv; ++j) {
    if (vdeg[j] < 0) return refuse(err, LB_ERR_GRAPH, "negative variable degree");
    sv += vdeg[j];
    maxdv = vdeg[j] > maxdv ? (int)vdeg[j] : maxdv;
  }
  for (int j = 0; j < Nc; ++j) {
    if (cdeg[j] < 1) return refuse(err, LB_ERR_GRAPH, "check node of degree < 1");
    sc += cdeg[j];
    maxdc = cdeg[j] > maxdc ? (int)cdeg[j] : maxdc;
    mindc = cdeg[j] < mindc ? (int)cdeg[j] : mindc;
  }
  if (sv != Nmsg || sc != Nmsg) return refuse(err, LB_ERR_GRAPH, "sum(vdeg) and sum(cdeg) must equal Nmsg");
  if (maxdc > 32) return refuse(err, LB_ERR_UNSUPPORTED, "check degree > 32");
  if (maxdv > 255) return refuse(err, LB_ERR_UNSUPPORTED, "variable degree > 255");
  std::vector<char> seen(Nmsg, 0);
  for (int i = 0; i < Nmsg; ++i) {
    if (intrlv[i] < 0 || intrlv[i] >= Nmsg || seen[intrlv[i]]) return refuse(err, LB_ERR_GRAPH, "intrlv is not a permutation");
    seen[intrlv[i]] = 1;
  }
  g = GraphPlan();
  g.Nv = Nv; g.Nc = Nc; g.Nmsg = Nmsg; g.maxdv = maxdv; g.maxdc = maxdc; g.mindc = mindc;
  return LB_OK;
}

// The device's tables of a checked graph
struct GraphTables {
  std::vector<int> vedge;     // [max(maxdv, 1)][Nv] message index of port k of variable node j
  std::vector<uint8_t> vdeg;  // [Nv]
  std::vector<int> cstart;    // [Nc+1] first message of each check node
  // edge table of the tail and the layered kernels: the variable node of each edge
  // (kept on the host as well: check_layers holds the layers against it)
  std::vector<int> evar;      // [Nmsg]
};
inline GraphTables graph_tables(const long* vdeg, const long* cdeg, const long* intrlv, const GraphPlan& g) {
  GraphTables t;
  t.vedge.assign((size_t)std::max(g.maxdv, 1) * g.Nv, 0);
  t.vdeg.resize(g.Nv);
  t.cstart.resize(g.Nc + 1);
  t.evar.resize(g.Nmsg);
  long p = 0;
  for (int j = 0; j < g.Nv; ++j) {
    t.vdeg[j] = (uint8_t)vdeg[j];
    for (int k = 0; k < vdeg[j]; ++k, ++p) {
      t.vedge[(size_t)k * g.Nv + j] = (int)intrlv[p];
      t.evar[intrlv[p]] = j;
    }
  }
  t.cstart[0] = 0;
  for (int j = 0; j < g.Nc; ++j) t.cstart[j + 1] = t.cstart[j] + (int)cdeg[j];
  return t;
}

// check-regular codes whose degree has a straight-line instance (lxfb_fixed)
inline bool fixed_dc(int mindc, int maxdc, int nt) { return mindc == maxdc && maxdc == 20 && nt <= kFixThreads; }

// g: check_graph's summary; the rest of the plan
inline GraphPlan plan_graph(GraphPlan g, Switches sw) {
  g.dcmax = dc_class(g.maxdc);
  g.lds = (size_t)g.Nmsg * sizeof(double) <= kLdsBytes - 64;
  // one thread per check node when possible (the check phase dominates)
  g.nt = std::min(kMaxThreads, std::max(256, (g.Nc + 63) / 64 * 64));
  g.fixed = fixed_dc(g.mindc, g.maxdc, g.nt);
  g.nq = g.maxdv <= 12 ? std::max(1, (g.maxdv + 3) / 4) : 0;
  g.tail_at = !g.nq ? 0 : sw.tail.set ? std::max(0, sw.tail.v) : kTailAt;
  g.tail_default = g.tail_at;
  return g;
}

// ---- the layers -----------------------------------------------------------------
// What lb_set_layers decides: the layers' sizes (check_layers), where the messages live
// (2: r + app in LDS, 1: app in LDS, 0: HBM) and threads per workgroup (plan_layers)
struct LayerPlan {
  int nlayers = 0, maxlayer = 0, maxedges = 0;  // the largest layer's checks and edges
  int lmode = 0, lnt = 0;
  int lmode32 = 0;      // lmode of the binary32 instances (LB_F32): the same choice at 4 bytes a message
  bool lfixed = false;  // check-regular of degree 20: the DCFIX instances, at most kFixThreads threads
  bool lone32 = false;  // LDPC_BP_LAYERED_F32_RESIDENT = 1: binary32 workgroups padded to one per CU
};

// lb_set_layers' validation against the graph's host tables (GraphTables::cstart, evar): LB_OK
// with nlayers, maxlayer and maxedges in l, or the code with its message in err.
inline int check_layers(const GraphPlan& g, const int* cstart, const int* evar, int nlayers, const int* first_check,
                        LayerPlan& l, std::string& err) {
  if (nlayers < 1 || !first_check) return refuse(err, LB_ERR_ARG, "bad layer arguments");
  if (first_check[0] != 0) return refuse(err, LB_ERR_GRAPH, "first_check[0] must be 0");
  int maxlayer = 0;
  for (int i = 0; i < nlayers; ++i) {
    if (first_check[i + 1] <= first_check[i] || first_check[i + 1] > g.Nc)
      return refuse(err, LB_ERR_GRAPH, "first_check must increase strictly from 0 to Nc (layer " + std::to_string(i) + ")");
    maxlayer = std::max(maxlayer, first_check[i + 1] - first_check[i]);
  }
  int maxedges = 0;
  for (int i = 0; i < nlayers; ++i) maxedges = std::max(maxedges, cstart[first_check[i + 1]] - cstart[first_check[i]]);
  if (first_check[nlayers] != g.Nc)
    return refuse(err, LB_ERR_GRAPH, "first_check[nlayers] = " + std::to_string(first_check[nlayers]) + " is not Nc = " +
                                std::to_string(g.Nc));
  std::vector<int> owner(g.Nv, -1);
  for (int i = 0; i < nlayers; ++i)
    for (int e = cstart[first_check[i]]; e < cstart[first_check[i + 1]]; ++e) {
      const int v = evar[e];
      if (owner[v] == i)
        return refuse(err, LB_ERR_GRAPH, "layer " + std::to_string(i) + ": variable " + std::to_string(v) + " occurs twice");
      owner[v] = i;
    }
  l = LayerPlan();
  l.nlayers = nlayers; l.maxlayer = maxlayer; l.maxedges = maxedges;
  return LB_OK;
}

// where a layered decoder's messages of el bytes live
inline int layered_mode(const GraphPlan& g, size_t el) {
  const size_t app_bytes = (size_t)g.Nv * el, r_bytes = (size_t)g.Nmsg * el;
  return app_bytes + r_bytes <= kLdsBytes - 64 ? 2 : (app_bytes <= kLdsBytes - 64 ? 1 : 0);
}

// l: check_layers' sizes; the rest of the plan
inline LayerPlan plan_layers(const GraphPlan& g, LayerPlan l, Switches sw) {
  l.lmode = layered_mode(g, sizeof(double));
  l.lmode32 = layered_mode(g, sizeof(float));
  if (sw.layered_lds.set) {
    l.lmode = std::min(l.lmode, std::max(0, sw.layered_lds.v));
    l.lmode32 = std::min(l.lmode32, std::max(0, sw.layered_lds.v));
  }
  l.lfixed = g.mindc == g.maxdc && g.maxdc == 20;
  // a thread per edge of the largest layer: gather and scatter take one pass where the bound
  // allows, the check chains run on the first waves (measured against a thread per check at
  // 802.16 5/6 z=192)
  const int ntmax = l.lfixed ? kFixThreads : kMaxThreads;
  l.lnt = std::min(ntmax, std::max(128, (l.maxedges + 63) / 64 * 64));
  if (sw.layered_threads.set) l.lnt = std::min(ntmax, std::max(64, sw.layered_threads.v / 64 * 64));
  l.lone32 = sw.layered_f32_resident.set && sw.layered_f32_resident.v == 1;
  return l;
}

// ---- fixed point ------------------------------------------------------------------
// Fixed-point layered min-sum (k_bplq): the widths (lb_set_fixed) and the plan made by
// lb_set_layers / lb_set_fixed: threads per workgroup, lanes per check, dynamic LDS bytes,
// whether the image fits
struct FixedPlan {
  int qfrac = 2, qmsg = 6, qapp = 8;
  int qnt = 0, qlanes = 0, qlds = 0;
  bool qfit = false;
};

// lb_set_fixed's width check
inline int check_widths(int frac_bits, int msg_bits, int app_bits, std::string& err) {
  if (frac_bits < 0 || frac_bits > 8 || msg_bits < 2 || msg_bits > 8 || app_bits < msg_bits || app_bits > 16)
    return refuse(err, LB_ERR_ARG, "fixed-point widths: frac_bits in 0..8, msg_bits in 2..8, app_bits in msg_bits..16");
  return LB_OK;
}

// Lanes: the largest power of two, at most the largest check degree and 16, at which the largest
// layer's groups still fit 768 threads (measured at 802.16 5/6 z=192, DESIGN.md section 10b: 4
// lanes against 2 and 8); threads: a lane for every group of the largest layer, and all 1024
// where that is more than a third of a CU's 2048 (two workgroups share a CU either way, and the
// loops over all checks and variables take fewer passes).
inline FixedPlan plan_fixed(int frac_bits, int msg_bits, int app_bits, int maxdc, int maxlayer, int Nv, int Nmsg,
                            Switches sw) {
  int cap = 1;
  while (cap * 2 <= maxdc && cap < 16) cap *= 2;
  int g = 1;
  while (g * 2 <= cap && (long long)maxlayer * g * 2 <= 768) g *= 2;
  if (const int v = sw.fixed_lanes.v; sw.fixed_lanes.set && (v == 1 || v == 2 || v == 4 || v == 8 || v == 16)) g = v;
  long long nt = std::min<long long>(kMaxThreads, ((long long)maxlayer * g + 63) / 64 * 64);
  if (nt * 3 > 2048) nt = kMaxThreads;
  if (sw.fixed_threads.set) nt = std::min(kMaxThreads, sw.fixed_threads.v / 64 * 64);
  FixedPlan q;
  q.qfrac = frac_bits; q.qmsg = msg_bits; q.qapp = app_bits;
  q.qlanes = g;
  q.qnt = (int)std::max<long long>(64, nt);
  const long long bytes = (2LL * Nv + Nmsg + 15) / 16 * 16;
  q.qfit = bytes <= (long long)kLdsBytes - 64;
  q.qlds = (int)std::min<long long>(bytes, INT32_MAX);
  return q;
}

// ---- decoder types ------------------------------------------------------------------
// the fixed-point kernels' parameters: fraction bits, the clips of r and app, 16 corr_factor
struct FixedPar {
  int frac, rmax, amax, alpha;
};
// A decoder type (`algo` of the C ABI: one of the five LB_* numbers, with LB_F32 or LB_FIXED) as
// resolve found it on a context's plans; what launch, stream_plan and launch_stream take.
struct DecType {
  int base = 0;   // LB_SUMPROD2 .. LB_LAYERED_MINSUM
  bool f32 = false, fixed = false;
  bool hbm = false;  // a layered type that keeps each word's messages in a slice of HBM (lmode < 2)
  FixedPar par{};    // fixed
};

// binary32 with app in HBM keeps it behind r in the word's slice of d_msg (Nmsg doubles)
inline int f32_slice_fits(const GraphPlan& g, const LayerPlan& l, const DecType& t, std::string& err) {
  if (t.f32 && l.lmode32 == 0 && g.Nv > g.Nmsg)
    return refuse(err, LB_ERR_UNSUPPORTED, "binary32 layered decoder without LDS needs Nv <= Nmsg");
  return LB_OK;
}

// Fill `t`, or refuse algo / corr / max_iter on these plans (LB_ERR_ARG, LB_ERR_UNSUPPORTED, the
// message in err): every refusal of a decoder type is here.  for_stream: the block stream, which
// has the layered types only and refuses up front what the batch path refuses once it has work.
inline int resolve(const GraphPlan& g, const LayerPlan& l, const FixedPlan& q, int algo, double corr, int max_iter,
                   bool for_stream, DecType* t, std::string& err) {
  DecType d;
  d.f32 = algo >= 0 && (algo & LB_F32);
  d.fixed = algo >= 0 && (algo & LB_FIXED);
  d.base = algo >= 0 ? algo & ~(LB_F32 | LB_FIXED) : algo;
  if (d.base < LB_SUMPROD2 || d.base > LB_LAYERED_MINSUM) return refuse(err, LB_ERR_ARG, "unknown decoder type");
  const bool layered = d.base >= LB_LAYERED_SUMPROD2;
  // LB_FIXED goes with layered min-sum alone
  if (d.fixed && d.f32) return refuse(err, LB_ERR_ARG, "LB_FIXED | LB_F32: the fixed-point decoder has no binary32 form");
  if (d.fixed && d.base != LB_LAYERED_MINSUM)
    return refuse(err, LB_ERR_UNSUPPORTED, "fixed-point (LB_FIXED) exists for layered min-sum (LB_LAYERED_MINSUM) only");
  if (d.f32 && !layered) return refuse(err, LB_ERR_UNSUPPORTED, "binary32 (LB_F32) exists for the layered decoder types only");
  if (for_stream && !layered)
    return refuse(err, LB_ERR_UNSUPPORTED, "the block stream exists for the layered decoder types only");
  if (max_iter < 0) return refuse(err, LB_ERR_ARG, "max_iter < 0");
  if (layered && !l.nlayers) return refuse(err, LB_ERR_ARG, "layered decoder on a context without layers (lb_set_layers)");
  if (d.fixed) {  // the kernel's parameters from the context's widths and corr_factor
    const double alpha = nearbyint(16.0 * corr);  // half to even, as rint in the statement
    if (!(alpha >= 1.0 && alpha <= 16.0))
      return refuse(err, LB_ERR_ARG, "fixed-point min-sum needs rint(16 corr_factor) in 1..16");
    if (!q.qfit)
      return refuse(err, LB_ERR_UNSUPPORTED, "fixed-point decoder: the image (" + std::to_string(q.qlds) +
                                        " bytes) does not fit a workgroup's LDS, and there is no HBM layout");
    d.par = {q.qfrac, (1 << (q.qmsg - 1)) - 1, (1 << (q.qapp - 1)) - 1, (int)alpha};
  }
  int rc;
  if (for_stream && (rc = f32_slice_fits(g, l, d, err))) return rc;  // (lb::launch: once it has work)
  d.hbm = layered && !d.fixed && (d.f32 ? l.lmode32 : l.lmode) < 2;
  *t = d;
  return LB_OK;
}

// How a resolved layered type launches: threads per workgroup, dynamic LDS bytes, and its
// instance class as numbers.  Floating point: k_bpl / k_bpl32 <ALGO, dcmax, dcfix, mode>;
// fixed point: k_bplq<lanes, epl>, epl the edges of the degree class dcmax over a group's lanes.
struct LayeredLaunch {
  int nt = 0;
  size_t shm = 0;
  int dcmax = 0;           // 8 / 16 / 32; fixed point: 8 / 16 / 20 / 32
  int dcfix = 0;           // 0 / 20
  int mode = 0;            // lmode / lmode32
  int lanes = 0, epl = 0;  // fixed point
};
inline LayeredLaunch layered_launch(const GraphPlan& g, const LayerPlan& l, const FixedPlan& q, const DecType& t) {
  LayeredLaunch s;
  if (t.fixed) {
    s.nt = q.qnt;
    s.shm = (size_t)q.qlds;
    s.dcmax = dc_class_fixed(g.maxdc);
    s.lanes = q.qlanes;
    s.epl = edges_per_lane(s.dcmax, s.lanes);
    return s;
  }
  const size_t el = t.f32 ? sizeof(float) : sizeof(double);
  s.mode = t.f32 ? l.lmode32 : l.lmode;
  s.dcmax = l.lfixed ? 32 : g.dcmax;
  s.dcfix = l.lfixed ? 20 : 0;
  s.nt = l.lnt;
  s.shm = s.mode == 2 ? (size_t)(g.Nv + g.Nmsg) * el : s.mode == 1 ? (size_t)g.Nv * el : 0;
  // measurement switch: more than half a CU's LDS, so that a binary32 workgroup has its CU alone
  if (t.f32 && l.lone32) s.shm = std::max(s.shm, kLdsBytes / 2 + 64);
  return s;
}

// ---- the tail launches -----------------------------------------------------------------
// The grids of the tail launches (k_bp_tail) over the n of B words that phase one left running.
// nsz, the words the grids are sized for: exact (sized_on_host), or the last device-sized tail's
// share est_n / est_B of its batch applied to this one (a quarter before any), with slack.
// m waves per workgroup so that the words' waves (one thread per check) cover the SIMDs of ncu
// CUs once: S = ceil(Nc / (cpt m)) workgroups per word.  split: the straight-line check rule,
// which runs on lane pairs (32 checks per wave).
struct TailShape {
  int nsz, cpt, m, S;  // cpt: checks per wave
};
inline TailShape tail_shape(int B, int n, bool sized_on_host, int est_n, int est_B, int Nc, int ncu, bool split) {
  TailShape s;
  s.nsz = n;
  if (!sized_on_host) {
    const double share = est_B > 0 ? (double)est_n / est_B : 0.25;
    s.nsz = std::min(B, std::max(8, (int)std::ceil(share * B * 1.25)));
  }
  s.cpt = split ? 32 : 64;
  const long waves = (long)s.nsz * ((Nc + s.cpt - 1) / s.cpt);
  const int mmax = (split ? kTailFixThreads : kTailThreads) / 64;
  s.m = (int)((waves + 4L * ncu - 1) / (4L * ncu));
  s.m = s.m < 1 ? 1 : (s.m > mmax ? mmax : s.m);
  s.S = (Nc + s.cpt * s.m - 1) / (s.cpt * s.m);
  return s;
}

}  // namespace lb
