// lb_host_check — the LDPC decoder's host rules from the command line, on a
// machine without a GPU (ldpc_plan.h and ldpc_bp.h only; no HIP).
//
//   lb_host_check plan [frac msg app [algo corr max_iter for_stream]] [tables] [LDPC_BP_NAME=value ...]
//     reads one code from stdin as whitespace-separated integers: Nv Nc Nmsg
//     nlayers, then vdeg[Nv], cdeg[Nc], intrlv[Nmsg] and, with nlayers != 0,
//     first_check[nlayers + 1].  One JSON object: the GraphPlan, a checksum
//     (64-bit FNV-1a over the entries) and the size of each of the four
//     tables, with nlayers != 0 the LayerPlan and the FixedPlan at the given
//     widths (2 6 8 without), and with algo the resolved decoder type, for a
//     layered type with its launch shape and instance class.  `tables` adds
//     the four tables in full.  The switches are taken from the NAME=value
//     words, never from the environment.  {"error", "message"} for whatever
//     lb_create, lb_set_layers, lb_set_fixed or a decode would refuse.
//   lb_host_check tail B n sized_on_host est_n est_B Nc ncu split
//     the TailShape of a tail over the n of B words that phase one left running.
// Exit status 2 on a malformed command line or input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "ldpc_plan.h"

using namespace lb;

// one field of a JSON object, by its name in the struct
#define F(s, x) std::printf("\"" #x "\": %lld, ", (long long)s.x);
#define LAST(s, x) std::printf("\"" #x "\": %lld}", (long long)s.x);

static int usage() {
  std::fprintf(stderr, "usage: lb_host_check plan [frac msg app [algo corr max_iter for_stream]] [tables] [LDPC_BP_NAME=value ...]"
                       " < code\n"
                       "       lb_host_check tail B n sized_on_host est_n est_B Nc ncu split\n");
  return 2;
}

static int refused(int rc, const std::string& err) {
  std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
  return 0;
}

template <typename T>
static void table(const char* name, const std::vector<T>& v, bool full) {
  uint64_t h = 1469598103934665603ull;
  for (T x : v) h = (h ^ (uint64_t)(uint32_t)x) * 1099511628211ull;
  std::printf("\"%s\": {\"size\": %zu, \"fnv\": %llu", name, v.size(), (unsigned long long)h);
  if (full) {
    std::printf(", \"values\": [");
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)v[i]);
    std::printf("]");
  }
  std::printf("}, ");
}

// `count` integers of stdin (none for count <= 0); false when the input ends early
static bool read_longs(std::vector<long>& v, long count) {
  v.clear();
  for (long i = 0, x; i < count; ++i) {
    if (!(std::cin >> x)) return false;
    v.push_back(x);
  }
  return true;
}

static int cmd_plan(const std::vector<double>& a, bool full, Switches sw) {
  if (a.size() != 0 && a.size() != 3 && a.size() != 7) return usage();
  std::vector<long> head, vdeg, cdeg, intrlv, first;
  if (!read_longs(head, 4)) return usage();
  const int Nv = (int)head[0], Nc = (int)head[1], Nmsg = (int)head[2], nlayers = (int)head[3];
  if (!read_longs(vdeg, Nv) || !read_longs(cdeg, Nc) || !read_longs(intrlv, Nmsg) ||
      !read_longs(first, nlayers ? (long)nlayers + 1 : 0))
    return usage();
  const std::vector<int> first_check(first.begin(), first.end());
  std::string err;
  int rc;
  GraphPlan g;
  if ((rc = check_graph(vdeg.data(), cdeg.data(), intrlv.data(), Nv, Nc, Nmsg, g, err))) return refused(rc, err);
  const GraphTables t = graph_tables(vdeg.data(), cdeg.data(), intrlv.data(), g);
  g = plan_graph(g, sw);
  LayerPlan l;
  FixedPlan q;
  if (a.size() >= 3) {
    if ((rc = check_widths((int)a[0], (int)a[1], (int)a[2], err))) return refused(rc, err);
    q = FixedPlan{(int)a[0], (int)a[1], (int)a[2]};
  }
  if (nlayers) {
    if ((rc = check_layers(g, t.cstart.data(), t.evar.data(), nlayers, first_check.data(), l, err))) return refused(rc, err);
    l = plan_layers(g, l, sw);
    q = plan_fixed(q.qfrac, q.qmsg, q.qapp, g.maxdc, l.maxlayer, g.Nv, g.Nmsg, sw);
  }
  DecType d;
  if (a.size() == 7 && (rc = resolve(g, l, q, (int)a[3], a[4], (int)a[5], a[6] != 0, &d, err))) return refused(rc, err);
  std::printf("{\"graph\": {");
  F(g, Nv) F(g, Nc) F(g, Nmsg) F(g, maxdv) F(g, maxdc) F(g, mindc) F(g, dcmax) F(g, lds) F(g, nt) F(g, fixed) F(g, nq)
  F(g, tail_at) LAST(g, tail_default)
  std::printf(", \"tables\": {");
  table("vedge", t.vedge, full);
  table("vdeg", t.vdeg, full);
  table("cstart", t.cstart, full);
  table("evar", t.evar, full);
  std::printf("\"maxdv_rows\": %d}", std::max(g.maxdv, 1));
  std::printf(", \"layers\": {");
  F(l, nlayers) F(l, maxlayer) F(l, maxedges) F(l, lmode) F(l, lmode32) F(l, lnt) F(l, lfixed) LAST(l, lone32)
  std::printf(", \"fixed\": {");
  F(q, qfrac) F(q, qmsg) F(q, qapp) F(q, qnt) F(q, qlanes) F(q, qlds) LAST(q, qfit)
  if (a.size() == 7) {
    std::printf(", \"type\": {");
    F(d, base) F(d, f32) F(d, fixed) F(d, hbm)
    std::printf("\"par\": [%d, %d, %d, %d]}", d.par.frac, d.par.rmax, d.par.amax, d.par.alpha);
    if (d.base >= LB_LAYERED_SUMPROD2) {
      const LayeredLaunch s = layered_launch(g, l, q, d);
      std::printf(", \"launch\": {");
      F(s, nt) F(s, shm) F(s, dcmax) F(s, dcfix) F(s, mode) F(s, lanes) LAST(s, epl)
    }
  }
  std::printf("}\n");
  return 0;
}

static int cmd_tail(const std::vector<double>& a) {
  if (a.size() != 8) return usage();
  const TailShape s = tail_shape((int)a[0], (int)a[1], a[2] != 0, (int)a[3], (int)a[4], (int)a[5], (int)a[6], a[7] != 0);
  std::printf("{");
  F(s, nsz) F(s, cpt) F(s, m) LAST(s, S)
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  std::vector<double> a;
  Switches sw;
  bool full = false;
  for (int i = 2; i < argc; ++i) {
    if (const char* eq = std::strchr(argv[i], '=')) {
      const SwitchName* hit = nullptr;
      for (const SwitchName& n : kSwitchNames)
        if (std::strlen(n.name) == (size_t)(eq - argv[i]) && !std::strncmp(n.name, argv[i], eq - argv[i])) hit = &n;
      if (!hit) return usage();
      sw.*hit->field = parse_switch(eq + 1);
    } else if (!std::strcmp(argv[i], "tables")) {
      full = true;
    } else {
      char* end = nullptr;
      a.push_back(std::strtod(argv[i], &end));
      if (end == argv[i] || *end) return usage();
    }
  }
  if (!std::strcmp(argv[1], "plan")) return cmd_plan(a, full, sw);
  if (!std::strcmp(argv[1], "tail") && !full) return cmd_tail(a);
  return usage();
}
