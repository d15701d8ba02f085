// Stand-alone driver of csrc/rows_route.hpp for tests/test_rows_route_cpu.py: reads cases on stdin, prints the plan the
// rule makes for each.  Pointers are the integers given (0 = null); nothing is dereferenced.
//   case:  pack fwd_mode bwd_mode hv fwd_wgs bwd_wgs head_wgs   (fwd_wgs: a number, or  unset)   then one of
//          gate bwd B H n_experts n_gates out_bf16    n_experts x (E dE lde ldde)
//               n_gates x (G Wg mix dmix dG ldg ldmix lddmix lddg Gd ne active, then ne x expert)
//          head train B n_heads dh_bf16    n_heads x (Hin w w2 dH gate dgate ldh lddh ldgate lddgate H kind)
//          shape H gd_max n_experts n_gates e_bf16
//   out:   gate:  plan family <name> lps . ne . ng . pack . hv . mode . grid . block . lds . wg_total . stride . ident .
//                 ws . ws_first . shape <gate_rows_shape of the group's own numbers> wg_off a,b,..
//          head:  plan family <name> lps . nt . gated . kinds . grid . block . hmax . stride . out_bits . loss_bits . ws .
//          then   ok   or   refused <code> <message>;   shape prints   shape <bits>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <string>

#include "rows_route.hpp"

template <class T>
static T* ptr(std::istream& in) {
  unsigned long long v = 0;
  in >> v;
  return reinterpret_cast<T*>((uintptr_t)v);
}

static void finish(const char* why, int code) {
  if (!why) printf("ok\n");
  else printf("refused %d %s\n", code, why);
}

int main() {
  static const char* gate_names[] = {"fwd_once", "fwd_fast", "bwd_fast", "fwd_generic", "bwd_generic"};
  mml::RowsEnv env;
  std::string fwd_wgs, kind;
  while (std::cin >> env.gate_pack >> env.gate_fwd_mode >> env.gate_bwd_mode >> env.gate_hv >> fwd_wgs >> env.gate_bwd_wgs >>
         env.head_wgs >> kind) {
    env.gate_fwd_wgs = fwd_wgs == "unset" ? mml::ROWS_UNSET : atoi(fwd_wgs.c_str());
    if (kind == "gate") {
      static mml_gate_group g;
      g = mml_gate_group{};
      int bwd;
      std::cin >> bwd >> g.B >> g.H >> g.n_experts >> g.n_gates >> g.out_bf16;
      if (!std::cin || g.n_experts < 1 || g.n_experts > MML_MAX_EXPERTS || g.n_gates < 1 || g.n_gates > MML_MAX_GATES) {
        printf("bad case: gate group\n");
        return 2;
      }
      for (int x = 0; x < g.n_experts; ++x) {
        g.E[x] = ptr<const float>(std::cin); g.dE[x] = ptr<float>(std::cin);
        std::cin >> g.lde[x] >> g.ldde[x];
      }
      int gd_max = 0;
      for (int i = 0; i < g.n_gates; ++i) {
        mml_gate_desc& d = g.gate[i];
        d.G = ptr<const float>(std::cin); d.Wg = ptr<const float>(std::cin); d.mix = ptr<float>(std::cin);
        d.dmix = ptr<const float>(std::cin); d.dG = ptr<float>(std::cin);
        std::cin >> d.ldg >> d.ldmix >> d.lddmix >> d.lddg >> d.Gd >> d.ne >> d.active;
        if (!std::cin || d.ne < 1 || d.ne > MML_MAX_EXPERTS) {
          printf("bad case: gate %d\n", i);
          return 2;
        }
        for (int e = 0; e < d.ne; ++e) std::cin >> d.expert[e];
        gd_max = d.Gd > gd_max ? d.Gd : gd_max;
      }
      static mml::GatePlan p;
      const char* why = mml::gate_route(&g, bwd != 0, env, p);
      printf("plan family %s lps %d ne %d ng %d pack %d hv %d mode %d grid %d block %d lds %lld wg_total %d stride %d ident %d "
             "ws %lld ws_first %lld shape %d wg_off ",
             gate_names[p.family], p.lps, p.ne, p.ng, p.pack, p.hv, p.mode, p.grid, p.block, (long long)p.lds, p.wg_total,
             p.stride, p.ident, (long long)p.ws_bytes, (long long)p.ws_first,
             mml::gate_rows_shape(g.H, gd_max, g.n_experts, g.n_gates, (g.out_bf16 & MML_GATE_E_BF16) != 0, env));
      for (int i = 0; i < g.n_gates; ++i) printf("%s%d", i ? "," : "", p.wg_off[i]);
      printf("\n");
      finish(why, p.why.code);
    } else if (kind == "head") {
      static mml_head_group g;
      g = mml_head_group{};
      int train;
      std::cin >> train >> g.B >> g.n_heads >> g.dh_bf16;
      if (!std::cin || g.n_heads < 1 || g.n_heads > MML_MAX_HEADS) {
        printf("bad case: head group\n");
        return 2;
      }
      for (int t = 0; t < g.n_heads; ++t) {
        mml_head_desc& d = g.head[t];
        d.Hin = ptr<const float>(std::cin); d.w = ptr<const float>(std::cin); d.w2 = ptr<const float>(std::cin);
        d.dH = ptr<float>(std::cin); d.gate = ptr<const float>(std::cin); d.dgate = ptr<float>(std::cin);
        std::cin >> d.ldh >> d.lddh >> d.ldgate >> d.lddgate >> d.H >> d.kind;
      }
      mml::HeadPlan p;
      const char* why = mml::head_route(&g, train != 0, env, p);
      printf("plan family %s lps %d nt %d gated %d kinds %d grid %d block %d hmax %d stride %d out_bits %u loss_bits %u ws %lld\n",
             p.family == mml::HEAD_FAST ? "fast" : "generic", p.lps, p.nt, p.gated, p.kinds, p.grid, p.block, p.hmax, p.stride,
             p.out_bits, p.loss_bits, (long long)p.ws_bytes);
      finish(why, p.why.code);
    } else if (kind == "shape") {
      int H, gd, ne, ng, e16;
      std::cin >> H >> gd >> ne >> ng >> e16;
      printf("shape %d\n", mml::gate_rows_shape(H, gd, ne, ng, e16 != 0, env));
    } else {
      printf("bad case: kind %s\n", kind.c_str());
      return 2;
    }
    if (!std::cin) {
      printf("bad case: short input\n");
      return 2;
    }
  }
  return 0;
}
