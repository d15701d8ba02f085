// Stand-alone driver of csrc/gemm_route.hpp for tests/test_gemm_route_cpu.py: reads calls on stdin, prints the launches the
// rule plans for each.  Pointers are the integers given (0 = null); nothing is dereferenced.
//   call:  mode panel ws os nt per_cu glds planes bn pad cus   then one of
//          fwd n      n x (A W bias C lda ldw ldc M N K act w_kn relu_mask ldmask amax_a amax_w amax_out w_planes w_kexp
//                          mul prod ldmul ldprod amax_prod)
//          dgrad n    n x (dA Y ldda ldy M K act n_src accumulate relu_mask ldmask amax_out gate_h gate_g d_h d_g ld_h ld_g
//                          ld_dh ld_dg act_h act_g acc_h acc_g, then min(max(n_src, 0), MML_MAX_SRC) x
//                          (dC W lddc ldw N w_kn amax_dc amax_w w_planes w_kexp))
//          wgrad n workspace_bytes phase    n x (dC A dW dbias lddc lda lddw M N K accumulate w_kn amax_dc amax_a)
//          wsbytes n  n x (the same)
//   out:   launch <symbol> | grid <g> dyn <bytes> first <i> count <n> <the family's plan fields as name value pairs>
//          ... one line per launch, then  ok  or  refused <code> <message>;  wsbytes prints  bytes <n>
#include <stdio.h>

#include <iostream>
#include <string>
#include <vector>

#include "gemm_route.hpp"

template <class T>
static T* ptr(std::istream& in) {
  unsigned long long v = 0;
  in >> v;
  return reinterpret_cast<T*>((uintptr_t)v);
}

static void print_launch(const mml::GemmLaunch& g) {
  printf("launch %s | grid %u dyn %d first %d count %d", g.symbol, g.grid, g.dyn_lds, g.first, g.count);
  switch (g.family) {
    case mml::GEMM_PANEL: printf(" rows %d masks %d", g.rows, (int)g.masks); break;
    case mml::GEMM_WS:
      printf(" nout %d dgroup %d k7 %d masks %d n_prob %d wg_per_prob %d members ", g.nout, g.dgroup, (int)g.k7, (int)g.masks,
             g.n_prob, g.wg_per_prob);
      for (int i = 0; i < g.n_prob; ++i) printf("%s%d", i ? "," : "", (int)g.member[i]);
      break;
    case mml::GEMM_OS: break;
    case mml::GEMM_NT:
      printf(" slabs %d tiles %lld partials %d reduce %d", g.slabs, (long long)g.tiles, (int)g.partials, (int)g.reduce);
      break;
    default:
      printf(" bn %d emu %d bpl %d bcols %d k7 %d row0 %d tiles_m %d total_ntiles %d", g.bn, g.emu, (int)g.bpl, (int)g.bcols,
             (int)g.k7, g.row0, g.tiles_m, g.total_ntiles);
      if (g.epi == mml::EPI_SLAB)
        printf(" S %d chunk %d slab_floats %lld ws_off %lld partials %d reduce %d", g.S, g.chunk, (long long)g.slab_floats,
               (long long)g.ws_off, (int)g.partials, (int)g.reduce);
      break;
  }
  printf("\n");
}

static void finish(int rc, const mml::GemmRefusal& why) {
  if (rc == MML_OK) printf("ok\n");
  else printf("refused %d %s\n", rc, why.msg);
}

static std::vector<mml_gemm_wgrad_desc> read_wgrad(std::istream& in, int n) {
  std::vector<mml_gemm_wgrad_desc> d((size_t)n);
  for (auto& q : d) {
    q = mml_gemm_wgrad_desc{};
    q.dC = ptr<const float>(in); q.A = ptr<const float>(in); q.dW = ptr<float>(in); q.dbias = ptr<float>(in);
    in >> q.lddc >> q.lda >> q.lddw >> q.M >> q.N >> q.K >> q.accumulate >> q.w_kn;
    q.amax_dc = ptr<const uint32_t>(in); q.amax_a = ptr<const uint32_t>(in);
  }
  return d;
}

int main() {
  mml::GemmEnv env;
  int cus, n;
  std::string kind;
  while (std::cin >> env.mode >> env.panel_on >> env.ws_on >> env.os_on >> env.nt_mode >> env.nt_per_cu >> env.glds_on >>
         env.planes_on >> env.force_bn >> env.wgrad_pad >> cus >> kind >> n) {
    mml::GemmRefusal why;
    if (n < 0 || n > 4096) {
      printf("bad case: %d problems\n", n);
      return 2;
    }
    if (kind == "fwd") {
      std::vector<mml_gemm_fwd_desc> d((size_t)n);
      for (auto& q : d) {
        q = mml_gemm_fwd_desc{};
        q.A = ptr<const float>(std::cin); q.W = ptr<const float>(std::cin); q.bias = ptr<const float>(std::cin);
        q.C = ptr<float>(std::cin);
        std::cin >> q.lda >> q.ldw >> q.ldc >> q.M >> q.N >> q.K >> q.act >> q.w_kn;
        q.relu_mask = ptr<uint32_t>(std::cin);
        std::cin >> q.ldmask;
        q.amax_a = ptr<const uint32_t>(std::cin); q.amax_w = ptr<const uint32_t>(std::cin);
        q.amax_out = ptr<uint32_t>(std::cin); q.w_planes = ptr<const uint32_t>(std::cin);
        q.w_kexp = ptr<const int32_t>(std::cin); q.mul = ptr<const float>(std::cin); q.prod = ptr<float>(std::cin);
        std::cin >> q.ldmul >> q.ldprod;
        q.amax_prod = ptr<uint32_t>(std::cin);
      }
      finish(mml::route_fwd(d.data(), n, env, cus, why,
                            [](const mml::GemmLaunch& g, const mml_gemm_fwd_desc*) { return print_launch(g), MML_OK; }),
             why);
    } else if (kind == "dgrad") {
      std::vector<mml_gemm_dgrad_desc> d((size_t)n);
      for (auto& q : d) {
        q = mml_gemm_dgrad_desc{};
        q.dA = ptr<float>(std::cin); q.Y = ptr<const float>(std::cin);
        std::cin >> q.ldda >> q.ldy >> q.M >> q.K >> q.act >> q.n_src >> q.accumulate;
        q.relu_mask = ptr<const uint32_t>(std::cin);
        std::cin >> q.ldmask;
        q.amax_out = ptr<uint32_t>(std::cin); q.gate_h = ptr<const float>(std::cin); q.gate_g = ptr<const float>(std::cin);
        q.d_h = ptr<float>(std::cin); q.d_g = ptr<float>(std::cin);
        std::cin >> q.ld_h >> q.ld_g >> q.ld_dh >> q.ld_dg >> q.act_h >> q.act_g >> q.acc_h >> q.acc_g;
        for (int s = 0; s < q.n_src && s < MML_MAX_SRC; ++s) {
          q.dC[s] = ptr<const float>(std::cin); q.W[s] = ptr<const float>(std::cin);
          std::cin >> q.lddc[s] >> q.ldw[s] >> q.N[s] >> q.w_kn[s];
          q.amax_dc[s] = ptr<const uint32_t>(std::cin); q.amax_w[s] = ptr<const uint32_t>(std::cin);
          q.w_planes[s] = ptr<const uint32_t>(std::cin); q.w_kexp[s] = ptr<const int32_t>(std::cin);
        }
      }
      finish(mml::route_dgrad(d.data(), n, env, cus, why,
                              [](const mml::GemmLaunch& g, const mml_gemm_dgrad_desc*) { return print_launch(g), MML_OK; }),
             why);
    } else if (kind == "wgrad") {
      long long bytes;
      int phase;
      std::cin >> bytes >> phase;
      const std::vector<mml_gemm_wgrad_desc> d = read_wgrad(std::cin, n);
      finish(mml::route_wgrad(d.data(), n, bytes, phase, env, cus, why,
                              [](const mml::GemmLaunch& g, const mml_gemm_wgrad_desc*) { return print_launch(g), MML_OK; }),
             why);
    } else if (kind == "wsbytes") {
      const std::vector<mml_gemm_wgrad_desc> d = read_wgrad(std::cin, n);
      printf("bytes %lld\n", (long long)mml::wgrad_workspace_bytes(d.data(), n, env));
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
