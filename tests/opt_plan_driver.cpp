// Stand-alone driver of csrc/opt_plan.hpp for tests/test_opt_plan_cpu.py: reads one case per line on stdin, prints one
// plan per line.
//   case:   cus variant cold_wgs resident_per_cu u_mark max_blocks cold_loop n  then n x (numel row_elems marks warm acc skip)
//           marks / warm / acc / skip are the pointers' integer values (0 = null); nothing is dereferenced
//   plan:   flat <grid.x>
//           form <form> U <u> grid <x> <y> prop <prop> variant <variant> blk0 <n + 1 numbers where prop != 0>
//           refused <message>
#include <stdio.h>

#include <iostream>
#include <vector>

#include "opt_plan.hpp"

int main() {
  long long cus, variant, cold_wgs, per_cu, u_mark, max_blocks, cold_loop, n;
  while (std::cin >> cus >> variant >> cold_wgs >> per_cu >> u_mark >> max_blocks >> cold_loop >> n) {
    if (n < 1 || n > MML_MAX_OPT_TENSORS) {
      printf("bad case: %lld tensors\n", n);
      return 2;
    }
    std::vector<mml_opt_tensor> t((size_t)n);
    for (auto& x : t) {
      long long numel, row_elems;
      unsigned long long marks, warm, acc, skip;
      if (!(std::cin >> numel >> row_elems >> marks >> warm >> acc >> skip)) {
        printf("bad case: short tensor list\n");
        return 2;
      }
      x = mml_opt_tensor{};
      x.n = numel;
      x.row_elems = (int32_t)row_elems;
      x.grad_marks = reinterpret_cast<uint8_t*>((uintptr_t)marks);
      x.warm_rows = reinterpret_cast<uint8_t*>((uintptr_t)warm);
      x.acc64 = reinterpret_cast<int64_t*>((uintptr_t)acc);
      x.skip_rows = reinterpret_cast<const uint32_t*>((uintptr_t)skip);
    }
    mml_opt_hyper h{};
    h.kind = MML_OPT_ADAM;
    h.max_blocks = (int32_t)max_blocks;
    h.cold_loop = (int32_t)cold_loop;
    const mml::OptEnv env = {(int)variant, (int)cold_wgs, (int)per_cu, (int)u_mark};
    mml::DensePlan P;
    const char* refused = mml::opt_plan_dense(t.data(), (int)n, h, env, (int)cus, P);
    if (refused) {
      printf("refused %s\n", refused);
    } else if (P.form == mml::OPT_FLAT) {
      printf("flat %u\n", P.grid_x);
    } else {
      printf("form %d U %d grid %u %u prop %d variant %d blk0", P.form, P.u, P.grid_x, P.grid_y, P.prop, P.variant);
      for (int k = 0; P.prop != 0 && k <= n; ++k) printf(" %d", P.blk0[k]);
      printf("\n");
    }
  }
  return 0;
}
