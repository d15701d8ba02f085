// Internal interface between gate_head.hip (C-ABI entry points, generic kernels) and rows_fast.hip (aligned fast paths):
// the launchers of what csrc/rows_route.hpp planned.
#pragma once
#include "common.hpp"
#include "rows_route.hpp"

namespace mml {

// Launch one kernel on the grid and block of the plan `p` and the stream `st` of the calling function, and return from it
// with the launch's status.  The kernel is written with literal template arguments: on success that very text becomes what
// mml_rows_last_kernel() reports.  `args`: the kernel's arguments in parentheses.
#define MML_ROWS_ARGS(...) __VA_ARGS__
#define MML_ROWS_LAUNCH(what, lds, args, ...)                                                          \
  do {                                                                                                 \
    MML_LAUNCH((__VA_ARGS__), dim3(p.grid), dim3(p.block), (size_t)(lds), st, MML_ROWS_ARGS args);     \
    return rows_launched(#__VA_ARGS__, what);                                                          \
  } while (0)
int rows_launched(const char* symbol, const char* what);  // (gate_head.hip)

// the fast families of a plan; slab: the workspace of a backward / training call
int gate_launch_fast(const mml_gate_group& g, const GatePlan& p, float* slab, hipStream_t st);
int head_launch_fast(const mml_head_group& g, const HeadPlan& p, float* slab, bool train, hipStream_t st);

}  // namespace mml
