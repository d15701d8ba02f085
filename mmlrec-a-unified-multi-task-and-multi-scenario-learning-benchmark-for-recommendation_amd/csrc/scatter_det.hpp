// Deterministic scatter, second launch (scatter_det_finalize_kernel, gather_scatter.hip): every marked row's 64-bit
// totals -> fp32, added to the gradient accumulator, the totals zeroed again.  Shared by mml_scatter_bwd_det (one entry
// per FIELD, one table per field) and mml_scatter_pool_bwd_det (one entry per TABLE).
#pragma once
#include "common.hpp"

namespace mml {

struct DetFinalArgs {
  float* gtab[MML_MAX_FIELDS];
  long long* acc64[MML_MAX_FIELDS];
  int64_t vocab[MML_MAX_FIELDS];
  int64_t markbase[MML_MAX_FIELDS];
  int32_t blk0[MML_MAX_FIELDS + 1];
  uint8_t* marks;
  const uint32_t* amax_dout;
  int32_t F, E, fix_shift, clear_marks;
};

// fills fa.blk0 (one workgroup range per entry, from fa.vocab) and launches the kernel
int launch_det_finalize(DetFinalArgs& fa, hipStream_t stream, const char* who);

}  // namespace mml
