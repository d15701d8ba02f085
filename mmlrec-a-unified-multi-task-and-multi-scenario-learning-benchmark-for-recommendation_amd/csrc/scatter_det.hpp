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

// the MML_SCATTER_DET_* flags of both deterministic scatters: unknown bits and the one exclusion are argument errors
inline int det_flags(int32_t flags, const char* who, bool* defer, int* clear_marks) {
  const int all_flags = MML_SCATTER_DET_CLEAR_MARKS | MML_SCATTER_DET_AMAX_SUPPLIED | MML_SCATTER_DET_DEFER_TOTALS;
  MML_REQUIRE((flags & ~all_flags) == 0, "%s: unknown flag bits 0x%x", who, flags & ~all_flags);
  *defer = (flags & MML_SCATTER_DET_DEFER_TOTALS) != 0;
  *clear_marks = flags & MML_SCATTER_DET_CLEAR_MARKS;
  MML_REQUIRE(!(*defer && *clear_marks), "%s: deferred totals are found through the marks: "
              "MML_SCATTER_DET_DEFER_TOTALS excludes MML_SCATTER_DET_CLEAR_MARKS", who);
  return MML_OK;
}

// the launch-wide magnitude of dOut[0:B, 0:ncols] into `slot` (a maximum does not depend on the order either)
inline int measure_dout(const float* dOut, int64_t B, int64_t ldo, int64_t ncols, uint32_t* slot, mml_stream_t stream) {
  int rc = mml_amax_reset(slot, 1, stream);
  if (rc) return rc;
  mml_amax_desc ad{};
  ad.x = dOut; ad.rows = B; ad.ld = ldo; ad.cols = (int32_t)ncols; ad.slot = slot;
  return mml_amax_batch(&ad, 1, stream);
}

}  // namespace mml
