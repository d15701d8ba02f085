// mml_opt_step_dense's launch rule as one pure host function: which kernel a group of tensors gets, its grid and what
// goes into OptLaunch.  No HIP in here and nothing is dereferenced but the descriptors themselves (pointers enter as
// integers: null or not, and the alignment of the map pointers), so a plain C++ compiler builds it and
// tests/test_opt_plan_cpu.py holds it against a table of plans without a GPU.  csrc/optim.hip is its one caller.
#pragma once
#include <stdint.h>

#include "../../include/mmlrec.h"

namespace mml {

// the wave-compacted loop of opt_dense_kernel (cold_span): rows per lane (one dword of each map), rows per wave trip
constexpr int COLD_RPL = 4, COLD_SPAN = 64 * COLD_RPL;

// the loop forms of opt_dense_kernel (described there), and the flat kernel
enum { OPT_FLAT = -1, OPT_PLAIN = 0, OPT_UNROLL2 = 1, OPT_SKIP_U = 2, OPT_MARK_U = 3, OPT_MARK_ACC_U = 4 };

// The lab knobs of the launch rule, read from the environment once (optim.hip: opt_env).
struct OptEnv {
  int variant;          // MMLREC_OPT_VARIANT: the low bits of OptLaunch.variant (bit 0 nontemporal, bit 1 2x unroll)
  int cold_wgs;         // MMLREC_OPT_COLD_WGS: workgroups per tensor at most when every tensor has a warm map, 1 .. 2 048
  int resident_per_cu;  // MMLREC_OPT_RESIDENT_PER_CU: workgroups per compute unit of the resident grid, 1 .. 64
  int u_mark;           // MMLREC_OPT_U: chunks in flight per thread of the marked forms (2, 4, 8)
};
constexpr OptEnv OPT_ENV_DEFAULT = {0, 256 * 8, 8, 2};

struct DensePlan {
  int form;  // OPT_FLAT, or the PATH of opt_dense_kernel<true, PATH, u>
  int u;
  unsigned grid_x, grid_y;
  int32_t variant, prop;                   // OptLaunch.variant / .prop
  int32_t blk0[MML_MAX_OPT_TENSORS + 1];  // OptLaunch.blk0 (prop != 0)
};

inline int64_t opt_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Plans the launch of one group: t[0 .. n) are the <= MML_MAX_OPT_TENSORS descriptors of one launch (each already
// validated by itself, at least one parameter in all), cus the device's compute units.  Returns null and the plan, or the
// refusal's message.
inline const char* opt_plan_dense(const mml_opt_tensor* t, int n, const mml_opt_hyper& h, const OptEnv& env, int cus,
                                  DensePlan& P) {
  P = DensePlan{};
  int64_t total = 0, chunks = 0, nmax = 0;
  for (int k = 0; k < n; ++k) {
    total += t[k].n;
    chunks += opt_cdiv(t[k].n, 4);
    nmax = t[k].n > nmax ? t[k].n : nmax;
  }
  P.variant = env.variant | (h.max_blocks > 0 ? 4 : 0) | (h.cold_loop == 1 ? 8 : 0);
  // the loop form (see opt_dense_kernel): decided for the launch, so every tensor of it must qualify
  bool all_gm = true, all_skip = true, none = true, any_acc = false;
  for (int k = 0; k < n; ++k) {
    any_acc = any_acc || t[k].acc64;
    all_gm = all_gm && t[k].grad_marks && !t[k].skip_rows;
    all_skip = all_skip && t[k].skip_rows;
    none = none && !t[k].grad_marks && !t[k].skip_rows;
  }
  // Round 6: a model's tables in ONE marked streaming launch (AE-30: 4 huge + 26 small; the small ones were a second
  // launch of the flat kernel, 31-34 us behind the stream): workgroups dealt in proportion to the tensors' sizes.
  const bool many = n > 4 && all_gm;
  if (any_acc && !all_gm) return "mml_opt_step_dense: a launch with acc64 tensors takes grad_marks on every tensor";
  // A group dominated by one huge tensor (the dense table update) streams with the per-tensor kernel (blockIdx.y =
  // tensor: no index search on the 2.7 GB stream); everything else (dozens of tensors from 64 B to a few MB) goes
  // through the flat kernel, where every workgroup has the same amount of work.
  if (!(total >= ((int64_t)1 << 24) && (n <= 4 || many))) {
    for (int k = 0; k < n; ++k)
      if (t[k].grad_marks)
        return "mml_opt_step_dense: grad_marks (and acc64) is only honoured by the streaming launch (>= 2^24 parameters "
               "in <= 4 tensors, or any number of marked tensors)";
    int64_t bx = opt_cdiv(chunks, 256);
    if (bx > 256 * 8) bx = 256 * 8;
    if (h.max_blocks > 0 && bx > h.max_blocks) bx = h.max_blocks;
    P.form = OPT_FLAT;
    P.grid_x = (unsigned)bx;
    P.grid_y = 1;
    return nullptr;
  }
  int64_t bx = opt_cdiv(opt_cdiv(nmax, 4), 256);
  if (bx > 256 * 8) bx = 256 * 8;
  if (h.max_blocks > 0 && bx * n > h.max_blocks) bx = opt_cdiv(h.max_blocks, n);
  P.grid_x = (unsigned)bx;
  P.grid_y = (unsigned)n;
  // Workgroups per tensor at most.  With a warm map on every tensor most of the stream is passed over and a workgroup's
  // fixed cost (tensor search, magnitude words, unbound bias corrections) is what is left of a short one:
  // MMLREC_OPT_COLD_WGS (lab knob) caps them lower.  Measured side by side at 3.8 % warm rows, 2 048 / 1 024 / 512:
  // 129.8 / 119.2 / 116.1 us -- which is why a launch that qualifies leaves this grid altogether (`resident`, below).
  bool all_warm = true;
  for (int k = 0; k < n; ++k) all_warm = all_warm && t[k].warm_rows;
  // One resident grid (cold_resident): the launch runs a kernel with the wave-compacted loop (forms 3 / 4), every
  // tensor carries a warm map with word-aligned map pointers, and the switch asks for it.  Sized for the chip -- twice
  // the kernel's workgroups that fit a compute unit (4 at its register count: two rounds, so that a workgroup whose
  // spans hold the warm head of a Zipf table is made up for by the late starters; cold_loop = 3: one round; lab knob
  // MMLREC_OPT_RESIDENT_PER_CU) x compute units -- and never above what the launch gets otherwise (max_blocks
  // included).  MMLREC_OPT_COLD_WGS means nothing here.
  bool resident = all_warm && all_gm && (any_acc || (P.variant & 4)) && (h.cold_loop == 0 || h.cold_loop == 3);
  int64_t nspan = 0;
  for (int k = 0; k < n && resident; ++k) {
    resident = (((uintptr_t)t[k].grad_marks | (uintptr_t)t[k].warm_rows) & 3) == 0;
    nspan += opt_cdiv(t[k].n / t[k].row_elems, COLD_SPAN);
  }
  resident = resident && nspan < ((int64_t)1 << 30);  // (span numbers are 32-bit in the kernel)
  const int64_t wg_cap = (all_warm && !resident) ? env.cold_wgs : 256 * 8;
  if (many) {
    // every tensor gets what a launch of its own would give it (one workgroup per 256 chunks, at most 2 048): the huge
    // tables stream exactly as in their four-tensor launch, the small ones add a few hundred workgroups (the caller
    // lists them FIRST: they start with the launch instead of trailing it).  Under a workgroup cap: in proportion.
    int64_t want = 0;
    for (int k = 0; k < n; ++k) {
      const int64_t need = opt_cdiv(opt_cdiv(t[k].n, 4), 256);
      want += need > wg_cap ? wg_cap : (need < 1 ? 1 : need);
    }
    const bool capped = h.max_blocks > 0 && want > h.max_blocks;
    int64_t tb = capped ? h.max_blocks : want;
    if (tb < n) tb = n;
    int64_t at = 0;
    for (int k = 0; k < n; ++k) {
      P.blk0[k] = (int32_t)at;
      const int64_t need = opt_cdiv(opt_cdiv(t[k].n, 4), 256);
      int64_t nb = capped ? tb * t[k].n / total : (need > wg_cap ? wg_cap : need);
      if (nb > need) nb = need;
      if (nb < 1) nb = 1;
      at += nb;
    }
    P.blk0[n] = (int32_t)at;
    P.prop = 1;
    P.grid_x = (unsigned)at;
    P.grid_y = 1;
  }
  if (resident) {
    int64_t wgs = (int64_t)P.grid_x * P.grid_y;
    const int64_t fit = (int64_t)(h.cold_loop == 3 ? 4 : env.resident_per_cu) * cus;
    if (wgs > fit) wgs = fit;
    int64_t at = 0;
    for (int k = 0; k < n; ++k) {
      P.blk0[k] = (int32_t)at;
      at += opt_cdiv(t[k].n / t[k].row_elems, COLD_SPAN);
    }
    P.blk0[n] = (int32_t)at;
    P.prop = 2;
    P.grid_x = (unsigned)(wgs < 1 ? 1 : wgs);
    P.grid_y = 1;
  }
  // the instantiation: a chunk count in flight that has no instantiation falls back to two
  if (any_acc) {  // (capped grid or not: the totals are only read by this form)
    P.form = OPT_MARK_ACC_U;
    P.u = env.u_mark == 4 ? 4 : 2;
  } else if ((P.variant & 4) && all_gm) {
    P.form = OPT_MARK_U;
    P.u = (env.u_mark == 4 || env.u_mark == 8) ? env.u_mark : 2;
  } else if ((P.variant & 4) && all_skip) {
    P.form = OPT_SKIP_U;
    P.u = 4;
  } else if ((P.variant & 2) && none) {
    P.form = OPT_UNROLL2;
    P.u = 1;
  } else {
    P.form = OPT_PLAIN;
    P.u = 1;
  }
  return nullptr;
}

}  // namespace mml
