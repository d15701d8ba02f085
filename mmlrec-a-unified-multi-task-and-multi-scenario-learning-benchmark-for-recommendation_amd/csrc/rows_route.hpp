// The dispatch rule of the gate and head row kernels (K4 / K5: mml_gate_mix_fwd, mml_gate_mix_bwd[_phase], mml_head_fwd,
// mml_head_bce_fwd_bwd[_phase]) as pure host functions: which kernel family serves a group, with which template
// arguments, grid, block and dynamic LDS, how the per-workgroup partial sums are laid out, how much workspace the call
// needs, and which groups are refused with which code and text.  No HIP in here and nothing is dereferenced but the
// descriptors themselves (pointers enter as "null or not" and as their alignment), so a plain C++ compiler builds it and
// tests/test_rows_route_cpu.py holds it against a table of launches without a GPU.  csrc/gate_head.hip is its one
// caller: every entry point validates its arguments, asks the route, and hands the plan to the launcher of the family
// (rows_fast.hip for the fast kernels), which only fills the kernel's argument block and launches.
#pragma once
#include <stdint.h>

#include "../../include/mmlrec.h"

namespace mml {

// Every switch the rule reads (gate_head.hip: rows_env() reads the environment once per process).
constexpr int ROWS_UNSET = INT32_MIN;
struct RowsEnv {
  int gate_pack;      // MMLREC_GATE_PACK: 0 = the eight separate butterflies of round 5 (no PACK forward, no HV form)
  int gate_fwd_mode;  // MMLREC_GATE_FWD_MODE: 0 = the per-gate forward kernel everywhere (measurement knob)
  int gate_bwd_mode;  // MMLREC_GATE_BWD_MODE: 0 / 1 / 2 asks for that MODE where it applies, -1 = the best applicable
  int gate_hv;        // MMLREC_GATE_HV: 0 = never eight columns per lane, 2 = also the 16-lane lab form, else the default
  int gate_fwd_wgs;   // MMLREC_GATE_FWD_WGS: workgroups per CU of the gate forward; ROWS_UNSET = 3 when ne * ng > 16, else 4
  int gate_bwd_wgs;   // MMLREC_GATE_BWD_WGS: ... of the fast gate backward
  int head_wgs;       // MMLREC_HEAD_WGS: ... of the fast head kernel
};
constexpr RowsEnv ROWS_ENV_DEFAULT = {1, -1, -1, 1, ROWS_UNSET, 4, 2};

// ---- shape constants of the kernels that the rule needs (the kernels' files include this header) ----
constexpr int FB = 256;      // fast kernels (rows_fast.hip): threads per workgroup
constexpr int FW = FB / 64;  // ... waves per workgroup; a wave holds 64 / LPS samples
constexpr int ROW_BLOCK = 256;             // generic kernels (gate_head.hip): 4 waves = 4 samples in flight per workgroup
constexpr int ROW_WAVES = ROW_BLOCK / 64;
constexpr int ROWS_MAX_WIDTH = 256;        // fast kernels: widest row (one float4 per lane of a 64-lane group)
constexpr int64_t GATE_FWD_FAST_LDS = 48 * 1024;  // per-gate forward: the gate weights
constexpr int64_t GATE_FAST_LDS = 60 * 1024;      // load-once forward and fast backward
constexpr int64_t GATE_GENERIC_LDS = 64 * 1024;   // generic backward: dWg accumulators + coefficient tables
// Persistent grids: one partial slab row per workgroup goes to the reducer.  (256 stands for the chip's compute units as it
// always did here; mml_gate_mix_bwd_workspace_bytes / mml_head_workspace_bytes assume at most 256 * 8 workgroups.)
constexpr int ROWS_GRID_CUS = 256;
constexpr int ROWS_GENERIC_PER_CU = 8;

inline int rows_lps(int width) { return width <= 64 ? 16 : (width <= 128 ? 32 : (width <= ROWS_MAX_WIDTH ? 64 : 0)); }
inline int rows_fast_grid(int64_t B, int lps, int per_cu) {
  const int spb = FW * (64 / lps);
  int64_t blocks = (B + spb - 1) / spb;
  if (blocks > (int64_t)ROWS_GRID_CUS * per_cu) blocks = (int64_t)ROWS_GRID_CUS * per_cu;
  return blocks < 1 ? 1 : (int)blocks;
}
inline int rows_generic_grid(int64_t B) {
  int64_t blocks = (B + ROW_WAVES - 1) / ROW_WAVES;
  if (blocks > ROWS_GRID_CUS * ROWS_GENERIC_PER_CU) blocks = ROWS_GRID_CUS * ROWS_GENERIC_PER_CU;
  return blocks < 1 ? 1 : (int)blocks;
}
inline bool rows_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool rows_vec4(const void* p, int64_t ld) { return rows_al16(p) && ld % 4 == 0; }

// A refusal: the code, and the text the entry point hands to set_error (`v` >= 0 is printed between the two halves).
struct RowsRefusal {
  int code;
  char msg[128];
};
inline const char* rows_refuse(RowsRefusal& why, int code, const char* a, long long v = -1, const char* b = "") {
  why.code = code;
  int n = 0;
  const int cap = (int)sizeof(why.msg);
  while (*a && n + 1 < cap) why.msg[n++] = *a++;
  if (v >= 0) {
    char dg[24];
    int k = 0;
    do dg[k++] = (char)('0' + v % 10); while (v /= 10);
    while (k && n + 1 < cap) why.msg[n++] = dg[--k];
  }
  while (*b && n + 1 < cap) why.msg[n++] = *b++;
  why.msg[n] = 0;
  return why.msg;
}

// ---- K4: the gate kernels ----
enum GateFamily {
  GATE_FWD_ONCE,     // gate_fwd_once_kernel<LPS, NE, NG, PACK, HV>: every expert row loaded once for all gates
  GATE_FWD_FAST,     // gate_fwd_fast_kernel<LPS, NE>: gate by gate
  GATE_BWD_FAST,     // gate_bwd_fast_kernel<LPS, NE, NG, MODE, HV>
  GATE_FWD_GENERIC,  // gate_mix_fwd_kernel: one wavefront per sample, any shape
  GATE_BWD_GENERIC   // gate_mix_bwd_kernel
};

struct GatePlan {
  int family;
  int lps, ne, ng, pack, hv, mode;  // the template arguments (those the family has)
  int grid, block;
  int64_t lds;                      // dynamic LDS bytes
  int32_t wg_off[MML_MAX_GATES];    // float offset of gate i's weight block inside a workgroup's slab row
  int32_t wg_total, stride;         // floats of all blocks; floats between two slab rows
  int ident;                        // every gate mixes experts 0 .. n_experts-1 in order (MMoE)
  // Backward: bytes of workspace the launch and its reduction use ([grid][stride] floats).  ws_first is non-zero when the
  // fast kernels' shape conditions hold and is checked BEFORE anything else of the plan is looked at, a refusal included
  // (the fast backward asks for its workspace before it asks whether its LDS fits).
  int64_t ws_bytes, ws_first;
  RowsRefusal why;
};

// What the rule reads of a group, gathered by gate_route from the descriptors and by gate_rows_shape from its assumptions.
struct GateDims {
  int H, gd_max, n_experts, ne_max, n_gates;
  int64_t wg_total;  // sum over ALL gates of ne * Gd
  bool vec4;         // every row this direction touches is 16-byte aligned with a pitch of 4k floats, every Gd = 4k
  bool e_bf16;       // the expert outputs arrive as bf16 (MML_GATE_E_BF16)
  bool ident;
  bool hv_pitch;     // the pitches the eight-columns-per-lane form needs in this direction (16-byte rows of bf16)
};

inline int64_t gate_fwd_once_lds(const GatePlan& p, int lps) {
  return ((int64_t)p.wg_total + (int64_t)FW * (64 / lps) * p.ng * MML_MAX_EXPERTS + (int64_t)p.ng * p.ne) * 4;
}
inline int64_t gate_bwd_fast_lds(const GatePlan& p) {
  const int spw = 64 / p.lps;
  return ((int64_t)p.wg_total + (int64_t)FW * spw * p.ng * MML_MAX_EXPERTS + (int64_t)FW * spw * p.wg_total +
          (int64_t)p.ng * p.ne) * 4;
}

// Family, template arguments and dynamic LDS of one direction.  Returns whether the fast kernels' shape conditions hold
// (the backward's workspace is then sized for them even where its LDS does not fit and the generic kernel runs).
inline bool gate_form(const GateDims& d, bool bwd, const RowsEnv& env, GatePlan& p) {
  p.family = bwd ? GATE_BWD_GENERIC : GATE_FWD_GENERIC;
  if (!d.vec4 || d.H % 4 || d.H > ROWS_MAX_WIDTH || d.gd_max > ROWS_MAX_WIDTH) return false;
  p.lps = rows_lps(d.H > d.gd_max ? d.H : d.gd_max);
  p.ne = d.ne_max <= 4 ? 4 : (d.ne_max <= 8 ? 8 : 16);
  p.ng = d.n_gates <= 2 ? 2 : (d.n_gates == 3 ? 3 : (d.n_gates <= 4 ? 4 : 8));  // 3: a PLE level at T = 2
  p.hv = 1;
  p.wg_total = (int32_t)d.wg_total;
  p.ident = d.ident ? 1 : 0;
  // does the load-once forward take the group on lane groups of `lps` lanes?
  auto once_ok = [&](int lps) {
    return env.gate_fwd_mode != 0 && d.n_experts <= p.ne && p.ne * p.ng <= 32 && gate_fwd_once_lds(p, lps) <= GATE_FAST_LDS;
  };
  // Eight row columns per lane (HV = 2; only gate_fwd_once_kernel and gate_bwd_fast_kernel have the form).  bf16 expert
  // rows wider than 128 columns under gate inputs of at most 128 (KuaiRec-32 in the bf16-storage mode): 32-lane groups,
  // two samples per wave and trip.  Lab, MMLREC_GATE_HV=2: the same on 16-lane groups for fp32 rows of 65..128 columns
  // under gate inputs of at most 64 (AE-30's MMoE: four samples per wave and trip).
  const bool wide16 = d.e_bf16 && d.H > 128;
  const bool narrow32 = env.gate_hv == 2 && !d.e_bf16 && d.H > 64 && d.H <= 128;
  if ((wide16 || narrow32) && d.H % 8 == 0 && p.ne == 4 && p.ng == 2 && env.gate_pack != 0 &&
      (!bwd || (d.ident && env.gate_bwd_mode == -1))) {
    const int lps_hv = wide16 ? 32 : 16, gd_cap = wide16 ? 128 : 64;
    if (env.gate_hv != 0 && d.n_experts <= 4 && (bwd || once_ok(lps_hv)) && d.hv_pitch && d.gd_max <= gd_cap) {
      p.lps = lps_hv;
      p.hv = 2;
    }
  }
  if (bwd) {
    if (p.ne * p.ng > 32) return false;  // register budget (upstream gradients, coefficients)
    if (gate_bwd_fast_lds(p) > GATE_FAST_LDS) return true;
    p.family = GATE_BWD_FAST;
    p.lds = gate_bwd_fast_lds(p);
    // MODE 1: identity maps, every expert row loaded once and kept; 2: loaded once per gate pass; 0: per gate and expert
    const int forced = env.gate_bwd_mode;
    if (p.hv == 2 || (d.ident && p.ne * p.ng <= 8 && forced != 2 && forced != 0)) p.mode = 1;
    else p.mode = (d.n_experts <= p.ne && forced != 0) ? 2 : 0;
    return true;
  }
  if ((int64_t)p.wg_total * 4 > GATE_FWD_FAST_LDS) return true;
  if (once_ok(p.lps)) {
    p.family = GATE_FWD_ONCE;
    p.lds = gate_fwd_once_lds(p, p.lps);
    p.pack = (p.ne == 4 && p.ng == 2 && env.gate_pack != 0) ? 1 : 0;
  } else {
    p.family = GATE_FWD_FAST;
    p.lds = (int64_t)p.wg_total * 4;
  }
  return true;
}

// The shape-only first stage, before any buffer exists: which of the fast forms a group of n_gates gates, each over all
// n_experts experts in order with inputs of gd_max columns, will get -- ASSUMING 16-byte aligned buffers and pitches that
// are multiples of 8.  Returns MML_GATE_SHAPE_* bits; gate_route below asks the same gate_form, so the two cannot disagree.
inline int gate_rows_shape(int H, int gd_max, int n_experts, int n_gates, bool e_bf16, const RowsEnv& env) {
  if (H < 1 || gd_max < 1 || n_experts < 1 || n_experts > MML_MAX_EXPERTS || n_gates < 1 || n_gates > MML_MAX_GATES) return 0;
  const GateDims d = {H, gd_max, n_experts, n_experts, n_gates, (int64_t)n_gates * n_experts * gd_max, gd_max % 4 == 0,
                      e_bf16, true, true};
  int bits = 0;
  GatePlan p{};
  gate_form(d, false, env, p);
  if (p.family != GATE_FWD_GENERIC) bits |= MML_GATE_SHAPE_FAST_FWD | (p.hv == 2 ? MML_GATE_SHAPE_HV_FWD : 0);
  p = GatePlan{};
  gate_form(d, true, env, p);
  if (p.family == GATE_BWD_FAST) bits |= MML_GATE_SHAPE_FAST_BWD | (p.hv == 2 ? MML_GATE_SHAPE_HV_BWD : 0);
  return bits;
}

// The plan of mml_gate_mix_fwd (bwd = false) or mml_gate_mix_bwd[_phase] for a group that check_gate_group has passed.
// Returns null with p filled, or the refusal's text with p.why.code set (p.ws_first / p.ws_bytes are valid either way).
inline const char* gate_route(const mml_gate_group* g, bool bwd, const RowsEnv& env, GatePlan& p) {
  p = GatePlan{};
  GateDims d = {g->H, 0, g->n_experts, 0, g->n_gates, 0, true, (g->out_bf16 & MML_GATE_E_BF16) != 0, true, true};
  for (int x = 0; x < g->n_experts; ++x) {
    d.vec4 = d.vec4 && rows_vec4(g->E[x], g->lde[x]) && (!bwd || rows_vec4(g->dE[x], g->ldde[x]));
    d.hv_pitch = d.hv_pitch && g->lde[x] % 8 == 0 &&
                 (!bwd || g->ldde[x] % ((g->out_bf16 & MML_GATE_DE_BF16) ? 8 : 4) == 0);
  }
  int32_t wg_off[MML_MAX_GATES];
  for (int i = 0; i < g->n_gates; ++i) {
    const mml_gate_desc& q = g->gate[i];
    d.vec4 = d.vec4 && q.Gd % 4 == 0 && rows_vec4(q.G, q.ldg) && rows_al16(q.Wg);
    if (!bwd) d.vec4 = d.vec4 && rows_vec4(q.mix, q.ldmix);
    if (bwd && q.active) d.vec4 = d.vec4 && rows_vec4(q.dmix, q.lddmix) && rows_vec4(q.dG, q.lddg);
    if (!bwd) d.hv_pitch = d.hv_pitch && q.ldmix % ((g->out_bf16 & MML_GATE_MIX_BF16) ? 8 : 4) == 0;
    if (q.Gd > d.gd_max) d.gd_max = q.Gd;
    if (q.ne > d.ne_max) d.ne_max = q.ne;
    if (q.ne != g->n_experts) d.ident = false;
    for (int e = 0; e < q.ne; ++e)
      if (q.expert[e] != e) d.ident = false;
    wg_off[i] = (int32_t)d.wg_total;
    d.wg_total += (int64_t)q.ne * q.Gd;
  }
  const bool shape_ok = gate_form(d, bwd, env, p);
  p.block = FB;
  if (shape_ok) {
    // The forward writes no per-workgroup partials.  Round 5: with the next trip's rows requested ahead (91 VGPRs for
    // MMoE's 4 experts x 2 gates) FOUR workgroups per CU are the best grid -- AE-30 at B = 65 536, device time of the call:
    // 45.7 us (5.2 TB/s of its own bytes) against 48.4 with five, 54.5 with six, 52.8 with eight; before the prefetch six
    // were one round of resident workgroups (64 us; eight 67-68, twelve 72).  The forward of a PLE level -- 8 experts x 3
    // gates, 148 VGPRs: three waves per SIMD -- is one round of resident workgroups at three per CU: 119.9 us against
    // 126.6 with four, 132.0 with two, B = 65 536.
    const int fwd_wgs = env.gate_fwd_wgs != ROWS_UNSET ? env.gate_fwd_wgs : (p.ne * p.ng > 16 ? 3 : 4);
    p.grid = rows_fast_grid(g->B, p.lps, bwd ? env.gate_bwd_wgs : fwd_wgs);
    for (int i = 0; i < g->n_gates; ++i) p.wg_off[i] = wg_off[i];
    p.stride = p.wg_total;
    if (bwd) p.ws_first = p.ws_bytes = (int64_t)p.grid * p.stride * 4;
  }
  if (p.family != GATE_FWD_GENERIC && p.family != GATE_BWD_GENERIC) return nullptr;
  const int64_t ws_first = p.ws_first;
  p = GatePlan{};
  p.family = bwd ? GATE_BWD_GENERIC : GATE_FWD_GENERIC;
  p.ws_first = ws_first;
  if (g->out_bf16)  // (bf16 outputs exist in the fast row kernels only: include/mmlrec.h)
    return rows_refuse(p.why, MML_ERR_UNSUPPORTED,
                       bwd ? "mml_gate_mix_bwd: out_bf16 on a shape the fast row kernel does not serve"
                           : "mml_gate_mix_fwd: out_bf16 on a shape the fast row kernel does not serve");
  p.grid = rows_generic_grid(g->B);
  p.block = ROW_BLOCK;
  if (!bwd) return nullptr;
  int32_t tot = 0;  // the generic backward keeps accumulators for the ACTIVE gates only
  for (int i = 0; i < g->n_gates; ++i) {
    p.wg_off[i] = tot;
    if (g->gate[i].active) tot += g->gate[i].ne * g->gate[i].Gd;
  }
  p.wg_total = p.stride = tot;
  p.ws_bytes = (int64_t)p.grid * tot * 4;
  p.lds = (int64_t)(tot + ROW_WAVES * MML_MAX_GATES * MML_MAX_EXPERTS) * 4;
  if (p.lds > GATE_GENERIC_LDS)
    return rows_refuse(p.why, MML_ERR_ARG, "mml_gate_mix_bwd: gate weights too large for the LDS accumulators (", p.lds, " B)");
  return nullptr;
}

// ---- K5: the head kernels ----
enum HeadFamily {
  HEAD_FAST,    // head_fast_kernel<LPS, NT, GATED, KINDS>
  HEAD_GENERIC  // head_kernel<KINDS>
};

struct HeadPlan {
  int family;
  int lps, nt, gated, kinds;     // the template arguments (those the family has)
  int grid, block;
  int32_t hmax, stride;          // widest head; training: floats per slab row (dw | dbias per head, then the loss)
  uint32_t out_bits, loss_bits;  // fast: head t's output form in bit t, its loss in bits 2t, 2t + 1
  int64_t ws_bytes;              // training: [grid][stride] floats
  RowsRefusal why;
};

// The plan of mml_head_fwd (train = false) or mml_head_bce_fwd_bwd[_phase] for a group that check_head_group has passed.
// Returns null, or the refusal's text; p is filled either way (the reduction phase alone runs on a refused group's layout).
inline const char* head_route(const mml_head_group* g, bool train, const RowsEnv& env, HeadPlan& p) {
  p = HeadPlan{};
  bool fast = true;
  for (int t = 0; t < g->n_heads; ++t) {
    const mml_head_desc& q = g->head[t];
    if (q.H > p.hmax) p.hmax = q.H;
    fast = fast && q.H % 4 == 0 && rows_vec4(q.Hin, q.ldh) && rows_al16(q.w) && (!q.w2 || rows_al16(q.w2)) &&
           (!train || rows_vec4(q.dH, q.lddh));
    if (q.gate) {
      fast = fast && rows_vec4(q.gate, q.ldgate) && (!train || rows_vec4(q.dgate, q.lddgate)) && !g->dh_bf16;
      p.gated = 1;
    }
    if (q.kind) p.kinds = 1;
    p.out_bits |= (uint32_t)(MML_HEAD_KIND_OUT(q.kind) & 1) << t;
    p.loss_bits |= (uint32_t)(MML_HEAD_KIND_LOSS(q.kind) & 3) << (2 * t);
  }
  fast = fast && p.hmax % 4 == 0 && p.hmax <= ROWS_MAX_WIDTH;
  p.stride = train ? g->n_heads * (p.hmax + 1) + 1 : 0;
  if (fast) {
    p.family = HEAD_FAST;
    p.lps = rows_lps(p.hmax);
    p.nt = g->n_heads <= 2 ? 2 : (g->n_heads <= 4 ? 4 : 8);
    // (two workgroups per CU since the trips hold U samples per lane group: the call -- kernel + the reduction of one
    // partial row per workgroup -- takes 29.4 us on AE-30 / 77.9 on PepNet at B = 65 536 against 34.3 / 83.0 with four,
    // 47.8 / 84.0 with eight, 31.5 / 104.8 with one)
    p.grid = rows_fast_grid(g->B, p.lps, env.head_wgs);
    p.block = FB;
  } else {
    p.family = HEAD_GENERIC;
    p.out_bits = p.loss_bits = 0;
    p.grid = rows_generic_grid(g->B);
    p.block = ROW_BLOCK;
  }
  p.ws_bytes = (int64_t)p.grid * p.stride * 4;
  if (fast) return nullptr;
  if (train && (g->dh_bf16 || p.gated))
    return rows_refuse(p.why, MML_ERR_UNSUPPORTED,
                       "mml_head_bce_fwd_bwd: dh_bf16 / gated heads on a shape the fast row kernel does not serve");
  if (!train && p.gated)
    return rows_refuse(p.why, MML_ERR_UNSUPPORTED, "mml_head_fwd: gated heads on a shape the fast row kernel does not serve");
  return nullptr;
}

}  // namespace mml
