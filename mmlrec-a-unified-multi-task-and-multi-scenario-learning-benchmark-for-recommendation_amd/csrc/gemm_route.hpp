// The dispatch rule of the grouped GEMM entry points (mml_gemm_grouped_fwd / _dgrad / _wgrad_phase) as pure host
// functions: which kernel family serves a call, with which template arguments, grid and dynamic LDS, in which order, and
// which calls are refused with which code and text.  No HIP in here and nothing is dereferenced but the descriptors
// themselves (pointers enter as integers: null or not, 16-byte alignment, equality with another pointer of the same
// call), so a plain C++ compiler builds it and tests/test_gemm_route_cpu.py holds it against a table of launches without
// a GPU.  csrc/gemm.hip is its one caller: it asks the route and hands every launch to its family's launcher
// (gemm_panel.hip, gemm_ws.hip, gemm_os.hip, gemm_nt.hip, launch_tiles in gemm.hip), which only fills the kernel's
// argument block and launches.
#pragma once
#include <stdint.h>

#include "../../include/mmlrec.h"

namespace mml {

// Every switch the rule reads (gemm.hip: gemm_env() reads the environment, the mml_gemm_set_* setters write here).
struct GemmEnv {
  int mode;       // MMLREC_GEMM_MODE / mml_gemm_set_mode: 0 fp32 MFMA, 1 bf16 operands, 3 three bf16 planes, 2 / 4 auto
  int panel_on;   // MMLREC_GEMM_PANEL / mml_gemm_set_panel
  int ws_on;      // MMLREC_GEMM_WS / mml_gemm_set_ws
  int os_on;      // MMLREC_GEMM_OS (read on every call)
  int nt_mode;    // MMLREC_GEMM_NT / mml_gemm_set_nt: 0 off, 1 every qualifying launch, 2 launches of >= 16 tiles, 3 lab
  int nt_per_cu;  // MMLREC_NT_PER_CU: workgroups of gemm_nt_kernel per CU, 1 or 2
  int glds_on;    // MMLREC_GEMM_GLDS: 0 = never the LDS-DMA tile kernel
  int planes_on;  // MMLREC_GEMM_PLANES: 0 = ignore pre-cut weights in the tile kernel
  int force_bn;   // MMLREC_GEMM_BN: 64 / 128 forces the tile width, anything else leaves it to pick_tiles
  int wgrad_pad;  // MMLREC_WGRAD_LDS_PAD / mml_gemm_set_wgrad_lds_pad: unused dynamic LDS of the wgrad tile launches
};
constexpr GemmEnv GEMM_ENV_DEFAULT = {4, 1, 1, 1, 1, 2, 1, 1, 0, 0};

// ---- shape constants of the kernels that the rule needs (the kernels' files include this header) ----
constexpr int BM = 128;          // tile kernels: rows of a block tile
constexpr int BK = 32;           // ... reduction depth of a register-staged step
constexpr int GK = 16;           // ... of an LDS-DMA step
constexpr int MAX_SOURCES = 24;  // ... sources per launch, over all problems (kernel-argument block stays < 4 KiB)
enum { EPI_FWD = 0, EPI_DGRAD = 1, EPI_SLAB = 2 };
constexpr int PN_BM = 128;   // panel kernel: rows of a panel (four waves x 32)
constexpr int PN_MAXH = 64;  // ... half tiles (64 columns) per launch
constexpr int PN_K_MIN = 160, PN_K_MAX = 320;  // ... the instantiated reduction lengths: every multiple of 16 between
constexpr int WS_W_BYTES = 128 * 1024;  // weight-stationary kernel: the weight image in LDS
constexpr int WS_MIN_ROWS = 8192;       // ... below: the tile kernel (a persistent grid would idle)
// ... k-steps per group for a reduction of `kred` values: 4 (multiples of 64), 5 (other multiples of 80), 0 = not served
constexpr int ws_dgroup(const int kred) { return kred <= 0 ? 0 : (kred % 64 == 0 ? 4 : (kred % 80 == 0 ? 5 : 0)); }
constexpr int OS_BM = 256;  // output-stationary kernel: rows of a workgroup's panel
constexpr int OS_NC = 256;  // ... output columns a workgroup holds
constexpr int NT_MAX_GROUP = 48;  // cut-once weight-gradient kernel: problems per launch
constexpr int NT_STEP = 32;       // ... batch rows per step
constexpr int NT_MIN_TILES = 16;  // ... mode 2: smallest launch it takes

enum GemmFamily { GEMM_PANEL, GEMM_WS, GEMM_OS, GEMM_NT, GEMM_PIPE, GEMM_REG };

// what the tile kernels' launch decisions read of a source / problem (the entry points copy these into Source / Problem)
struct TileSrc {
  int32_t Kred, vecA, vecB;  // reduction extent; 16-byte vector loads legal on the row / column operand
};
struct TileProb {
  int32_t M, N, src0, nsrc;  // output extent; sources [src0, src0 + nsrc) of the launch
  int32_t tiles_m, tiles_n, tile0, vec_out;
};

// One launch of a call.  `first`, `count`: the descriptors it serves, of the array that is handed on with it.
struct GemmLaunch {
  int family;
  int first, count;
  uint32_t grid;
  int32_t dyn_lds;
  char symbol[96];  // as mml_gemm_last_kernel() reports it
  // template arguments (tile kernels: all; ws: epi = MODE, masks, k7)
  bool arc, brc, bcols, bpl, k7, masks;
  int bn, epi, emu;
  // panel: rows [0, rows) of the batch; a tile launch behind it: rows [row0, M)
  int32_t rows, row0;
  // ws: one class of the call's problems
  int nout, dgroup, n_prob, wg_per_prob;
  uint8_t member[MML_MAX_GROUP];
  // nt (ntd: the lab variant gemm_ntd_kernel of mode 3, reported under gemm_nt_kernel's symbol)
  int slabs;
  int64_t tiles;
  bool ntd;
  // tile kernels
  TileSrc s[MAX_SOURCES];
  TileProb p[MML_MAX_GROUP];
  int32_t total_ntiles, tiles_m;
  // weight gradients: which of the two steps this call runs, the split of the batch and the group's piece of the workspace
  bool partials, reduce;
  int32_t S, chunk;
  int64_t slab_floats, ws_off;
};

struct GemmRefusal {
  int code;  // 0: not refused by the rule
  char msg[256];
};

// ---- text without <stdio.h> ----
struct RouteText {
  char* s;
  int cap, n;
  RouteText(char* buf, int c) : s(buf), cap(c), n(0) { s[0] = 0; }
  RouteText& operator<<(const char* t) {
    while (*t && n + 1 < cap) s[n++] = *t++;
    s[n] = 0;
    return *this;
  }
  RouteText& operator<<(long long v) {
    char dg[24];
    int k = 0;
    unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    do dg[k++] = (char)('0' + u % 10); while (u /= 10);
    if (v < 0) dg[k++] = '-';
    while (k && n + 1 < cap) s[n++] = dg[--k];
    s[n] = 0;
    return *this;
  }
  RouteText& operator<<(int v) { return *this << (long long)v; }
};
inline RouteText refuse(GemmRefusal& why, int code) {
  why.code = code;
  return RouteText(why.msg, (int)sizeof(why.msg));
}

// The one place a kernel symbol is spelled (as a profiler prints it: every template argument, the defaulted ones too).
inline void gemm_symbol(GemmLaunch& g) {
  RouteText t(g.symbol, (int)sizeof(g.symbol));
  auto tf = [](bool b) { return b ? "true" : "false"; };
  switch (g.family) {
    case GEMM_PANEL: t << "gemm_panel_kernel"; break;
    case GEMM_OS: t << "gemm_os_kernel"; break;
    case GEMM_NT: t << "gemm_nt_kernel"; break;
    case GEMM_WS:
      t << "gemm_ws_kernel<" << g.nout / 32 << ", " << g.epi << ", " << tf(g.masks && !g.k7) << ", " << g.dgroup << ", "
        << tf(g.k7) << ">";
      break;
    case GEMM_PIPE:
      t << "gemm_pipe_kernel<" << tf(g.arc) << ", " << tf(g.brc) << ", " << g.bn << ", " << g.epi << ", " << g.emu << ", "
        << tf(g.bcols) << ", " << tf(g.bpl) << ">";
      break;
    default: t << "gemm_kernel<" << tf(g.arc) << ", " << tf(g.brc) << ", " << g.bn << ", " << g.epi << ">"; break;
  }
}

inline int64_t route_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool route_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int32_t route_vec_ok(const void* p, int64_t ld) { return (route_al16(p) && ld % 4 == 0) ? 1 : 0; }
// panel / ws / os / nt run the two-plane arithmetic: in the auto modes only
inline bool planes_kernels_on(const GemmEnv& env) { return env.mode >= 2 && env.mode != 3; }

// ---- gemm_panel_kernel: forward launches whose problems all read ONE input (first DNN layers) ----
// Rows of the batch the panel kernel takes: 0 (not its call), or M - M % 128 -- the rest of a ragged batch is routed again
// (a row's result does not depend on the tile it is computed in: tests/test_gemm_panel_gpu.py).
inline int32_t panel_rows(const mml_gemm_fwd_desc* d, int n, const GemmEnv& env, bool& store_masks) {
  if (!env.panel_on || n < 1 || n > MML_MAX_GROUP) return 0;
  const mml_gemm_fwd_desc& d0 = d[0];
  // (other reduction lengths arrive padded with zero columns on both operands: AE's K0 = 303 as 304)
  if (d0.K % 16 != 0 || d0.K < PN_K_MIN || d0.K > PN_K_MAX) return 0;
  if (d0.M < PN_BM * 64) return 0;  // (small batches: the tile kernel)
  const int32_t rows = d0.M - d0.M % PN_BM;
  if (!d0.amax_a || !route_al16(d0.A) || d0.lda % 4 != 0) return 0;
  int halves = 0, masks = 0;
  for (int i = 0; i < n; ++i) {
    const mml_gemm_fwd_desc& q = d[i];
    if (q.mul || q.prod) return 0;  // (K7 products: the tile kernel's epilogue)
    if (q.A != d0.A || q.lda != d0.lda || q.M != d0.M || q.K != d0.K || q.amax_a != d0.amax_a) return 0;
    if (q.w_kn != 0 || !q.w_planes || !q.w_kexp || !route_al16(q.w_planes) || q.ldw % 4 != 0) return 0;
    if (q.N % 64 != 0 || q.N < 64) return 0;
    if (q.act != MML_ACT_RELU) return 0;
    if (!route_al16(q.C) || q.ldc % 4 != 0 || (q.bias && !route_al16(q.bias))) return 0;
    if ((int64_t)rows * q.ldc >= (1ll << 30) || (int64_t)rows * q.ldmask >= (1ll << 30)) return 0;  // (32-bit offsets)
    const bool m = q.relu_mask != nullptr;
    if (m && q.ldmask * 32 < q.N) return 0;
    masks += m ? 1 : 0;
    halves += q.N / 64;
  }
  if (halves > PN_MAXH || halves % 2 != 0) return 0;
  if (masks != 0 && masks != n) return 0;  // (the waits count the stores of a piece: all or none)
  store_masks = masks != 0;
  return rows;
}

// ---- gemm_ws_kernel: problems that each stream their own input past a weight that fits the LDS ----
inline bool ws_fwd_ok(const mml_gemm_fwd_desc& q, const mml_gemm_fwd_desc& d0) {
  if (q.M != d0.M || ws_dgroup(q.K) == 0) return false;
  if (q.N != 256 && q.N != 128 && q.N != 64) return false;  // (the instantiated output widths)
  if ((int64_t)q.N * q.K * 4 > WS_W_BYTES) return false;
  if (!q.A || !q.C || !q.w_planes || !q.w_kexp || !q.amax_a) return false;
  if (q.mul || q.prod) {  // K7: prod = act(..) (.) mul from the same turn
    if (!q.mul || !q.prod || q.ldmul < q.N || q.ldprod < q.N) return false;
    if (!route_al16(q.mul) || q.ldmul % 4 != 0 || !route_al16(q.prod) || q.ldprod % 4 != 0) return false;
    if (q.act == MML_ACT_RELU && q.relu_mask) return false;  // (no instantiation with sign masks: gates end in a sigmoid)
    if (q.N == 256) return false;                            // (nor with eight sub-tiles: registers)
  }
  if (q.act != MML_ACT_RELU && q.act != MML_ACT_NONE && q.act != MML_ACT_SIGMOID && q.act != MML_ACT_SIGMOID2) return false;
  if (!route_al16(q.A) || q.lda % 4 != 0 || !route_al16(q.C) || q.ldc % 4 != 0) return false;
  if (!q.w_kn && (!route_al16(q.w_planes) || q.ldw % 4 != 0)) return false;
  if (q.act == MML_ACT_RELU && q.relu_mask && q.ldmask * 32 < q.N) return false;
  return true;
}
// the whole call: every problem must qualify, and every class gets >= 1 workgroup per problem (decided before the first
// launch, never between two of them)
inline bool ws_fwd_serves(const mml_gemm_fwd_desc* d, int n, const GemmEnv& env, int cus) {
  if (!env.ws_on || n < 1 || n > MML_MAX_GROUP || d[0].M < WS_MIN_ROWS) return false;
  for (int i = 0; i < n; ++i)
    if (!ws_fwd_ok(d[i], d[0])) return false;
  return n <= cus;
}

inline bool ws_dgrad_ok(const mml_gemm_dgrad_desc& q, const mml_gemm_dgrad_desc& d0) {
  if (q.n_src != 1 || q.M != d0.M) return false;
  if (q.gate_h) {  // K7 gate mode: dH / dG instead of dA
    if (!q.gate_g || !q.d_h || !q.d_g || q.ld_h < q.K || q.ld_g < q.K || q.ld_dh < q.K || q.ld_dg < q.K) return false;
    if (!route_al16(q.gate_h) || !route_al16(q.gate_g) || !route_al16(q.d_h) || !route_al16(q.d_g) || q.ld_h % 4 != 0 ||
        q.ld_g % 4 != 0 || q.ld_dh % 4 != 0 || q.ld_dg % 4 != 0)
      return false;
  } else if (!q.dA) {
    return false;
  }
  const int32_t kred = q.N[0];
  if (ws_dgroup(kred) == 0) return false;
  if (q.K != 64 && q.K != 128 && q.K != 256) return false;  // (the instantiated output widths)
  if ((int64_t)q.K * kred * 4 > WS_W_BYTES) return false;
  if (!q.dC[0] || !q.w_planes[0] || !q.w_kexp[0] || !q.amax_dc[0]) return false;
  const bool m = q.act == MML_ACT_RELU && q.relu_mask != nullptr;
  if (q.gate_h) {
    if (m || q.Y || q.K == 256) return false;  // (gate mode: no derivative of the product itself; no 256-wide instantiation)
    if (!route_al16(q.dC[0]) || q.lddc[0] % 4 != 0) return false;
    if (q.w_kn[0] && (!route_al16(q.w_planes[0]) || q.ldw[0] % 4 != 0)) return false;
    return true;
  }
  if (q.act != MML_ACT_NONE && !m) return false;  // (derivatives from the stored outputs: the tile kernel)
  if (m && q.ldmask * 32 < q.K) return false;
  if (!route_al16(q.dC[0]) || q.lddc[0] % 4 != 0 || !route_al16(q.dA) || q.ldda % 4 != 0) return false;
  if (q.w_kn[0] && (!route_al16(q.w_planes[0]) || q.ldw[0] % 4 != 0)) return false;
  return true;
}
inline bool ws_dgrad_serves(const mml_gemm_dgrad_desc* d, int n, const GemmEnv& env, int cus) {
  if (!env.ws_on || n < 1 || n > MML_MAX_GROUP || d[0].M < WS_MIN_ROWS) return false;
  for (int i = 0; i < n; ++i)
    if (!ws_dgrad_ok(d[i], d[0])) return false;
  // Two problems of one call that write the same dA (an overwriting and an accumulating one) need an ORDER: the
  // problems of a class run in one kernel launch on disjoint workgroup ranges, i.e. concurrently, and classes are
  // launched in the order of their first members -- neither keeps the call's order.  Left to the tile kernel (the
  // engine never builds such a call: chunks of one input go into different launches).
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const float* ti[2] = {d[i].gate_h ? d[i].d_h : d[i].dA, d[i].gate_h ? d[i].d_g : nullptr};
      const float* tj[2] = {d[j].gate_h ? d[j].d_h : d[j].dA, d[j].gate_h ? d[j].d_g : nullptr};
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
          if (ti[a] && ti[a] == tj[b]) return false;
    }
  return n <= cus;
}

// The classes of a served call -- one kernel launch per (output width, sign masks, K7, k-steps per group) -- in the order
// of their first members.  key(i, nout, masks, k7, dgroup) describes problem i.
template <class Key, class Emit>
inline int ws_classes(int n, int epi, int cus, Key&& key, Emit&& emit) {
  bool done[MML_MAX_GROUP] = {};
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    GemmLaunch g{};
    g.family = GEMM_WS;
    g.epi = epi;
    g.first = i;
    key(i, g.nout, g.masks, g.k7, g.dgroup);
    for (int j = i; j < n; ++j) {
      int nout, dgroup;
      bool masks, k7;
      key(j, nout, masks, k7, dgroup);
      if (done[j] || nout != g.nout || masks != g.masks || k7 != g.k7 || dgroup != g.dgroup) continue;
      done[j] = true;
      g.member[g.n_prob++] = (uint8_t)j;
    }
    g.count = g.n_prob;
    g.wg_per_prob = cus / g.n_prob;
    g.grid = (uint32_t)(g.wg_per_prob * g.n_prob);
    gemm_symbol(g);
    const int rc = emit(g);
    if (rc != MML_OK) return rc;
  }
  return MML_OK;
}

// ---- gemm_os_kernel: ONE wide input gradient summed over many sources (d(dnn_input)) ----
inline bool os_serves(const mml_gemm_dgrad_desc* d, int n, const GemmEnv& env) {
  if (!env.os_on || !d || n != 1) return false;
  const mml_gemm_dgrad_desc& q = d[0];
  if (q.gate_h || q.Y || q.relu_mask || q.act != MML_ACT_NONE || !q.dA) return false;
  if (q.n_src < 2 || q.n_src > MML_MAX_SRC) return false;  // (one source: the weight-stationary kernel's)
  // (every workgroup computes OS_NC = 256 columns: a narrower gradient wastes the difference -- PLE's K = 128 launches
  // measured 1 % slower per step with this kernel than with the tile kernel, so they stay there)
  if (q.M < 16384 || q.K < 192 || q.K > OS_NC || q.K % 4 != 0) return false;
  if (!route_al16(q.dA) || q.ldda % 4 != 0 || q.ldda < q.K) return false;
  if ((int64_t)q.M * q.ldda >= (1ll << 40)) return false;
  int64_t ntot = 0;
  for (int s = 0; s < q.n_src; ++s) {
    if (q.w_kn[s] != 0 || !q.dC[s] || !q.w_planes[s] || !q.w_kexp[s] || !q.amax_dc[s]) return false;
    if (q.w_kexp[s] != q.w_kexp[0]) return false;  // (one group, one exponent)
    if (q.N[s] <= 0 || q.N[s] % 16 != 0) return false;
    if (!route_al16(q.dC[s]) || q.lddc[s] % 4 != 0 || q.lddc[s] < q.N[s]) return false;
    if (!route_al16(q.w_planes[s]) || q.ldw[s] % 4 != 0 || q.ldw[s] < q.K) return false;
    ntot += q.N[s];
  }
  return ntot >= 256;  // (short reductions: the ring would not fill)
}

// ---- gemm_nt_kernel: weight gradients cut once per workgroup (large batches, both operand magnitudes known) ----
inline bool nt_problem_ok(const mml_gemm_wgrad_desc& q) {
  if (q.M < 16384 || q.M % NT_STEP != 0) return false;
  if (q.w_kn || !q.dC || !q.A || !q.dW || !q.amax_dc || !q.amax_a) return false;
  if (q.N <= 0 || q.N % 32 != 0 || q.K <= 0 || q.K % 4 != 0) return false;
  if (!route_al16(q.dC) || !route_al16(q.A) || q.lddc % 4 != 0 || q.lda % 4 != 0 || q.lddc < q.N || q.lda < q.K ||
      q.lddw < q.K)
    return false;
  return true;
}
// The whole call; fills g (slabs, tiles, grid, dynamic LDS).  The decision depends on the descriptors and the workspace
// size only, so phase 2 of a call pair decides like its phase 1.
inline bool nt_serves(const mml_gemm_wgrad_desc* d, int n, int64_t workspace_bytes, const GemmEnv& env, int cus,
                      GemmLaunch& g) {
  if (env.nt_mode == 0 || n < 1 || n > NT_MAX_GROUP) return false;
  const int32_t M = d[0].M;
  if (M < 16384 || M % NT_STEP != 0) return false;
  int64_t tiles = 0, elems = 0;
  for (int i = 0; i < n; ++i) {
    const mml_gemm_wgrad_desc& q = d[i];
    if (q.M != M || !nt_problem_ok(q)) return false;
    tiles += route_cdiv(q.N, 128) * route_cdiv(q.K, 128);
    elems += (int64_t)q.N * q.K + q.N;
  }
  if (env.nt_mode == 2 && tiles < NT_MIN_TILES) return false;
  const int steps = M / NT_STEP;
  int64_t slabs = (env.nt_per_cu * (int64_t)cus) / tiles;  // two workgroups per CU (64 KiB of LDS each), or one
  if (slabs > steps / 8) slabs = steps / 8;                // at least 256 batch rows per slab
  if (slabs > 64) slabs = 64;
  const int64_t fit = workspace_bytes / (elems * 4);  // (the caller sized the workspace for the tile kernel's split)
  if (slabs > fit) slabs = fit;
  if (slabs < 1) return false;
  g.family = GEMM_NT;
  g.first = 0;
  g.count = n;
  g.slabs = (int)slabs;
  g.tiles = tiles;
  g.grid = (uint32_t)(tiles * slabs);
  g.ntd = env.nt_mode == 3;  // (dC fragments straight from global memory -- measured 19-21 % slower)
  // (one per CU: 20 KiB of unused dynamic LDS on top of the 64 KiB make a second workgroup not fit)
  g.dyn_lds = (env.nt_per_cu == 1 && !g.ntd) ? 20480 : 0;
  return true;
}

// ---- the tile kernels: gemm_pipe_kernel (LDS-DMA) and the register-staged gemm_kernel ----
// Tile width and arithmetic of one grouped launch.  Measured on MI355X at M = 65536 with gemm_pipe_kernel
// (tools/gsweep.sh, us):
//                                  fp32 MFMA 128x64 | 128x128     three planes 128x64 | 128x128
//   L1 4x(240->256)+2x(240->64)  fwd 346|345 wgrad 618|400 dgrad 384|330     fwd 295|262 wgrad 488|286 dgrad 304|241
//   L2 4x(256->128)              fwd 179|152 wgrad 267|201 dgrad 228|234     fwd 145|113 wgrad 209|154 dgrad 202|197
//   towers 2x(128->64)           fwd  40| 46 wgrad  93| 70 dgrad  44| 34     fwd  32| 36 wgrad  75| 59 dgrad  34| 27
// 128x128 tiles run two workgroups per CU (<= 256 VGPRs), 128x64 three.
inline void pick_tiles(const int32_t* Ns, int n, int64_t row_tiles, const GemmEnv& env, int& bn, int& emu) {
#ifdef MML_LAB  // ablation builds (tools/lab): one tile width / arithmetic only
  bn = MML_LAB_BN;
  emu = MML_LAB_EMU;
  return;
#endif
  int64_t pad64 = 0, pad128 = 0;
  for (int i = 0; i < n; ++i) {
    pad64 += route_cdiv(Ns[i], 64) * 64;
    pad128 += route_cdiv(Ns[i], 128) * 128;
  }
  bn = (pad128 * 100 <= pad64 * 150) ? 128 : 64;  // wide tiles unless > 1/3 of their columns would be padding
  if (row_tiles * (pad128 / 128) < 1024) bn = 64;  // ... or they would not fill the 512 resident slots twice
  if (env.force_bn == 64 || env.force_bn == 128) bn = env.force_bn;
  emu = (env.mode == 0) ? 0 : (env.mode == 1 ? 1 : 3);  // (3 becomes 2 in plan_tiles when the magnitudes are there)
}

// eligibility of a whole launch for the direct-to-LDS path
inline bool pipe_ok(const GemmLaunch& g, const GemmEnv& env) {
  if (!env.glds_on) return false;
  for (int i = 0; i < g.count; ++i) {
    const TileProb& P = g.p[i];
    if (!g.arc && (P.M % 4 != 0 || P.M < 4)) return false;
    if (!g.brc && (P.N % 4 != 0 || P.N < 4)) return false;
    if (P.M < 1 || P.N < 1) return false;
    for (int s = 0; s < P.nsrc; ++s) {
      const TileSrc& S = g.s[P.src0 + s];
      if (S.Kred % GK != 0 || S.Kred < GK || !S.vecA || !S.vecB) return false;
    }
  }
  if (g.epi == EPI_SLAB && g.chunk % GK != 0) return false;
  return true;
}

// what a run's operands allow, gathered while its descriptors are walked
struct TileRun {
  bool amax_all;    // every source comes with both magnitudes: the two-plane fp16 arithmetic
  bool planes_all;  // every source has a 16-byte aligned pre-cut image, one exponent word per problem
  bool any_k7;      // PepNet gate products in the epilogue
};

// Everything launch_tiles used to decide: g comes with arc, brc, epi, bcols, bn, the first arithmetic (pick_tiles) and
// the shapes; nblocks = the tiles of the launch.  1: nothing to launch, 0: planned, < 0: refused.
inline int plan_tiles(GemmLaunch& g, const TileRun& r, int64_t nblocks, const GemmEnv& env, int cus, const char* who,
                      GemmRefusal& why) {
  if (nblocks <= 0) return 1;
  if (nblocks > 0x7fffffff) {
    refuse(why, MML_ERR_ARG) << who << ": grid too large";
    return MML_ERR_ARG;
  }
  // 0 = fp32 MFMA, 1 = bf16 operands, 2 = two scaled fp16 planes, 3 = three bf16 planes
  if (g.emu == 3 && env.mode != 3 && r.amax_all) g.emu = 2;
  const bool pipe = pipe_ok(g, env);
  g.bpl = g.epi != EPI_SLAB && g.emu == 2 && pipe && env.planes_on != 0 && r.planes_all;
  g.k7 = r.any_k7;
  // The weight-gradient GEMMs run on a side stream next to the HBM-bound table optimizer (trainer.py).  An unused
  // dynamic-LDS request (mml_gemm_set_wgrad_lds_pad) lowers their residency so that the optimizer's waves co-reside.
  g.dyn_lds = g.epi == EPI_SLAB ? env.wgrad_pad : 0;
  g.grid = (uint32_t)nblocks;
  if (!pipe) {
#ifdef MML_LAB
    refuse(why, MML_ERR_UNSUPPORTED) << who << ": lab build has only the direct-to-LDS kernel";
    return MML_ERR_UNSUPPORTED;
#endif
    // shapes the LDS-DMA path cannot take (reduction extents not a multiple of 16, unaligned operands): register-staged
    // fp32 MFMA kernel
    g.family = GEMM_REG;
    g.emu = 0;
    gemm_symbol(g);
    return 0;
  }
  g.family = GEMM_PIPE;
  // persistent workgroups: one per resident slot (128 x 128 tiles: 2 per CU; 128 x 64: 3), each loops over tiles
  const int64_t slots = (int64_t)cus * ((g.bn == 64 && g.epi != EPI_DGRAD && !g.k7) ? 3 : 2);
  if (nblocks > slots) g.grid = (uint32_t)slots;
#ifndef MML_LAB
  if (g.k7) {
    // nn.Linear weights [N, K] only; gate mode on 128 x 64 tiles only: h, g and both gradients of a 128-wide tile do not
    // fit the registers next to the accumulators (route_dgrad picks the narrow tiles for it)
    if (g.epi == EPI_SLAB || (g.epi == EPI_FWD) != g.brc || (g.epi == EPI_DGRAD && g.bn != 64)) {
      refuse(why, MML_ERR_UNSUPPORTED) << who << ": the K7 products need nn.Linear weights ([N, K])";
      return MML_ERR_UNSUPPORTED;
    }
    if (g.emu != 2 && g.emu != 3) {  // (the two-plane and three-plane forms only: what the engine runs)
      refuse(why, MML_ERR_UNSUPPORTED) << who << ": the K7 products run on the plane-emulated GEMM forms only";
      return MML_ERR_UNSUPPORTED;
    }
  }
#endif
  gemm_symbol(g);
  return 0;
}

// tiles of the run's problems at width g.bn, one after the other
inline int tile_columns(GemmLaunch& g) {
  int t = 0;
  for (int k = 0; k < g.count; ++k) {
    g.p[k].tiles_n = (int)route_cdiv(g.p[k].N, g.bn);
    g.p[k].tile0 = t;
    t += g.p[k].tiles_n;
  }
  return g.total_ntiles = t;
}

// Split of a weight-gradient group d[i .. j) over the batch: S chunks of `chunk` rows, one partial tile set each.
inline void plan_wgrad(const mml_gemm_wgrad_desc* d, int i, int j, const GemmEnv& env, GemmLaunch& w) {
  int32_t cols[MML_MAX_GROUP];
  int64_t rt = 0;
  for (int k = i; k < j; ++k) {
    cols[k - i] = d[k].w_kn ? d[k].N : d[k].K;
    const int64_t r = route_cdiv(d[k].w_kn ? d[k].K : d[k].N, BM);
    rt = r > rt ? r : rt;
  }
  pick_tiles(cols, j - i, rt * route_cdiv(d[i].M, 8 * BK), env, w.bn, w.emu);
  int64_t tiles = 0, out_elems = 0, bias_elems = 0;
  for (int k = i; k < j; ++k) {
    const int rows = d[k].w_kn ? d[k].K : d[k].N, cls = d[k].w_kn ? d[k].N : d[k].K;
    tiles += route_cdiv(rows, BM) * route_cdiv(cls, w.bn);
    out_elems += (int64_t)d[k].N * d[k].K;
    if (d[k].dbias) bias_elems += d[k].N;
  }
  const int64_t M = d[i].M;
  int64_t S = tiles > 0 ? (w.bn == 128 ? 512 : 768) / tiles : 1;  // one batch chunk per resident (persistent) workgroup
  const int64_t maxS = route_cdiv(M, 8 * BK);                     // at least 256 batch rows per split
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  int64_t chunk = route_cdiv(route_cdiv(M, S), BK) * BK;
  if (chunk < BK) chunk = BK;
  S = route_cdiv(M, chunk);
  if (S < 1) S = 1;
  w.S = (int)S;
  w.chunk = (int)chunk;
  w.slab_floats = S * (out_elems + bias_elems);  // all problems, all splits, incl. bias slabs
}
// the runs a weight-gradient call is cut into: <= MML_MAX_GROUP problems of one batch size and weight layout
inline int wgrad_run_end(const mml_gemm_wgrad_desc* d, int n, int i) {
  int j = i;
  while (j < n && j - i < MML_MAX_GROUP && d[j].M == d[i].M && d[j].w_kn == d[i].w_kn) ++j;
  return j;
}
inline int64_t wgrad_workspace_bytes(const mml_gemm_wgrad_desc* d, int n, const GemmEnv& env) {
  if (n <= 0 || !d) return 0;
  int64_t best = 0;
  for (int i = 0; i < n;) {
    const int j = wgrad_run_end(d, n, i);
    GemmLaunch w{};
    plan_wgrad(d, i, j, env, w);
    best += ((w.slab_floats * 4 + 255) / 256) * 256;  // groups are laid out one after another (phased launches)
    i = j;
  }
  return best + 256;
}

#define MML_ROUTE_REQUIRE(cond, text)      \
  do {                                     \
    if (!(cond)) {                         \
      refuse(why, MML_ERR_ARG) << text;    \
      return MML_ERR_ARG;                  \
    }                                      \
  } while (0)

// ---- the three routes ----
// emit(launch, descriptors) is called once per launch, in order; a non-zero return ends the call with that code.  Returns
// MML_OK, emit's code, or the rule's own refusal (then why.code is set and why.msg holds the text).  A call that is cut
// into several launches may have emitted some before a later descriptor is refused.

// (the tile kernels' part of a forward call, which serves rows [row0, row0 + M) of the call's batch)
template <class Emit>
inline int route_fwd_tiles(const mml_gemm_fwd_desc* d, int n, int32_t row0, const GemmEnv& env, int cus, GemmRefusal& why,
                           Emit&& emit) {
  // runs of <= MML_MAX_GROUP problems with one batch size and weight layout
  int i = 0;
  while (i < n) {
    int j = i;
    int32_t Ns[MML_MAX_GROUP];
    GemmLaunch g{};
    TileRun r = {true, true, false};
    while (j < n && j - i < MML_MAX_GROUP && d[j].w_kn == d[i].w_kn && d[j].M == d[i].M) {
      const mml_gemm_fwd_desc& q = d[j];
      MML_ROUTE_REQUIRE(q.A && q.W && q.C, "mml_gemm_grouped_fwd: null pointer in problem " << j);
      MML_ROUTE_REQUIRE(q.M >= 0 && q.N > 0 && q.K > 0, "mml_gemm_grouped_fwd: bad sizes in problem " << j);
      MML_ROUTE_REQUIRE(q.lda >= q.K && q.ldc >= q.N && q.ldw >= (q.w_kn ? q.N : q.K),
                        "mml_gemm_grouped_fwd: leading dimension too small in problem " << j);
      TileProb& P = g.p[j - i];
      P.nsrc = 1;
      P.src0 = j - i;
      P.M = q.M;
      P.N = q.N;
      TileSrc& S = g.s[j - i];
      S.Kred = q.K;
      S.vecA = route_vec_ok(q.A, q.lda);
      S.vecB = route_vec_ok(q.W, q.ldw);
      r.amax_all = r.amax_all && q.amax_a && q.amax_w;
      r.planes_all = r.planes_all && q.w_planes && q.w_kexp && route_al16(q.w_planes);
      MML_ROUTE_REQUIRE(!q.relu_mask || q.ldmask * 32 >= q.N, "mml_gemm_grouped_fwd: ldmask too small in problem " << j);
      P.vec_out = (route_vec_ok(q.C, q.ldc) && q.N % 4 == 0 && (!q.bias || route_al16(q.bias))) ? 1 : 0;
      if (q.mul || q.prod) {  // K7: prod = C * mul from the same epilogue
        MML_ROUTE_REQUIRE(q.mul && q.prod && q.ldmul >= q.N && q.ldprod >= q.N,
                          "mml_gemm_grouped_fwd: problem " << j << " needs both mul and prod, with pitches >= N");
        MML_ROUTE_REQUIRE(P.vec_out && route_vec_ok(q.mul, q.ldmul) && route_vec_ok(q.prod, q.ldprod),
                          "mml_gemm_grouped_fwd: mul / prod of problem "
                              << j << " need 16-byte aligned operands and N % 4 == 0");
        r.any_k7 = true;
      }
      Ns[j - i] = q.N;
      ++j;
    }
    g.first = i;
    g.count = j - i;
    g.row0 = row0;
    g.arc = true;
    g.brc = d[i].w_kn == 0;
    g.epi = EPI_FWD;
    g.tiles_m = (int)route_cdiv(d[i].M, BM);
    pick_tiles(Ns, g.count, g.tiles_m, env, g.bn, g.emu);
    const int t = tile_columns(g);
    if (r.any_k7 && !pipe_ok(g, env)) {
      refuse(why, MML_ERR_UNSUPPORTED)
          << "mml_gemm_grouped_fwd: mul / prod need the LDS-DMA kernel (K % 16 == 0, 16-byte aligned operands)";
      return MML_ERR_UNSUPPORTED;
    }
    int rc = plan_tiles(g, r, (int64_t)g.tiles_m * t, env, cus, "mml_gemm_grouped_fwd", why);
    if (rc < 0) return rc;
    if (rc == 0 && (rc = emit(g, d)) != MML_OK) return rc;
    i = j;
  }
  return MML_OK;
}

template <class Emit>
inline int route_fwd(const mml_gemm_fwd_desc* d, int n, const GemmEnv& env, int cus, GemmRefusal& why, Emit&& emit) {
  why.code = 0;
  why.msg[0] = 0;
  if (n > 0 && planes_kernels_on(env)) {
    bool store_masks = false;
    const int32_t rows = panel_rows(d, n, env, store_masks);
    if (rows) {
      GemmLaunch g{};
      g.family = GEMM_PANEL;
      g.count = n;
      g.rows = rows;
      g.masks = store_masks;
      const int64_t npanels = rows / PN_BM;
      g.grid = (uint32_t)(npanels < cus ? npanels : cus);
      gemm_symbol(g);
      const int rc = emit(g, d);
      if (rc != MML_OK || rows == d[0].M) return rc;
      mml_gemm_fwd_desc tail[MML_MAX_GROUP];  // the last M % 128 rows: too few for panel or ws, the tile kernel
      for (int i = 0; i < n; ++i) {
        tail[i] = d[i];
        tail[i].M = d[i].M - rows;
        tail[i].A = d[i].A + (int64_t)rows * d[i].lda;
        tail[i].C = d[i].C + (int64_t)rows * d[i].ldc;
        if (d[i].relu_mask) tail[i].relu_mask = d[i].relu_mask + (int64_t)rows * d[i].ldmask;
      }
      return route_fwd_tiles(tail, n, rows, env, cus, why, emit);
    }
    if (ws_fwd_serves(d, n, env, cus))
      return ws_classes(
          n, EPI_FWD, cus,
          [&](int i, int& nout, bool& masks, bool& k7, int& dgroup) {
            nout = d[i].N;
            masks = d[i].act == MML_ACT_RELU && d[i].relu_mask != nullptr;
            k7 = d[i].mul != nullptr;
            dgroup = ws_dgroup(d[i].K);
          },
          [&](GemmLaunch& g) { return emit(g, d); });
  }
  return route_fwd_tiles(d, n, 0, env, cus, why, emit);
}

template <class Emit>
inline int route_dgrad(const mml_gemm_dgrad_desc* d, int n, const GemmEnv& env, int cus, GemmRefusal& why, Emit&& emit) {
  why.code = 0;
  why.msg[0] = 0;
  if (n > 0 && planes_kernels_on(env)) {
    if (os_serves(d, n, env)) {
      GemmLaunch g{};
      g.family = GEMM_OS;
      g.count = 1;
      const int64_t npanels = route_cdiv(d[0].M, OS_BM);
      g.grid = (uint32_t)(npanels < cus ? npanels : cus);
      gemm_symbol(g);
      return emit(g, d);
    }
    if (ws_dgrad_serves(d, n, env, cus))
      return ws_classes(
          n, EPI_DGRAD, cus,
          [&](int i, int& nout, bool& masks, bool& k7, int& dgroup) {
            nout = d[i].K;
            masks = d[i].act == MML_ACT_RELU && d[i].relu_mask != nullptr;
            k7 = d[i].gate_h != nullptr;
            dgroup = ws_dgroup(d[i].N[0]);
          },
          [&](GemmLaunch& g) { return emit(g, d); });
  }
  // runs of <= MML_MAX_GROUP problems (<= MAX_SOURCES sources) with one batch size and weight layout
  int i = 0;
  while (i < n) {
    int j = i;
    int32_t Ns[MML_MAX_GROUP];
    GemmLaunch g{};
    TileRun r = {true, true, false};
    const int32_t lay = d[i].n_src > 0 ? d[i].w_kn[0] : 0;
    int nsources = 0;
    while (j < n && j - i < MML_MAX_GROUP && d[j].M == d[i].M) {
      const mml_gemm_dgrad_desc& q = d[j];
      MML_ROUTE_REQUIRE((q.dA || q.gate_h) && q.n_src >= 1 && q.n_src <= MML_MAX_SRC,
                        "mml_gemm_grouped_dgrad: problem " << j << " malformed");
      MML_ROUTE_REQUIRE(q.M >= 0 && q.K > 0 && q.ldda >= q.K, "mml_gemm_grouped_dgrad: bad sizes in problem " << j);
      MML_ROUTE_REQUIRE(q.act == MML_ACT_NONE || q.Y || q.relu_mask,
                        "mml_gemm_grouped_dgrad: act set but Y null in problem " << j);
      bool same = true;
      for (int s = 0; s < q.n_src; ++s) same = same && (q.w_kn[s] == lay);
      if ((!same || nsources + q.n_src > MAX_SOURCES) && j > i) break;
      MML_ROUTE_REQUIRE(same, "mml_gemm_grouped_dgrad: mixed weight layouts inside problem " << j);
      TileProb& P = g.p[j - i];
      P.nsrc = q.n_src;
      P.src0 = nsources;
      for (int s = 0; s < q.n_src; ++s) {
        MML_ROUTE_REQUIRE(q.dC[s] && q.W[s] && q.N[s] > 0,
                          "mml_gemm_grouped_dgrad: null source " << s << " in problem " << j);
        TileSrc& S = g.s[nsources++];
        S.Kred = q.N[s];
        S.vecA = route_vec_ok(q.dC[s], q.lddc[s]);
        S.vecB = route_vec_ok(q.W[s], q.ldw[s]);
        r.amax_all = r.amax_all && q.amax_dc[s] && q.amax_w[s];
        // (one exponent per problem: the kernel reads the first source's)
        r.planes_all = r.planes_all && q.w_planes[s] && q.w_kexp[s] && route_al16(q.w_planes[s]) &&
                       q.w_kexp[s] == q.w_kexp[0];
      }
      P.M = q.M;
      P.N = q.K;
      MML_ROUTE_REQUIRE(!q.relu_mask || (q.act == MML_ACT_RELU && q.ldmask * 32 >= q.K),
                        "mml_gemm_grouped_dgrad: relu_mask needs act == RELU and ldmask >= K/32 (problem " << j << ")");
      P.vec_out = (route_vec_ok(q.dA, q.ldda) && q.K % 4 == 0 && (!q.Y || route_vec_ok(q.Y, q.ldy))) ? 1 : 0;
      if (q.gate_h) {  // K7 backward: the gradients of the two factors of the gated input
        MML_ROUTE_REQUIRE(
            q.gate_g && q.d_h && q.d_g && q.ld_h >= q.K && q.ld_g >= q.K && q.ld_dh >= q.K && q.ld_dg >= q.K,
            "mml_gemm_grouped_dgrad: gate mode of problem " << j << " needs gate_g, d_h, d_g and pitches >= K");
        MML_ROUTE_REQUIRE(q.K % 4 == 0 && route_vec_ok(q.gate_h, q.ld_h) && route_vec_ok(q.gate_g, q.ld_g) &&
                              route_vec_ok(q.d_h, q.ld_dh) && route_vec_ok(q.d_g, q.ld_dg),
                          "mml_gemm_grouped_dgrad: gate mode of problem "
                              << j << " needs 16-byte aligned operands and K % 4 == 0");
        P.vec_out = 1;
        r.any_k7 = true;
      } else {
        MML_ROUTE_REQUIRE(q.dA, "mml_gemm_grouped_dgrad: problem " << j << " has no dA");
      }
      Ns[j - i] = q.K;
      ++j;
    }
    g.first = i;
    g.count = j - i;
    g.arc = true;
    g.brc = lay == 1;  // col operand = W: reduction index is W's row for [N,K] (not contiguous), contiguous for [K,N]
    g.epi = EPI_DGRAD;
    g.tiles_m = (int)route_cdiv(d[i].M, BM);
    pick_tiles(Ns, g.count, g.tiles_m, env, g.bn, g.emu);
    if (r.any_k7) g.bn = 64;  // (gate mode: see plan_tiles)
    const int t = tile_columns(g);
    if (r.any_k7 && !pipe_ok(g, env)) {
      refuse(why, MML_ERR_UNSUPPORTED)
          << "mml_gemm_grouped_dgrad: gate mode needs the LDS-DMA kernel (N_s % 16 == 0, 16-byte aligned operands)";
      return MML_ERR_UNSUPPORTED;
    }
    int rc = plan_tiles(g, r, (int64_t)g.tiles_m * t, env, cus, "mml_gemm_grouped_dgrad", why);
    if (rc < 0) return rc;
    if (rc == 0 && (rc = emit(g, d)) != MML_OK) return rc;
    i = j;
  }
  return MML_OK;
}

// phase: 1 = partial tiles, 2 = their reduction, 0 = both.  Every group is emitted in every phase (the reduction needs
// its plan too); g.partials says whether the GEMM kernel itself is launched.  n >= 1, the workspace checked by the caller.
template <class Emit>
inline int route_wgrad(const mml_gemm_wgrad_desc* d, int n, int64_t workspace_bytes, int phase, const GemmEnv& env, int cus,
                       GemmRefusal& why, Emit&& emit) {
  why.code = 0;
  why.msg[0] = 0;
  if (planes_kernels_on(env)) {
    GemmLaunch g{};
    if (nt_serves(d, n, workspace_bytes, env, cus, g)) {
      g.partials = phase != 2;
      g.reduce = phase != 1;
      gemm_symbol(g);
      return emit(g, d);
    }
  }
  int64_t ws_off = 0;  // bytes: every group of problems owns its own piece of the workspace
  for (int i = 0; i < n;) {
    const int j = wgrad_run_end(d, n, i);
    GemmLaunch g{};
    TileRun r = {true, false, false};
    plan_wgrad(d, i, j, env, g);
    MML_ROUTE_REQUIRE(ws_off + g.slab_floats * 4 <= workspace_bytes,
                      "mml_gemm_grouped_wgrad: workspace " << (long long)workspace_bytes << " < "
                                                           << (long long)(ws_off + g.slab_floats * 4) << " bytes");
    g.first = i;
    g.count = j - i;
    g.ws_off = ws_off;
    ws_off += ((g.slab_floats * 4 + 255) / 256) * 256;
    int t = 0;
    for (int k = i; k < j; ++k) {
      const mml_gemm_wgrad_desc& q = d[k];
      MML_ROUTE_REQUIRE(q.dC && q.A && q.dW, "mml_gemm_grouped_wgrad: null pointer in problem " << k);
      MML_ROUTE_REQUIRE(q.M >= 0 && q.N > 0 && q.K > 0, "mml_gemm_grouped_wgrad: bad sizes in problem " << k);
      MML_ROUTE_REQUIRE(q.lddc >= q.N && q.lda >= q.K && q.lddw >= (q.w_kn ? q.N : q.K),
                        "mml_gemm_grouped_wgrad: leading dimension too small in problem " << k);
      TileProb& P = g.p[k - i];
      P.nsrc = 1;
      P.src0 = k - i;
      TileSrc& S = g.s[k - i];
      // rows of the output tile come from dC^T (n) unless the weight is stored [K,N]; both operands are batch-major in
      // memory, i.e. NOT reduction-contiguous.
      P.M = q.w_kn ? q.K : q.N;
      P.N = q.w_kn ? q.N : q.K;
      S.Kred = q.M;
      S.vecA = q.w_kn ? route_vec_ok(q.A, q.lda) : route_vec_ok(q.dC, q.lddc);
      S.vecB = q.w_kn ? route_vec_ok(q.dC, q.lddc) : route_vec_ok(q.A, q.lda);
      r.amax_all = r.amax_all && q.amax_dc && q.amax_a;
      P.tiles_m = (int)route_cdiv(P.M, BM);
      P.tiles_n = (int)route_cdiv(P.N, g.bn);
      P.tile0 = t;
      t += P.tiles_m * P.tiles_n;
    }
    g.total_ntiles = t;
    g.arc = g.brc = false;
    g.epi = EPI_SLAB;
    g.bcols = d[i].w_kn != 0;  // bias partials are sums of the column operand (uniform per run)
    g.reduce = phase != 1;
    g.family = GEMM_PIPE;  // (a reduction alone, phase 2, launches neither tile kernel)
    if (phase != 2) {
      const int rc = plan_tiles(g, r, (int64_t)t * g.S, env, cus, "mml_gemm_grouped_wgrad", why);
      if (rc < 0) return rc;
      g.partials = rc == 0;
    }
    const int rc = emit(g, d);
    if (rc != MML_OK) return rc;
    i = j;
  }
  return MML_OK;
}

}  // namespace mml
