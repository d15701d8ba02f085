// K8 optimizers (torch.optim.{SGD,Adam,Adagrad,RMSprop} with their defaults, as built by
// BaseModel._get_optim, model/basemodel.py:569-584, and stepped at :313).
// All of these are pure streaming kernels: 16-byte accesses per lane, grid-stride, HBM-bound.
#include "common.hpp"
#include "fold_fixed.hpp"
#include "opt_plan.hpp"

#include <stdlib.h>

#include <mutex>
#include <vector>

// chunks whose mark / warm bytes a thread of the mostly-cold table stream reads before it looks at any of them (lab builds:
// -DMML_OPT_COLD_CB=2 / 4 / 16, tools/lab/opt_cold_rows.py; DESIGN_HISTORY.md has the numbers)
#ifndef MML_OPT_COLD_CB
#define MML_OPT_COLD_CB 8
#endif

namespace mml {

struct OptLaunch {
  mml_opt_tensor t[MML_MAX_OPT_TENSORS];
  int32_t n;
  int32_t variant;  // streaming form of the vector loop (tuning knob MMLREC_OPT_VARIANT): bit 0 = nontemporal, bit 1 = 2x unroll; bit 2 = capped grid (4 chunks in flight per thread); bit 3 = mml_opt_hyper.cold_loop is 1 (the byte-walking loop over a warm map)
  mml_opt_hyper h;
  int64_t chunk0[MML_MAX_OPT_TENSORS + 1];  // flat kernel: first 4-element chunk of tensor i in the concatenation
  // streaming kernel over MANY tensors (round 6: every table of the model in one marked launch): a 1-D grid whose
  // workgroups are dealt to the tensors in proportion to their sizes; blk0[i] = first workgroup of tensor i (prop != 0)
  int32_t blk0[MML_MAX_OPT_TENSORS + 1];
  // 2: one grid over the 256-row spans of ALL tensors (cold_resident); blk0[i] = first span of tensor i instead
  int32_t prop;
  // the step's constants where mml_opt_step_begin keeps them for h.step_dev (null: every workgroup computes them)
  const mml_opt_step_consts* sc;
};
static_assert(sizeof(OptLaunch) <= 4096, "OptLaunch travels by value: the kernel-argument block holds 4 KB");

struct StepConsts {
  float step_size;  // Adam: lr / (1 - beta1^t)
  float inv_bc2s;   // Adam: 1 / sqrt(1 - beta2^t)
};

// The constants of step t (one copy of the expressions: the same double operations in the same order wherever they run).
__device__ __forceinline__ StepConsts step_consts_of(const mml_opt_hyper& h, int t) {
  StepConsts c{h.lr, 1.f};
  if (h.kind == MML_OPT_ADAM) {
    // torch computes the bias corrections in double precision on the host (python floats)
    const double bc1 = 1.0 - pow((double)h.beta1, (double)t);
    const double bc2 = 1.0 - pow((double)h.beta2, (double)t);
    c.step_size = (float)((double)h.lr / bc1);
    c.inv_bc2s = (float)(1.0 / sqrt(bc2));
  }
  return c;
}

// bound: the buffer mml_opt_step_begin filled for h.step_dev with this optimizer's lr / beta1 / beta2 at the start of the
// step (the host looked the binding up) -- two uniform loads, no barrier; the buffer names the step it was computed for,
// and a counter that somebody else has moved since sends the workgroup down the path below.
// Else computed by ONE lane per workgroup (double-precision pow is hundreds of instructions) and broadcast through LDS.
__device__ __forceinline__ StepConsts step_consts(const mml_opt_hyper& h, const mml_opt_step_consts* bound = nullptr) {
  // (one exit for the bound path: with a return per case the compiler keeps the whole kernel-argument block in scratch)
  bool have = false;
  StepConsts r{h.lr, 1.f};
  if (bound) {  // (workgroup-uniform, as is what it reads)
    if (h.kind != MML_OPT_ADAM) {
      have = true;
    } else if (bound->step == *h.step_dev) {
      r.step_size = bound->step_size;
      r.inv_bc2s = bound->inv_bc2s;
      have = true;
    }
  }
  if (have) return r;
  __shared__ StepConsts sc;
  if (threadIdx.x == 0)  // (only Adam reads the step)
    sc = step_consts_of(h, h.kind != MML_OPT_ADAM ? 0 : h.step_dev ? *h.step_dev : h.step);
  __syncthreads();
  return sc;
}

// One element of torch.optim's single-tensor update (the _single_tensor_* functions with default flags).
__device__ __forceinline__ void opt_update(const mml_opt_hyper& h, const StepConsts& c, float& p, float g, float& s1,
                                           float& s2) {
  switch (h.kind) {
    case MML_OPT_SGD:
      p -= h.lr * g;
      break;
    case MML_OPT_ADAM: {
      s1 = s1 + (1.f - h.beta1) * (g - s1);               // exp_avg.lerp_(grad, 1-beta1)
      s2 = h.beta2 * s2 + (1.f - h.beta2) * g * g;        // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
      const float denom = sqrtf(s2) * c.inv_bc2s + h.eps; // (sqrt(v) / sqrt(bc2)).add_(eps)
      p -= c.step_size * (s1 / denom);                    // param.addcdiv_(exp_avg, denom, value=-step_size)
      break;
    }
    case MML_OPT_ADAGRAD:
      s1 += g * g;                                        // state_sum.addcmul_(g, g)
      p -= h.lr * (g / (sqrtf(s1) + h.eps));              // param.addcdiv_(g, sqrt(sum)+eps, value=-lr)
      break;
    case MML_OPT_RMSPROP:
      s1 = h.alpha * s1 + (1.f - h.alpha) * g * g;        // square_avg.mul_(alpha).addcmul_(g, g, 1-alpha)
      p -= h.lr * (g / (sqrtf(s1) + h.eps));
      break;
  }
}

// Gradient of the regulariser folded into the update (model/basemodel.py:524-540): d/dp [l1 |p| + l2 p^2].
__device__ __forceinline__ float reg_grad(float g, float p, float l1, float l2) {
  if (l2 != 0.f) g += (2.f * l2) * p;
  if (l1 != 0.f) g += l1 * (p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f));
  return g;
}

// ---- the wave-compacted loop over a warm map: one span of one tensor ---------------------------------------------------
// Mostly-cold stream (forms 3 and 4 of opt_dense_kernel, tensors with a warm map whose map pointers are 4-byte aligned).
// A wave owns spans of SPAN consecutive rows; lane l reads the marks and the warm bytes of rows [4 l, 4 l + 4) of the span
// with one aligned dword load each (the next span's are in flight while this one is worked on) and is the only reader and
// writer of those map bytes in the launch.  The live rows (marked or warm) are listed in the wave's LDS list -- exclusive
// prefix sum of the lanes' counts from ballots of the counts' bits, no atomics, no workgroup barrier -- and the list's
// 16-byte chunks are shared out 128 at a time, two per lane in flight, every load of a lane before its first store: a wave
// pays one round trip for the maps (hidden behind the previous span) and one per 128 live chunks, wherever in the span
// they lie.  A span with no live row costs nothing more; one with more than a few live rows skips the list (DENSE_PCT).
// (Four dwords of each map per lane, spans of 1 024 rows, lost at every warm share: DESIGN_HISTORY.md, "Cold rows".)
// Which wave takes which span is the caller's business: opt_dense_kernel deals a tensor's spans to the waves of the
// tensor's workgroups, or -- cold_resident, OptLaunch.prop = 2 -- the spans of all tensors to the waves of one grid.
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef long long vl2 __attribute__((ext_vector_type(2)));
// (COLD_RPL rows per lane -- one dword of each map -- and COLD_SPAN rows per wave trip: opt_plan.hpp, whose resident grid
// counts spans)
// Live rows, in per cent of a span, from which the span is walked row by row instead of listed.  Measured with 1, 15,
// 33, 50 and 100: listing spans that are 15-50 % live cost 8-12 us of ~500 at 60-76 % warm rows, at 15 the launch is
// level with the loop before from there on and keeps the list's whole gain below (DESIGN_HISTORY.md).
constexpr int COLD_DENSE_PCT = 15;
constexpr int COLD_WAVES = 4;  // per workgroup: every launch of these kernels has 256 threads (__launch_bounds__(256))

struct ColdTensor {  // what the loop needs of one tensor (wave-uniform)
  vf4 *P, *G, *S1, *S2;
  vl2* A64;  // the deferred totals (form 4), or null
  uint8_t *gm, *wr;
  int64_t rows;
  int csh;   // log2(chunks per row): row_elems / 4 is a power of two (mml_opt_step_dense checks)
  int emax, acc_shift;
  bool zg;
};

template <int WITH_ACC>
__device__ __forceinline__ ColdTensor cold_tensor(const mml_opt_tensor& T) {
  ColdTensor X;
  X.P = reinterpret_cast<vf4*>(T.param);
  X.G = reinterpret_cast<vf4*>(const_cast<float*>(T.grad));
  X.S1 = reinterpret_cast<vf4*>(T.state1);
  X.S2 = reinterpret_cast<vf4*>(T.state2);
  X.A64 = WITH_ACC ? reinterpret_cast<vl2*>(T.acc64) : nullptr;
  X.gm = T.grad_marks;
  X.wr = T.warm_rows;
  const int rsh = __builtin_ctz((unsigned)T.row_elems);
  X.rows = T.n >> rsh;
  X.csh = rsh - 2;
  X.emax = 1;
  if (WITH_ACC && X.A64) {  // the unit's exponent as scatter_det_finalize_kernel takes it
    uint32_t m = 0;
    for (int w = 0; w < MML_AMAX_WORDS; ++w) m = T.acc_amax[w] > m ? T.acc_amax[w] : m;
    X.emax = (int)(m >> 23);
    X.emax = X.emax < 1 ? 1 : (X.emax > 254 ? 254 : X.emax);
  }
  X.acc_shift = T.acc_shift;
  X.zg = T.zero_grads != 0;
  return X;
}

// the lane's map bytes of span s: the whole words where all four rows exist, else the bytes below `rows` one by one
__device__ __forceinline__ void cold_scan(const uint8_t* gm, const uint8_t* wr, int64_t rows, int64_t s, int lane,
                                          uint32_t& mk, uint32_t& wk) {
  const int64_t r0 = s * COLD_SPAN + lane * COLD_RPL;
  mk = wk = 0u;
  if (r0 + COLD_RPL <= rows) {
    mk = *reinterpret_cast<const uint32_t*>(gm + r0);
    wk = *reinterpret_cast<const uint32_t*>(wr + r0);
  } else {
#pragma unroll
    for (int k = 0; k < COLD_RPL; ++k)
      if (r0 + k < rows) {
        mk |= (uint32_t)gm[r0 + k] << (8 * k);
        wk |= (uint32_t)wr[r0 + k] << (8 * k);
      }
  }
}

// Span s of tensor X from the map dwords (mk, wk) cold_scan read for it: map upkeep and the update of its live rows.
// lst = the wave's list of COLD_SPAN entries in LDS (entry: bits 0-13 row of the span, 14 marked, 15 was warm).
template <int WITH_ACC>
__device__ __forceinline__ void cold_span(const mml_opt_hyper& h, const StepConsts& c, bool nt, const ColdTensor& X,
                                          int64_t s, int lane, uint16_t* lst, uint32_t mk, uint32_t wk) {
  constexpr int RPL = COLD_RPL, SPAN = COLD_SPAN;
  const vf4 zero = {0.f, 0.f, 0.f, 0.f};
  const vl2 lzero = {0, 0};
  // 0x80 in every byte of x that is not zero
  auto nz80 = [](uint32_t x) { return (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; };
  auto pack4 = [](uint32_t t) { return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u); };
  const uint32_t lm = pack4(nz80(mk)), wm = pack4(nz80(wk));  // bit k: row k of this lane is marked / warm
  const uint32_t act = lm | wm;
  if (__builtin_amdgcn_ballot_w64(act != 0) == 0) return;
  auto ld = [&](const vf4* q) { return nt ? __builtin_nontemporal_load(q) : *q; };
  auto st = [&](vf4* q, const vf4& v) {
    if (nt) __builtin_nontemporal_store(v, q);
    else *q = v;
  };
  const int csh = X.csh;
  const int64_t rows = X.rows, row0 = s * SPAN;
  // live rows of the span and, per lane, of the lanes below it: ballots of the bits of the lanes' counts
  const uint32_t cnt = (uint32_t)__builtin_popcount(act);
  uint32_t pre = 0;
  int nlive = 0;
#pragma unroll
  for (int bit = 0; (1 << bit) <= RPL; ++bit) {
    const uint64_t bal = __builtin_amdgcn_ballot_w64(((cnt >> bit) & 1u) != 0);
    pre += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u)) << bit;
    nlive += __builtin_popcountll(bal) << bit;
  }
  // A span with that many live rows is walked row by row without the list, dead chunks passed over (the 100 %-warm
  // stream pays no compaction)
  const bool dense = nlive * 100 >= SPAN * COLD_DENSE_PCT;
  if (!dense) {
    // (the lanes' reads of the previous span's list come before these writes, and these before the reads below:
    // the LDS serves a wave's instructions in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < RPL; ++k)
      if ((act >> k) & 1u)
        lst[pre++] = (uint16_t)((lane * RPL + k) | (((lm >> k) & 1u) << 14) | (((wm >> k) & 1u) << 15));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // map upkeep by the bytes' only reader: marks cleared, the marked rows that were cold now warm
  if (lm) {
    const int64_t r0 = row0 + lane * RPL;
    if (r0 + RPL <= rows) {
      *reinterpret_cast<uint32_t*>(X.gm + r0) = 0u;
      const uint32_t set = (nz80(mk) & ~nz80(wk)) >> 7;  // 1 in the byte of every marked row that was cold
      if (set) *reinterpret_cast<uint32_t*>(X.wr + r0) = wk | set;
    } else {
#pragma unroll
      for (int k = 0; k < RPL; ++k)
        if ((lm >> k) & 1u) {  // (only rows below `rows` were read)
          X.gm[r0 + k] = 0;
          if (!((wm >> k) & 1u)) X.wr[r0 + k] = 1;
        }
    }
  }
  const int items = (dense ? SPAN : nlive) << csh;
#pragma unroll 1
  for (int b0 = 0; b0 < items; b0 += 128) {
    vf4 p[2], a[2], b[2], g[2];
    vl2 t0[2], t1[2];
    int64_t jj[2];
    bool on[2], lv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int it = b0 + 64 * k + lane;
      const int ent = it >> csh;
      on[k] = it < items;
      uint32_t e;
      if (dense) {  // (all 256 rows in order; the live and marked bits from the lane that read the row's bytes)
        const uint32_t src = (uint32_t)__shfl((int)(lm | (act << 16)), (ent / RPL) & 63);
        on[k] = on[k] && ((src >> (16 + (ent & (RPL - 1)))) & 1u);
        e = (uint32_t)ent | (((src >> (ent & (RPL - 1))) & 1u) << 14);
      } else {
        e = on[k] ? lst[ent] : 0u;
      }
      lv[k] = on[k] && ((e >> 14) & 1u);
      const int64_t j = ((row0 + (int64_t)(e & 0x3fffu)) << csh) | (int64_t)(it & ((1 << csh) - 1));
      jj[k] = j;
      p[k] = a[k] = b[k] = g[k] = zero;
      t0[k] = t1[k] = lzero;
      if (on[k]) {
        p[k] = ld(X.P + j);
        if (X.S1) a[k] = ld(X.S1 + j);
        if (X.S2) b[k] = ld(X.S2 + j);
      }
      if (lv[k]) {
        if (!X.zg) g[k] = ld(X.G + j);
        if (WITH_ACC && X.A64) {
          t0[k] = X.A64[2 * j];
          t1[k] = X.A64[2 * j + 1];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!on[k]) continue;
      const int64_t j = jj[k];
      vf4 gs = g[k];
      if (WITH_ACC && X.A64 && lv[k]) {
        // g + from_fixed(total) for the non-zero totals (the expression of the finalize launch's dst[e] += ...), the
        // totals it used zeroed again
        const vl2 u0 = t0[k], u1 = t1[k];
        if (u0.x) gs.x += from_fixed(u0.x, X.emax, X.acc_shift);
        if (u0.y) gs.y += from_fixed(u0.y, X.emax, X.acc_shift);
        if (u1.x) gs.z += from_fixed(u1.x, X.emax, X.acc_shift);
        if (u1.y) gs.w += from_fixed(u1.y, X.emax, X.acc_shift);
        if (u0.x | u0.y) X.A64[2 * j] = lzero;
        if (u1.x | u1.y) X.A64[2 * j + 1] = lzero;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // (a tensor with a warm map carries no regulariser)
        float pe = p[k][e], ae = a[k][e], be = b[k][e];
        opt_update(h, c, pe, gs[e], ae, be);
        p[k][e] = pe;
        a[k][e] = ae;
        b[k][e] = be;
      }
      st(X.P + j, p[k]);
      if (X.S1) st(X.S1 + j, a[k]);
      if (X.S2) st(X.S2 + j, b[k]);
      if (h.zero_grad && (g[k].x != 0.f || g[k].y != 0.f || g[k].z != 0.f || g[k].w != 0.f)) X.G[j] = zero;
    }
  }
}

// One grid sized for the chip over the spans of ALL tensors of a marked launch whose tensors all take the loop above
// (L.blk0[i] = first span of tensor i): wave w of the grid's W takes spans w, w + W, w + 2 W, ... of that index space --
// strided, so that the hot head of a Zipf table is spread over all waves -- and finds (tensor, span) with scalar code;
// the tensor's values are loaded again only when the tensor changes.  The next span's map dwords are in flight while
// this one is worked on, also across a tensor change.  No workgroup waits for another.  The grid is two rounds of the
// workgroups the chip holds (mml_opt_step_dense): with one, the waves dealt the warm head finish last with nothing behind them.
template <int WITH_ACC>
__device__ __forceinline__ void cold_resident(const OptLaunch& L, const StepConsts& c, uint16_t (*live_rows)[COLD_SPAN]) {
  const mml_opt_hyper& h = L.h;
  const bool nt = (L.variant & 1) != 0;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (scalar: the span loop is wave-uniform)
  uint16_t* const lst = live_rows[wv];
  const int nspan = L.blk0[L.n], nwv = (int)gridDim.x * COLD_WAVES;
  int s = (int)blockIdx.x * COLD_WAVES + wv;
  if (s >= nspan) return;
  int ti = 0;
  while (s >= L.blk0[ti + 1]) ++ti;  // (s < blk0[n]: stops at a tensor that has spans)
  ColdTensor X = cold_tensor<WITH_ACC>(L.t[ti]);
  uint32_t mk, wk;
  cold_scan(X.gm, X.wr, X.rows, s - L.blk0[ti], lane, mk, wk);
  for (;;) {  // (wave-uniform)
    const int sn = s + nwv;
    int tn = ti;
    uint32_t mkn = 0, wkn = 0;
    if (sn < nspan) {
      while (sn >= L.blk0[tn + 1]) ++tn;
      const mml_opt_tensor& Tn = L.t[tn];
      cold_scan(Tn.grad_marks, Tn.warm_rows, Tn.n >> __builtin_ctz((unsigned)Tn.row_elems), sn - L.blk0[tn], lane, mkn,
                wkn);
    }
    cold_span<WITH_ACC>(h, c, nt, X, s - L.blk0[ti], lane, lst, mk, wk);
    if (sn >= nspan) break;
    if (tn != ti) {
      ti = tn;
      X = cold_tensor<WITH_ACC>(L.t[ti]);
    }
    s = sn;
    mk = mkn;
    wk = wkn;
  }
}

// blockIdx.y = tensor, blockIdx.x strides over that tensor in float4 chunks.
// STREAM is only ever instantiated as true: everything that does not stream >= 2^24 parameters (MLP parameters, small
// tables) goes through opt_flat_kernel.  The parameter stays because it is part of the symbol profiles and tests name.
// PATH = the form of the vector loop, one instantiation each so that each keeps ITS register count (all forms in one
// kernel: 170 VGPRs, two waves per SIMD -- and the plain loop, which needs 40, ran at that occupancy too):
//   0 plain grid-stride loop (also the remainder loop of every other form)   1 two chunks per iteration
//   2 split update, untouched rows, U chunks in flight per thread            3 marked gradients, U chunks in flight
//   4 marked gradients whose rows' 64-bit totals of the deterministic scatter are still in mml_opt_tensor.acc64 (the
//     scatter's second launch folded in): as 3, plus 32 bytes of totals read, converted and zeroed per marked chunk
// Forms 3 and 4 with a warm map (mml_opt_tensor.warm_rows, decided at run time inside the same instantiations): a row that
// is neither marked nor warm has m = v = 0 and g = 0, the update leaves p, m and v as they are bit for bit, and the kernel
// neither reads nor writes it -- it walks the two byte maps and touches the rows they name.
// (the forms' names, OPT_PLAIN .. OPT_MARK_ACC_U: opt_plan.hpp)
template <bool STREAM, int PATH, int U>
__global__ __launch_bounds__(256) void opt_dense_kernel(const OptLaunch L) {
  // (workgroup-uniform: scalar loads and compares)
  int ti = blockIdx.y, nblk = gridDim.x, lblk = blockIdx.x;
  if (L.prop == 1) {
    ti = 0;
    while (ti + 1 < L.n && (int)blockIdx.x >= L.blk0[ti + 1]) ++ti;
    nblk = L.blk0[ti + 1] - L.blk0[ti];
    lblk = (int)blockIdx.x - L.blk0[ti];
  }
  const mml_opt_tensor& T = L.t[ti];
  const mml_opt_hyper& h = L.h;
  const StepConsts c = step_consts(h, L.sc);
  // the wave-compacted loop's lists of live rows, one per wave (cold_span)
  __shared__ uint16_t live_rows[(PATH == OPT_MARK_U || PATH == OPT_MARK_ACC_U) ? COLD_WAVES : 1][COLD_SPAN];
  if ((PATH == OPT_MARK_U || PATH == OPT_MARK_ACC_U) && L.prop == 2) {  // (the launch's switch)
    cold_resident<PATH == OPT_MARK_ACC_U>(L, c, live_rows);
    return;
  }
  const int64_t n4 = T.n >> 2;
  const bool vec = aligned16(T.param) && aligned16(T.grad) && (!T.state1 || aligned16(T.state1)) &&
                   (!T.state2 || aligned16(T.state2));
  const int64_t stride = (int64_t)nblk * blockDim.x;
  const int64_t tid = (int64_t)lblk * blockDim.x + threadIdx.x;
  float* gw = const_cast<float*>(T.grad);
  const bool reg = T.l1 != 0.f || T.l2 != 0.f;
  if (vec) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const bool nt = (L.variant & 1) != 0;
    f4* P = reinterpret_cast<f4*>(T.param);
    f4* G = reinterpret_cast<f4*>(gw);
    f4* S1 = reinterpret_cast<f4*>(T.state1);
    f4* S2 = reinterpret_cast<f4*>(T.state2);
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    auto ld = [&](const f4* q) { return nt ? __builtin_nontemporal_load(q) : *q; };
    auto st = [&](f4* q, const f4& v) {
      if (nt) __builtin_nontemporal_store(v, q);
      else *q = v;
    };
    auto one = [&](f4& p, const f4& g, f4& a, f4& b) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], ae = a[e], be = b[e];
        opt_update(h, c, pe, reg ? reg_grad(g[e], pe, T.l1, T.l2) : g[e], ae, be);
        p[e] = pe;
        a[e] = ae;
        b[e] = be;
      }
    };
    const uint32_t* skip = T.skip_rows;
    const int re = T.row_elems > 0 ? T.row_elems : 1;
    // row of chunk c = elements [4c, 4c + 4) (inside ONE row when row_elems % 4 == 0): a shift for the usual power-of-two
    // embedding widths (a 64-bit division is ~100 VALU instructions per chunk, issue slots the GEMM waves beside this
    // kernel want)
    const int rsh = (re & (re - 1)) == 0 ? __builtin_ctz((unsigned)re) : -1;
    auto row_of = [&](int64_t c) { return rsh >= 0 ? ((c << 2) >> rsh) : ((c << 2) / re); };
    auto skipped = [&](int64_t c) {
      const int64_t row = row_of(c);
      return (skip[row >> 5] >> (row & 31)) & 1u;
    };
    const bool zg = T.zero_grads != 0;
    // marked gradients: a row whose byte is 0 has a zero gradient, not read.  The chunks of a row sit in adjacent lanes
    // of ONE wave (row_elems / 4 is a power of two <= 64, chunk index = lane + multiple of 64): every lane of the row
    // reads the byte in the same wave-instruction, before the first chunk's lane clears it further down.
    uint8_t* const gm = T.grad_marks;
    // deferred totals (PATH 4 only; a tensor of the launch without them is a plain marked tensor): chunk c of the table
    // = totals [4c, 4c + 4) = two 16-byte pieces; the unit's exponent as scatter_det_finalize_kernel takes it
    typedef long long l2 __attribute__((ext_vector_type(2)));
    l2* const A64 = PATH == OPT_MARK_ACC_U ? reinterpret_cast<l2*>(T.acc64) : nullptr;
    const l2 lzero = {0, 0};
    int emax = 1;
    if (PATH == OPT_MARK_ACC_U && A64) {
      uint32_t m = 0;
      for (int w = 0; w < MML_AMAX_WORDS; ++w) m = T.acc_amax[w] > m ? T.acc_amax[w] : m;
      emax = (int)(m >> 23);
      emax = emax < 1 ? 1 : (emax > 254 ? 254 : emax);
    }
    // g + from_fixed(total) for the non-zero totals (the expression of the finalize launch's dst[e] += ...), the totals
    // it used zeroed again
    auto add_totals = [&](f4& g, const l2& t0, const l2& t1, int64_t c) {
      if (t0.x) g.x += from_fixed(t0.x, emax, T.acc_shift);
      if (t0.y) g.y += from_fixed(t0.y, emax, T.acc_shift);
      if (t1.x) g.z += from_fixed(t1.x, emax, T.acc_shift);
      if (t1.y) g.w += from_fixed(t1.y, emax, T.acc_shift);
      if (t0.x | t0.y) A64[2 * c] = lzero;
      if (t1.x | t1.y) A64[2 * c + 1] = lzero;
    };
    int64_t i = tid;
    if (PATH == OPT_UNROLL2 && !skip && !gm) {
      for (; i + stride < n4; i += 2 * stride) {  // eight 16-byte loads in flight per thread
        const int64_t j = i + stride;
        f4 p0 = ld(P + i), p1 = ld(P + j);
        const f4 g0 = ld(G + i), g1 = ld(G + j);
        f4 a0 = S1 ? ld(S1 + i) : zero, a1 = S1 ? ld(S1 + j) : zero;
        f4 b0 = S2 ? ld(S2 + i) : zero, b1 = S2 ? ld(S2 + j) : zero;
        one(p0, g0, a0, b0);
        one(p1, g1, a1, b1);
        st(P + i, p0);
        st(P + j, p1);
        if (S1) { st(S1 + i, a0); st(S1 + j, a1); }
        if (S2) { st(S2 + i, b0); st(S2 + j, b1); }
        if (h.zero_grad && (g0.x != 0.f || g0.y != 0.f || g0.z != 0.f || g0.w != 0.f)) G[i] = zero;
        if (h.zero_grad && (g1.x != 0.f || g1.y != 0.f || g1.z != 0.f || g1.w != 0.f)) G[j] = zero;
      }
    }
    if (PATH == OPT_SKIP_U && skip) {
      // early half of the split table update under a capped grid (mml_opt_hyper.max_blocks): it runs BESIDE other
      // kernels with few waves, so the memory-level parallelism has to come from the thread: U independent chunks (3U
      // 16-byte loads) in flight.  (With the full grid the plain loop below is faster: fewer registers, more waves.)
      for (; i + (U - 1) * stride < n4; i += U * stride) {
        f4 p[U], a[U], b[U];
        uint32_t w[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {  // the U bitmap words first ...
          const int64_t row = row_of(i + k * stride);
          w[k] = (skip[row >> 5] >> (row & 31)) & 1u;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {  // ... then every load of the live chunks
          const int64_t j = i + k * stride;
          if (!w[k]) {
            p[k] = ld(P + j);
            a[k] = S1 ? ld(S1 + j) : zero;
            b[k] = S2 ? ld(S2 + j) : zero;
          }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          if (w[k]) continue;
          const int64_t j = i + k * stride;
          const f4 g = zg ? zero : ld(G + j);
          one(p[k], g, a[k], b[k]);
          st(P + j, p[k]);
          if (S1) st(S1 + j, a[k]);
          if (S2) st(S2 + j, b[k]);
          if (h.zero_grad && (g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f)) G[j] = zero;
        }
      }
    }
    // warm map (forms 3 and 4, and the remainder loop of every form): 0 = the row's moments are still zero.  Read like
    // the mark: by every lane of the row in one wave-instruction, before the first chunk's lane sets it.
    uint8_t* const wr = gm ? T.warm_rows : nullptr;
    // (workgroup-uniform: the launch's switch and this tensor's map pointers)
    const bool compact = !(L.variant & 8) && wr &&
                         ((reinterpret_cast<uintptr_t>(gm) | reinterpret_cast<uintptr_t>(wr)) & 3) == 0;
    if ((PATH == OPT_MARK_U || PATH == OPT_MARK_ACC_U) && compact && !skip) {
      // The wave-compacted loop (cold_span, above) on this tensor's own workgroups: its spans are dealt to their waves by the
      // wave's number among them.  (The grid of a launch some tensor of which does not qualify for cold_resident, and
      // the A/B arm mml_opt_hyper.cold_loop = 2.)
      const int lane = threadIdx.x & 63;
      const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (scalar: the span loop is wave-uniform)
      const ColdTensor X = cold_tensor<PATH == OPT_MARK_ACC_U>(T);
      const int64_t nspan = (X.rows + COLD_SPAN - 1) / COLD_SPAN, nwv = (int64_t)nblk * COLD_WAVES;
      int64_t s = (int64_t)lblk * COLD_WAVES + wv;
      uint32_t mk = 0, wk = 0;
      if (s < nspan) cold_scan(gm, wr, X.rows, s, lane, mk, wk);
      for (; s < nspan; s += nwv) {  // (wave-uniform)
        uint32_t mkn = 0, wkn = 0;
        if (s + nwv < nspan) cold_scan(gm, wr, X.rows, s + nwv, lane, mkn, wkn);
        cold_span<PATH == OPT_MARK_ACC_U>(h, c, nt, X, s, lane, live_rows[wv], mk, wk);
        mk = mkn;
        wk = wkn;
      }
      i = n4;  // (every chunk of the tensor is done: the loops below find nothing left)
    }
    if ((PATH == OPT_MARK_U || PATH == OPT_MARK_ACC_U) && wr && !skip && !compact) {  // (workgroup-uniform)
      // The loop before the compacted one (mml_opt_hyper.cold_loop = 1, or map pointers that are not aligned for the word
      // loads).  Mostly-cold stream: the bytes of CB chunks' rows (2 CB one-byte loads in flight, no load depends on another), then
      // only the live chunks, two at a time as in the forms below; a wave none of whose lanes has a live chunk moves on
      // without a further memory access.  The block covers its own remainder (chunks past the end are not live).
      constexpr int CB = MML_OPT_COLD_CB;
      for (; i < n4; i += CB * stride) {
        uint32_t lm = 0, wm = 0;  // bit k: chunk i + k * stride is marked / warm
#pragma unroll
        for (int k = 0; k < CB; ++k) {
          const int64_t j = i + k * stride;
          const bool in = j < n4;
          const int64_t row = row_of(in ? j : i);  // (a valid address either way: no branch around the loads)
          const uint8_t mk = gm[row], wk = wr[row];
          lm |= (uint32_t)(in && mk != 0) << k;
          wm |= (uint32_t)(in && wk != 0) << k;
        }
        const uint32_t act = lm | wm;
        if (__builtin_amdgcn_ballot_w64(act != 0) == 0) continue;
#pragma unroll 1
        for (int kk = 0; kk < CB; kk += 2) {  // (one copy of the pair's code: unrolled, the kernel loses a wave per SIMD)
          if (__builtin_amdgcn_ballot_w64(((act >> kk) & 3u) != 0) == 0) continue;
          f4 p[2], a[2], b[2], g[2];
          l2 t0[2], t1[2];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int64_t j = i + (kk + k) * stride;
            const bool on = (act >> (kk + k)) & 1u, lv = (lm >> (kk + k)) & 1u;
            p[k] = a[k] = b[k] = g[k] = zero;
            t0[k] = t1[k] = lzero;
            if (on) {
              p[k] = ld(P + j);
              if (S1) a[k] = ld(S1 + j);
              if (S2) b[k] = ld(S2 + j);
            }
            if (lv) {
              if (!zg) g[k] = ld(G + j);
              if (PATH == OPT_MARK_ACC_U && A64) {
                t0[k] = A64[2 * j];
                t1[k] = A64[2 * j + 1];
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int64_t j = i + (kk + k) * stride;
            const bool on = (act >> (kk + k)) & 1u, lv = (lm >> (kk + k)) & 1u;
            if (!on) continue;
            f4 gs = g[k];
            if (PATH == OPT_MARK_ACC_U && A64 && lv) add_totals(gs, t0[k], t1[k], j);
            one(p[k], gs, a[k], b[k]);
            st(P + j, p[k]);
            if (S1) st(S1 + j, a[k]);
            if (S2) st(S2 + j, b[k]);
            if (h.zero_grad && (g[k].x != 0.f || g[k].y != 0.f || g[k].z != 0.f || g[k].w != 0.f)) G[j] = zero;
            const int64_t row = row_of(j);
            if (lv && (j << 2) == row * re) {
              gm[row] = 0;
              if (!((wm >> (kk + k)) & 1u)) wr[row] = 1;
            }
          }
        }
      }
    }
    if (PATH == OPT_MARK_U && gm && !skip) {
      // marked single-launch update under a capped grid (mml_opt_hyper.max_blocks: it runs beside the weight-gradient
      // GEMMs and leaves them their wave slots): the memory-level parallelism comes from the thread -- U chunks, 3U
      // 16-byte loads in flight
      for (; i + (U - 1) * stride < n4; i += U * stride) {
        f4 p[U], a[U], b[U], g[U];
        bool lv[U];
        int64_t rw[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          rw[k] = row_of(i + k * stride);
          lv[k] = gm[rw[k]] != 0;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t j = i + k * stride;
          p[k] = ld(P + j);
          a[k] = S1 ? ld(S1 + j) : zero;
          b[k] = S2 ? ld(S2 + j) : zero;
          g[k] = (zg || !lv[k]) ? zero : ld(G + j);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t j = i + k * stride;
          one(p[k], g[k], a[k], b[k]);
          st(P + j, p[k]);
          if (S1) st(S1 + j, a[k]);
          if (S2) st(S2 + j, b[k]);
          if (h.zero_grad && (g[k].x != 0.f || g[k].y != 0.f || g[k].z != 0.f || g[k].w != 0.f)) G[j] = zero;
          if (lv[k] && (j << 2) == rw[k] * re) gm[rw[k]] = 0;
        }
      }
    }
    if (PATH == OPT_MARK_ACC_U && gm && !skip) {
      // the marked form above with the totals of the live chunks in flight beside the gradient (2 more 16-byte loads)
      for (; i + (U - 1) * stride < n4; i += U * stride) {
        f4 p[U], a[U], b[U], g[U];
        l2 t0[U], t1[U];
        bool lv[U];
        int64_t rw[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          rw[k] = row_of(i + k * stride);
          lv[k] = gm[rw[k]] != 0;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t j = i + k * stride;
          p[k] = ld(P + j);
          a[k] = S1 ? ld(S1 + j) : zero;
          b[k] = S2 ? ld(S2 + j) : zero;
          g[k] = (zg || !lv[k]) ? zero : ld(G + j);
          t0[k] = (A64 && lv[k]) ? A64[2 * j] : lzero;
          t1[k] = (A64 && lv[k]) ? A64[2 * j + 1] : lzero;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t j = i + k * stride;
          f4 gs = g[k];
          if (A64 && lv[k]) add_totals(gs, t0[k], t1[k], j);
          one(p[k], gs, a[k], b[k]);
          st(P + j, p[k]);
          if (S1) st(S1 + j, a[k]);
          if (S2) st(S2 + j, b[k]);
          if (h.zero_grad && (g[k].x != 0.f || g[k].y != 0.f || g[k].z != 0.f || g[k].w != 0.f)) G[j] = zero;
          if (lv[k] && (j << 2) == rw[k] * re) gm[rw[k]] = 0;
        }
      }
    }
    for (; i < n4; i += stride) {
      if (skip && skipped(i)) continue;
      bool live = true, warm = true;
      int64_t row = 0;
      if (gm) {
        row = row_of(i);
        live = gm[row] != 0;
        if (wr) {
          warm = wr[row] != 0;
          if (!live && !warm) continue;  // (zero moments, zero gradient: the update changes nothing)
        }
      }
      f4 p = ld(P + i);
      const f4 g = (zg || !live) ? zero : ld(G + i);
      f4 a = S1 ? ld(S1 + i) : zero;
      f4 b = S2 ? ld(S2 + i) : zero;
      if (PATH == OPT_MARK_ACC_U) {  // (the remainder of the form above: the other forms keep their loop as it was)
        f4 gs = g;
        if (A64 && gm && live) add_totals(gs, A64[2 * i], A64[2 * i + 1], i);
        one(p, gs, a, b);
      } else {
        one(p, g, a, b);
      }
      st(P + i, p);
      if (S1) st(S1 + i, a);
      if (S2) st(S2 + i, b);
      // re-zero only what the scatter touched (~1 % of the rows): saves the 4 B/element store of a blind memset
      if (h.zero_grad && (g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f)) G[i] = zero;
      if (gm && live && (i << 2) == row * re) {
        gm[row] = 0;
        if (!warm) wr[row] = 1;
      }
    }
  }
  const int64_t tail0 = vec ? (n4 << 2) : 0;
  for (int64_t i = tail0 + tid; i < T.n; i += stride) {
    if (T.skip_rows) {
      const int64_t row = i / (T.row_elems > 0 ? T.row_elems : 1);
      if ((T.skip_rows[row >> 5] >> (row & 31)) & 1u) continue;
    }
    float p = T.param[i], a = T.state1 ? T.state1[i] : 0.f, b = T.state2 ? T.state2[i] : 0.f;
    opt_update(h, c, p, reg_grad(T.zero_grads ? 0.f : T.grad[i], p, T.l1, T.l2), a, b);
    T.param[i] = p;
    if (T.state1) T.state1[i] = a;
    if (T.state2) T.state2[i] = b;
    if (h.zero_grad && T.grad[i] != 0.f) gw[i] = 0.f;
  }
}

// Many tensors of very different sizes (MLP weights and biases, the small tables) in ONE balanced launch: the tensors
// are concatenated in units of 4 elements and a thread strides over that index space; the tensor of a chunk is found
// by bisection of the prefix table (kept in LDS with the descriptors: a per-lane index into the kernel-argument block
// would send it to scratch).
__global__ __launch_bounds__(256) void opt_flat_kernel(const OptLaunch L) {
  __shared__ mml_opt_tensor ts[MML_MAX_OPT_TENSORS];
  __shared__ int64_t pre[MML_MAX_OPT_TENSORS + 1];
  for (int i = threadIdx.x; i < L.n; i += 256) ts[i] = L.t[i];
  for (int i = threadIdx.x; i <= L.n; i += 256) pre[i] = L.chunk0[i];
  const mml_opt_hyper& h = L.h;
  __syncthreads();  // (publishes ts / pre)
  const StepConsts c = step_consts(h, L.sc);
  const int64_t total = pre[L.n];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < total; ch += stride) {
    int lo = 0, hi = L.n;  // largest t with pre[t] <= ch
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pre[mid] <= ch) lo = mid;
      else hi = mid;
    }
    const mml_opt_tensor T = ts[lo];
    const int64_t e0 = (ch - pre[lo]) << 2;
    float* gw = const_cast<float*>(T.grad);
    const int re = T.row_elems > 0 ? T.row_elems : 1;
    if (T.skip_rows && re % 4 == 0) {  // chunk inside one row
      const int64_t row = e0 / re;
      if ((T.skip_rows[row >> 5] >> (row & 31)) & 1u) continue;
    }
    const bool vec = (e0 + 4 <= T.n) && aligned16(T.param) && aligned16(T.grad) && (!T.state1 || aligned16(T.state1)) &&
                     (!T.state2 || aligned16(T.state2));
    if (vec) {
      float4 p = *reinterpret_cast<float4*>(T.param + e0);
      const float4 g = T.zero_grads ? make_float4(0, 0, 0, 0) : *reinterpret_cast<const float4*>(T.grad + e0);
      float4 a = T.state1 ? *reinterpret_cast<float4*>(T.state1 + e0) : make_float4(0, 0, 0, 0);
      float4 b = T.state2 ? *reinterpret_cast<float4*>(T.state2 + e0) : make_float4(0, 0, 0, 0);
      opt_update(h, c, p.x, reg_grad(g.x, p.x, T.l1, T.l2), a.x, b.x);
      opt_update(h, c, p.y, reg_grad(g.y, p.y, T.l1, T.l2), a.y, b.y);
      opt_update(h, c, p.z, reg_grad(g.z, p.z, T.l1, T.l2), a.z, b.z);
      opt_update(h, c, p.w, reg_grad(g.w, p.w, T.l1, T.l2), a.w, b.w);
      *reinterpret_cast<float4*>(T.param + e0) = p;
      if (T.state1) *reinterpret_cast<float4*>(T.state1 + e0) = a;
      if (T.state2) *reinterpret_cast<float4*>(T.state2 + e0) = b;
      if (h.zero_grad && (g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f))
        *reinterpret_cast<float4*>(gw + e0) = make_float4(0, 0, 0, 0);
    } else {
      for (int64_t i = e0; i < e0 + 4 && i < T.n; ++i) {
        if (T.skip_rows) {
          const int64_t row = i / re;
          if ((T.skip_rows[row >> 5] >> (row & 31)) & 1u) continue;
        }
        float p = T.param[i], a = T.state1 ? T.state1[i] : 0.f, b = T.state2 ? T.state2[i] : 0.f;
        const float g = T.zero_grads ? 0.f : T.grad[i];
        opt_update(h, c, p, reg_grad(g, p, T.l1, T.l2), a, b);
        T.param[i] = p;
        if (T.state1) T.state1[i] = a;
        if (T.state2) T.state2[i] = b;
        if (h.zero_grad && g != 0.f) gw[i] = 0.f;
      }
    }
  }
}

// sparse rows: one E-float row per group of lanes, rows taken from the touched list
struct RowsLaunch {
  float* tab[MML_MAX_FIELDS];
  float* grad[MML_MAX_FIELDS];
  float* s1[MML_MAX_FIELDS];
  float* s2[MML_MAX_FIELDS];
  uint32_t* seen[MML_MAX_FIELDS];
  int64_t rowbase[MML_MAX_FIELDS + 1];
  int32_t F, E;
  int32_t* last[MML_MAX_FIELDS];  // lazy-exact mode: per-row "current as of step" words (or all null)
  const int32_t* touched;
  const int32_t* touched_count;
  int32_t cap;
  int32_t pad_;
  mml_opt_hyper h;
  const mml_opt_step_consts* sc;  // as OptLaunch.sc
};

// field of a global row id: bisection of an LDS copy of rowbase (a per-lane scan of the kernel-argument array is a
// chain of up to F dependent loads: it was most of the touched-row kernels' time)
__device__ __forceinline__ int field_of_row(const int64_t* rb_lds, int F, int64_t grow) {
  int lo = 0, hi = F;  // largest f with rb[f] <= grow
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rb_lds[mid] <= grow) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One lane = one 16-byte piece of a touched row (E % 4 == 0; else one float): four independent element updates per
// lane, and the row / field decode once per piece instead of once per float.
template <int VEC>
__global__ __launch_bounds__(256) void opt_rows_kernel(const RowsLaunch L) {
  const mml_opt_hyper& h = L.h;
  // per-field descriptors in LDS: a per-lane index into the kernel-argument arrays is a memory load per use
  __shared__ int64_t rb_lds[MML_MAX_FIELDS + 1];
  __shared__ float* tab_l[MML_MAX_FIELDS];
  __shared__ float* grad_l[MML_MAX_FIELDS];
  __shared__ float* s1_l[MML_MAX_FIELDS];
  __shared__ float* s2_l[MML_MAX_FIELDS];
  __shared__ uint32_t* seen_l[MML_MAX_FIELDS];
  __shared__ int32_t* last_l[MML_MAX_FIELDS];
  for (int i = threadIdx.x; i <= L.F; i += 256) rb_lds[i] = L.rowbase[i];
  for (int i = threadIdx.x; i < L.F; i += 256) {
    tab_l[i] = L.tab[i]; grad_l[i] = L.grad[i]; s1_l[i] = L.s1[i]; s2_l[i] = L.s2[i]; seen_l[i] = L.seen[i];
    last_l[i] = L.last[i];
  }
  __syncthreads();  // (publishes rb_lds and the descriptors)
  const StepConsts c = step_consts(h, L.sc);
  int32_t cnt = *L.touched_count;
  if (cnt > L.cap) cnt = L.cap;
  const int per_row = L.E / VEC;
  const int64_t total = (int64_t)cnt * per_row;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < total; item += stride) {
    const int32_t li = (int32_t)(item / per_row);
    const int e = (int)(item - (int64_t)li * per_row) * VEC;
    const int64_t grow = L.touched[li];
    const int f = field_of_row(rb_lds, L.F, grow);
    const int64_t row = grow - rb_lds[f];
    const int64_t o = row * L.E + e;
    float* const T_ = tab_l[f];
    float* const G_ = grad_l[f];
    float* const S1 = s1_l[f];
    float* const S2 = s2_l[f];
    float p[VEC], g[VEC], a[VEC], b[VEC];
    if (VEC == 4) {
      *reinterpret_cast<float4*>(p) = *reinterpret_cast<const float4*>(T_ + o);
      *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(G_ + o);
      if (S1) *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(S1 + o);
      if (S2) *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(S2 + o);
    } else {
      p[0] = T_[o];
      g[0] = G_[o];
      if (S1) a[0] = S1[o];
      if (S2) b[0] = S2[o];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (!S1) a[k] = 0.f;
      if (!S2) b[k] = 0.f;
      opt_update(h, c, p[k], g[k], a[k], b[k]);
    }
    if (VEC == 4) {
      *reinterpret_cast<float4*>(T_ + o) = *reinterpret_cast<float4*>(p);
      if (S1) *reinterpret_cast<float4*>(S1 + o) = *reinterpret_cast<float4*>(a);
      if (S2) *reinterpret_cast<float4*>(S2 + o) = *reinterpret_cast<float4*>(b);
      *reinterpret_cast<float4*>(G_ + o) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      T_[o] = p[0];
      if (S1) S1[o] = a[0];
      if (S2) S2[o] = b[0];
      G_[o] = 0.f;
    }
    if (e == 0) {
      atomicAnd(seen_l[f] + (row >> 5), ~(1u << (row & 31)));
      if (last_l[f]) last_l[f][row] = h.step_dev ? *h.step_dev : h.step;
    }
  }
}

// ---- lazy-exact catch-up ---------------------------------------------------------------------------
// Replays the zero-gradient steps (from, to] of the dense optimizer for one element, with the per-step arithmetic of
// opt_update (g = 0).  Bias corrections follow torch (double precision powers), advanced by recurrence.
__device__ __forceinline__ void catchup_element(const mml_opt_hyper& h, int from, int to, float& p, float& m, float& v) {
  if (to <= from) return;
  if (h.kind == MML_OPT_ADAM) {
    if (m == 0.f) {  // never had a gradient (or fully decayed): p cannot move, v only decays
      v *= powf(h.beta2, (float)(to - from));
      return;
    }
    // bias-correction powers by float recurrence (one powf to start): ~1e-7 relative on the step size, far below
    // the 1e-4 parity budget, and an order of magnitude cheaper per replayed step than double-precision pow/div/sqrt
    float b1p = powf(h.beta1, (float)from), b2p = powf(h.beta2, (float)from);
    int j = from;
    while (j < to) {
      ++j;
      b1p *= h.beta1;
      b2p *= h.beta2;
      StepConsts c;
      c.step_size = h.lr / (1.f - b1p);
      c.inv_bc2s = rsqrtf(1.f - b2p);
      const float before = p;
      opt_update(h, c, p, 0.f, m, v);
      // the per-step move shrinks by ~0.9 per step once the bias-correction growth has died out (j > 16): when it
      // no longer changes p in fp32 it never will again, and only the moments keep decaying
      if (p == before && j - from > 16) {
        const float rem = (float)(to - j);
        m *= powf(h.beta1, rem);
        v *= powf(h.beta2, rem);
        return;
      }
    }
  } else if (h.kind == MML_OPT_RMSPROP) {
    m *= powf(h.alpha, (float)(to - from));  // `m` carries state1 = square_avg: p does not move, the average decays
  }
  // SGD / Adagrad: a zero gradient changes nothing
}

struct CatchupLaunch {
  float* tab[MML_MAX_FIELDS];
  float* s1[MML_MAX_FIELDS];
  float* s2[MML_MAX_FIELDS];
  int32_t* last[MML_MAX_FIELDS];
  int64_t rowbase[MML_MAX_FIELDS + 1];
  int32_t F, E;
  const int32_t* touched;
  const int32_t* touched_count;
  int32_t cap;
  int32_t dense;      // 1: every row of table 0 (V rows), no list
  int64_t V;
  mml_opt_hyper h;
};

// log2 of the lanes a row of E elements gets in opt_catchup_kernel: the next power of two at or above E (1 <= E <= 64)
__host__ __device__ __forceinline__ int catchup_group_shift(int E) {
  int s = 0;
  while ((1 << s) < E) ++s;
  return s;
}

__global__ __launch_bounds__(256) void opt_catchup_kernel(const CatchupLaunch L) {
  __shared__ int64_t rb_lds[MML_MAX_FIELDS + 1];
  if (!L.dense) {
    for (int i = threadIdx.x; i <= L.F; i += 256) rb_lds[i] = L.rowbase[i];
    __syncthreads();
  }
  const mml_opt_hyper& h = L.h;
  const int target = (h.step_dev ? *h.step_dev : h.step) - (L.dense ? 0 : 1);
  int64_t nrows;
  if (L.dense) {
    nrows = L.V;
  } else {
    int32_t cnt = *L.touched_count;
    nrows = cnt > L.cap ? L.cap : cnt;
  }
  // A row is a group of 2^gsh adjacent lanes, the next power of two at or above E (E <= 64: launch_catchup), lanes
  // e >= E idle: the group lies inside ONE wave and ONE trip of the loop (2^gsh divides the wave, the workgroup and the
  // grid's stride).  For E a power of two the items are row * E + e as they always were.
  const int gsh = catchup_group_shift(L.E);
  const int64_t total = nrows << gsh;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < total; item += stride) {
    const int64_t li = item >> gsh;
    const int e = (int)(item & ((1 << gsh) - 1));
    if (e >= L.E) continue;
    int f = 0;
    int64_t row = li;
    if (!L.dense) {
      const int64_t grow = L.touched[li];
      f = field_of_row(rb_lds, L.F, grow);
      row = grow - rb_lds[f];
    }
    const int from = L.last[f][row];
    if (from >= target) continue;
    const int64_t o = row * L.E + e;
    float p = L.tab[f][o];
    float m = L.s1[f] ? L.s1[f][o] : 0.f, v = L.s2[f] ? L.s2[f][o] : 0.f;
    catchup_element(h, from, target, p, m, v);
    L.tab[f][o] = p;
    if (L.s1[f]) L.s1[f][o] = m;
    if (L.s2[f]) L.s2[f][o] = v;
    // The row's lanes are one lane group of this wave in this trip (above), so all of them have read `from` in the one
    // wave-instruction above, which the wave issues before this store: lane 0 may now publish the new step.  No lane of
    // another wave, workgroup or trip reads this row's word.  (Items dealt as row * E + e put the elements of a row
    // into two waves or two trips whenever E does not divide 64: the late ones found from == target and skipped
    // their replay.)
    __builtin_amdgcn_wave_barrier();
    if (e == 0) L.last[f][row] = target;
  }
}

// the counter's bump and the new step's constants in one launch (mml_opt_step_begin); the step is written last: it is
// what tells a reader whose constants these are
__global__ void step_begin_kernel(int32_t* c, int32_t delta, const mml_opt_hyper h, mml_opt_step_consts* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int t = *c + delta;
    *c = t;
    const StepConsts k = step_consts_of(h, t);
    out->step_size = k.step_size;
    out->inv_bc2s = k.inv_bc2s;
    out->pad_ = 0;
    out->step = t;
  }
}

}  // namespace mml

using namespace mml;

static int check_hyper(const mml_opt_hyper* h, const char* who) {
  MML_REQUIRE(h, "%s: null hyper", who);
  MML_REQUIRE(h->kind >= MML_OPT_SGD && h->kind <= MML_OPT_RMSPROP, "%s: unknown optimizer kind %d", who, h->kind);
  MML_REQUIRE(h->kind != MML_OPT_ADAM || h->step_dev || h->step >= 1, "%s: Adam needs step >= 1", who);
  return MML_OK;
}

// ---- step constants kept on the device (mml_opt_step_begin) ----------------------------------------------------------
// step counter -> the buffer its constants are in and the hyper values they were computed under.  A handful of entries
// (one per optimizer alive in the process), looked up on the host by every optimizer launch.
namespace {
struct StepBinding {
  const int32_t* step_dev;
  const mml_opt_step_consts* consts;
  int32_t kind;
  float lr, beta1, beta2;
};
std::mutex g_step_mu;
std::vector<StepBinding> g_step_bindings;

void step_unbind(const int32_t* step_dev) {
  std::lock_guard<std::mutex> lk(g_step_mu);
  for (size_t i = 0; i < g_step_bindings.size(); ++i)
    if (g_step_bindings[i].step_dev == step_dev) {
      g_step_bindings[i] = g_step_bindings.back();
      g_step_bindings.pop_back();
      return;
    }
}

// the constants' buffer for a launch under `h`, or null (then every workgroup computes them)
const mml_opt_step_consts* step_bound(const mml_opt_hyper& h) {
  if (!h.step_dev) return nullptr;
  std::lock_guard<std::mutex> lk(g_step_mu);
  for (const StepBinding& b : g_step_bindings)
    if (b.step_dev == h.step_dev)
      return (b.kind == h.kind && b.lr == h.lr && b.beta1 == h.beta1 && b.beta2 == h.beta2) ? b.consts : nullptr;
  return nullptr;
}
}  // namespace

extern "C" int mml_opt_step_begin(int32_t* step_dev, int32_t delta, const mml_opt_hyper* hyper,
                                  mml_opt_step_consts* consts, mml_stream_t stream) {
  MML_REQUIRE(hyper, "mml_opt_step_begin: null hyper");
  MML_REQUIRE(hyper->kind >= MML_OPT_SGD && hyper->kind <= MML_OPT_RMSPROP, "mml_opt_step_begin: unknown optimizer kind %d",
              hyper->kind);
  MML_REQUIRE(step_dev && consts && aligned16(consts), "mml_opt_step_begin: needs a counter and a 16-byte aligned buffer");
  MML_LAUNCH(step_begin_kernel, dim3(1), dim3(64), 0, to_stream(stream), step_dev, delta, *hyper, consts);
  const int rc = check_launch("mml_opt_step_begin");
  if (rc) return rc;
  step_unbind(step_dev);
  std::lock_guard<std::mutex> lk(g_step_mu);
  g_step_bindings.push_back(StepBinding{step_dev, consts, hyper->kind, hyper->lr, hyper->beta1, hyper->beta2});
  return MML_OK;
}

extern "C" int mml_opt_step_unbind(const int32_t* step_dev) {
  step_unbind(step_dev);
  return MML_OK;
}

namespace {
// the lab knobs of the launch rule (opt_plan.hpp), read once
const OptEnv& opt_env() {
  static const OptEnv env = [] {
    auto num = [](const char* name, int dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) : dflt;
    };
    OptEnv v = OPT_ENV_DEFAULT;
    v.variant = num("MMLREC_OPT_VARIANT", v.variant);
    v.cold_wgs = num("MMLREC_OPT_COLD_WGS", v.cold_wgs);
    if (v.cold_wgs < 1 || v.cold_wgs > 256 * 8) v.cold_wgs = 256 * 8;
    v.resident_per_cu = num("MMLREC_OPT_RESIDENT_PER_CU", v.resident_per_cu);
    if (v.resident_per_cu < 1 || v.resident_per_cu > 64) v.resident_per_cu = 8;
    v.u_mark = num("MMLREC_OPT_U", v.u_mark);  // (a value without an instantiation: the plan falls back to 2)
    return v;
  }();
  return env;
}

// every instantiation of opt_dense_kernel (DensePlan.form, .u)
typedef void (*DenseKernel)(const OptLaunch);
const struct {
  int form, u;
  DenseKernel kernel;
} DENSE_KERNELS[] = {
    {OPT_PLAIN, 1, opt_dense_kernel<true, OPT_PLAIN, 1>},
    {OPT_UNROLL2, 1, opt_dense_kernel<true, OPT_UNROLL2, 1>},
    {OPT_SKIP_U, 4, opt_dense_kernel<true, OPT_SKIP_U, 4>},
    {OPT_MARK_U, 2, opt_dense_kernel<true, OPT_MARK_U, 2>},
    {OPT_MARK_U, 4, opt_dense_kernel<true, OPT_MARK_U, 4>},
    {OPT_MARK_U, 8, opt_dense_kernel<true, OPT_MARK_U, 8>},
    {OPT_MARK_ACC_U, 2, opt_dense_kernel<true, OPT_MARK_ACC_U, 2>},
    {OPT_MARK_ACC_U, 4, opt_dense_kernel<true, OPT_MARK_ACC_U, 4>},
};

int check_dense_tensor(const mml_opt_tensor& t, int i, const mml_opt_hyper* hyper) {
  MML_REQUIRE(t.param && t.grad && t.n >= 0, "mml_opt_step_dense: tensor %d malformed", i);
  MML_REQUIRE(hyper->kind == MML_OPT_SGD || t.state1, "mml_opt_step_dense: tensor %d needs state1", i);
  MML_REQUIRE(hyper->kind != MML_OPT_ADAM || t.state2, "mml_opt_step_dense: tensor %d needs state2 (Adam)", i);
  // (both kernels decide per 16-byte chunk by the row of its first element: a chunk must not straddle two rows)
  MML_REQUIRE(!t.skip_rows || (t.row_elems > 0 && t.row_elems % 4 == 0 && t.n % t.row_elems == 0 &&
                               aligned16(t.param)),
              "mml_opt_step_dense: tensor %d: skip_rows needs row_elems %% 4 == 0 dividing n and a 16-byte aligned "
              "parameter (16-byte chunks must lie inside one row)", i);
  if (t.acc64) {
    MML_REQUIRE(t.grad_marks && !t.skip_rows && t.acc_amax && aligned16(t.acc64) && t.acc_shift >= 4 &&
                    t.acc_shift <= 28,
                "mml_opt_step_dense: tensor %d: acc64 (deferred totals of mml_scatter_bwd_det) needs grad_marks, no "
                "skip_rows, a 16-byte aligned int64 array, acc_amax and acc_shift = mml_scatter_det_shift(B)", i);
  }
  if (t.grad_marks) {
    const int cpr = t.row_elems / 4;
    MML_REQUIRE(t.row_elems > 0 && t.row_elems % 4 == 0 && cpr <= 64 && (cpr & (cpr - 1)) == 0 &&
                    t.n % t.row_elems == 0 && !t.skip_rows && aligned16(t.param) && aligned16(t.grad) &&
                    (!t.state1 || aligned16(t.state1)) && (!t.state2 || aligned16(t.state2)),
                "mml_opt_step_dense: tensor %d: grad_marks needs 16-byte aligned [rows, row_elems] tensors with "
                "row_elems / 4 a power of two <= 64 and no skip_rows", i);
  }
  if (t.warm_rows) {
    MML_REQUIRE(t.grad_marks && t.l1 == 0.f && t.l2 == 0.f,
                "mml_opt_step_dense: tensor %d: warm_rows needs grad_marks and no regulariser (a regulariser moves a "
                "row whose moments and gradient are zero)", i);
  }
  return MML_OK;
}
}  // namespace

// Per group of at most MML_MAX_OPT_TENSORS tensors: validate each descriptor, plan the group (opt_plan.hpp), fill
// OptLaunch from the plan, launch from the table.
extern "C" int mml_opt_step_dense(const mml_opt_tensor* tensors, int32_t n, const mml_opt_hyper* hyper,
                                  mml_stream_t stream) {
  int rc = check_hyper(hyper, "mml_opt_step_dense");
  if (rc) return rc;
  const mml_opt_step_consts* const bound = step_bound(*hyper);
  MML_REQUIRE(n >= 0 && (n == 0 || tensors), "mml_opt_step_dense: bad tensor array");
  int i = 0;
  while (i < n) {
    OptLaunch L{};
    L.h = *hyper;
    L.sc = bound;
    int64_t total = 0, chunks = 0;
    while (i < n && L.n < MML_MAX_OPT_TENSORS) {
      rc = check_dense_tensor(tensors[i], i, hyper);
      if (rc) return rc;
      L.chunk0[L.n] = chunks;
      L.t[L.n++] = tensors[i];
      total += tensors[i].n;
      chunks += cdiv(tensors[i].n, 4);
      ++i;
    }
    L.chunk0[L.n] = chunks;
    if (total == 0) continue;
    DensePlan P;
    const char* const refused = opt_plan_dense(L.t, L.n, *hyper, opt_env(), device_cus(), P);
    MML_REQUIRE(!refused, "%s", refused);
    L.variant = P.variant;
    L.prop = P.prop;
    memcpy(L.blk0, P.blk0, sizeof(L.blk0));
    if (P.form == OPT_FLAT) {
      MML_LAUNCH(opt_flat_kernel, dim3(P.grid_x), dim3(256), 0, to_stream(stream), L);
    } else {
      DenseKernel kernel = nullptr;
      for (const auto& k : DENSE_KERNELS)
        if (k.form == P.form && k.u == P.u) kernel = k.kernel;
      MML_REQUIRE(kernel, "mml_opt_step_dense: no opt_dense_kernel<true, %d, %d>", P.form, P.u);
      MML_LAUNCH(kernel, dim3(P.grid_x, P.grid_y), dim3(256), 0, to_stream(stream), L);
    }
    rc = check_launch("mml_opt_step_dense");
    if (rc) return rc;
  }
  return MML_OK;
}

// max_rows rows at most, each a lane group of the next power of two at or above E (opt_catchup_kernel); E a power of
// two: the grid of max_rows * E items.  E > 64 is refused: a row has to fit one wave.
static int launch_catchup(CatchupLaunch& L, int64_t max_rows, hipStream_t st, const char* who) {
  MML_REQUIRE(L.E <= 64, "%s: E = %d: a row's elements are the lanes of one wave, E <= 64", who, L.E);
  int64_t blocks = cdiv(max_rows << catchup_group_shift(L.E), 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (blocks < 1) blocks = 1;
  MML_LAUNCH(opt_catchup_kernel, dim3((unsigned)blocks), dim3(256), 0, st, L);
  return check_launch(who);
}

extern "C" int mml_opt_catchup_rows(float* const* tables, float* const* state1, float* const* state2,
                                    int32_t* const* last, const int64_t* rowbase, int32_t F, int32_t E,
                                    const int32_t* touched, const int32_t* touched_count, int32_t touched_cap,
                                    const mml_opt_hyper* hyper, mml_stream_t stream) {
  int rc = check_hyper(hyper, "mml_opt_catchup_rows");
  if (rc) return rc;
  MML_REQUIRE(F >= 1 && F <= MML_MAX_FIELDS && E > 0 && tables && last && rowbase && touched && touched_count &&
                  touched_cap > 0, "mml_opt_catchup_rows: bad arguments");
  if (hyper->kind == MML_OPT_SGD || hyper->kind == MML_OPT_ADAGRAD) return MML_OK;  // zero gradients change nothing
  CatchupLaunch L{};
  for (int f = 0; f < F; ++f) {
    MML_REQUIRE(tables[f] && last[f] && state1 && state1[f], "mml_opt_catchup_rows: field %d null", f);
    MML_REQUIRE(hyper->kind != MML_OPT_ADAM || (state2 && state2[f]), "mml_opt_catchup_rows: field %d needs state2", f);
    L.tab[f] = tables[f]; L.s1[f] = state1[f]; L.s2[f] = state2 ? state2[f] : nullptr; L.last[f] = last[f];
    L.rowbase[f] = rowbase[f];
  }
  L.rowbase[F] = rowbase[F];
  L.F = F; L.E = E; L.touched = touched; L.touched_count = touched_count; L.cap = touched_cap; L.h = *hyper;
  return launch_catchup(L, (int64_t)touched_cap, to_stream(stream), "mml_opt_catchup_rows");
}

extern "C" int mml_opt_catchup_dense(float* table, float* state1, float* state2, int32_t* last, int64_t V, int32_t E,
                                     const mml_opt_hyper* hyper, mml_stream_t stream) {
  int rc = check_hyper(hyper, "mml_opt_catchup_dense");
  if (rc) return rc;
  MML_REQUIRE(table && last && V >= 0 && E > 0, "mml_opt_catchup_dense: bad arguments");
  if (V == 0 || hyper->kind == MML_OPT_SGD || hyper->kind == MML_OPT_ADAGRAD) return MML_OK;
  MML_REQUIRE(state1 && (hyper->kind != MML_OPT_ADAM || state2), "mml_opt_catchup_dense: optimizer state missing");
  CatchupLaunch L{};
  L.tab[0] = table; L.s1[0] = state1; L.s2[0] = state2; L.last[0] = last;
  L.F = 1; L.E = E; L.dense = 1; L.V = V; L.h = *hyper;
  return launch_catchup(L, V, to_stream(stream), "mml_opt_catchup_dense");
}

extern "C" int mml_opt_step_rows(float* const* tables, float* const* grad_tables, float* const* state1,
                                 float* const* state2, uint32_t* const* seen, const int64_t* rowbase, int32_t F,
                                 int32_t E, const int32_t* touched, const int32_t* touched_count, int32_t touched_cap,
                                 int32_t* const* last, const mml_opt_hyper* hyper, mml_stream_t stream) {
  int rc = check_hyper(hyper, "mml_opt_step_rows");
  if (rc) return rc;
  MML_REQUIRE(F >= 1 && F <= MML_MAX_FIELDS && E > 0, "mml_opt_step_rows: bad F/E");
  MML_REQUIRE(tables && grad_tables && seen && rowbase && touched && touched_count && touched_cap > 0,
              "mml_opt_step_rows: null argument");
  RowsLaunch L{};
  for (int f = 0; f < F; ++f) {
    MML_REQUIRE(tables[f] && grad_tables[f] && seen[f], "mml_opt_step_rows: field %d null", f);
    L.tab[f] = tables[f]; L.grad[f] = grad_tables[f]; L.seen[f] = seen[f];
    L.s1[f] = state1 ? state1[f] : nullptr;
    L.s2[f] = state2 ? state2[f] : nullptr;
    MML_REQUIRE(hyper->kind == MML_OPT_SGD || L.s1[f], "mml_opt_step_rows: field %d needs state1", f);
    MML_REQUIRE(hyper->kind != MML_OPT_ADAM || L.s2[f], "mml_opt_step_rows: field %d needs state2", f);
    L.rowbase[f] = rowbase[f];
    L.last[f] = last ? last[f] : nullptr;
  }
  L.rowbase[F] = rowbase[F];
  L.F = F; L.E = E; L.touched = touched; L.touched_count = touched_count; L.cap = touched_cap; L.h = *hyper;
  L.sc = step_bound(*hyper);
  // the row count lives on the device: size the grid for the capacity, surplus workgroups exit at once
  bool vec = (E % 4 == 0);
  for (int f = 0; f < F && vec; ++f)
    vec = aligned16(L.tab[f]) && aligned16(L.grad[f]) && (!L.s1[f] || aligned16(L.s1[f])) && (!L.s2[f] || aligned16(L.s2[f]));
  int64_t blocks = cdiv((int64_t)touched_cap * (vec ? E / 4 : E), 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (vec) MML_LAUNCH(opt_rows_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, to_stream(stream), L);
  else MML_LAUNCH(opt_rows_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, to_stream(stream), L);
  return check_launch("mml_opt_step_rows");
}

