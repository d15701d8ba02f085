// K1p / K2p: multi-valued (pooled) sparse features beside the single-valued ones (include/mmlrec.h: mml_pool_desc).
//
// K1p restates varlen_embedding_lookup + get_varlen_pooling_list + SequencePoolingLayer of the reference
// (model/utils.py:520-533, :449-463, :258-326) together with K1's input_from_feature_columns / combined_dnn_input as
// ONE launch: the workgroups of segment 0 copy the single-valued blocks and the dense columns exactly as
// gather_vec4_kernel does, the workgroups of segment 1 + p pool field p.
//
// K2p is their backward: one workgroup takes ONE field and a chunk of at most CHUNK lookups (a single-valued field:
// CHUNK samples; a pooled field: CHUNK / maxlen samples x maxlen positions), folds duplicate rows in LDS in 64-bit
// fixed point and flushes E contiguous float atomics per distinct row -- the fold of scatter_fold.hpp, shared with
// scatter_fold_kernel, with one lookup per lane group.  The bookkeeping is per TABLE, so fields that share a table
// share its bitmap and its mark range.
//
// K2p deterministic (mml_scatter_pool_bwd_det): the same kernel with DET set -- the fixed-point unit comes from the
// launch-wide magnitude of dOut and the shift of mml_scatter_pool_det_shift, and the flush adds the chunk sums to
// per-TABLE 64-bit row totals with integer atomics; scatter_det_finalize_kernel (gather_scatter.hip) turns them into
// the fp32 gradient, one workgroup range per table.
#include "common.hpp"
#include "scatter_det.hpp"
#include "scatter_fold.hpp"

namespace mml {

// ------------------------------------------------------------------------------------------------
// K1p gather
// ------------------------------------------------------------------------------------------------
struct PoolGatherArgs {
  // segment 0: single-valued fields (table pointers resolved on the host) and the dense columns
  const float* s_tab[MML_MAX_FIELDS];
  int32_t s_vocab[MML_MAX_FIELDS];
  int32_t s_col[MML_MAX_FIELDS];
  // segment 1 + p: pooled field p
  const float* p_tab[MML_MAX_POOLED];
  int32_t p_vocab[MML_MAX_POOLED];
  int32_t p_col0[MML_MAX_POOLED], p_T[MML_MAX_POOLED], p_len_col[MML_MAX_POOLED], p_comb[MML_MAX_POOLED];
  int32_t blk0[MML_MAX_POOLED + 2];  // first workgroup of every segment
  const float* X;
  int64_t ldX, B, ldo, ldarg;
  int32_t F, P, E, dense_col0, Nd;
  float* out;
  uint8_t* argmax;
  float* wgmax;
  int32_t* status;
};

// lanes of one (sample, pooled field): LPS lanes per row piece x the smallest power of two of positions >= maxlen,
// at most one wave
__host__ __device__ inline int pool_group(int T, int lps) {
  int g = lps;
  while (g < 64 && g < T * lps) g <<= 1;
  return g;
}

// samples one lane group pools: a field whose positions fit one pass (maxlen <= G / LPS) takes kPoolSamples samples per
// group, so that every lane still has that many independent id -> row loads in flight
constexpr int kPoolSamples = 4;
__host__ __device__ inline int pool_block_samples(int T, int lps) {
  const int g = pool_group(T, lps);
  return (256 / g) * (T * lps <= g ? kPoolSamples : 1);
}

__device__ __forceinline__ void pool_take_max(float& v, int& at, float w, int t) {
  // the lowest position wins a tie (torch's max over dim on the CPU, and the rule mml_scatter_pool_bwd follows)
  if (w > v || (w == v && t < at)) {
    v = w;
    at = t;
  }
}

// One row piece of position t joins the running reduction of its lane.
__device__ __forceinline__ void pool_combine(int comb, bool inr, bool valid, const float4& r, int t, float4& acc,
                                             int at[4], int& cnt) {
  if (!inr) return;
  if (comb == MML_POOL_MAX) {
    const float off = valid ? 0.f : 1e9f;  // row_t - (1 - valid_t) * 1e9 (model/utils.py:315): exact for a valid row
    pool_take_max(acc.x, at[0], valid ? r.x : r.x - off, t);
    pool_take_max(acc.y, at[1], valid ? r.y : r.y - off, t);
    pool_take_max(acc.z, at[2], valid ? r.z : r.z - off, t);
    pool_take_max(acc.w, at[3], valid ? r.w : r.w - off, t);
  } else if (valid) {
    acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += r.w;
  }
  cnt += valid ? 1 : 0;
}

// The positions of one sample, spread over the lanes of its group, are reduced (aligned power-of-two lane groups: the
// xor stays inside) and the lanes of position 0 store the block.
template <bool WGMAX>
__device__ __forceinline__ void pool_finish(const PoolGatherArgs& a, int p, int comb, int G, int e4, int64_t b, bool live,
                                            int tp, int part, float4 acc, int at[4], int cnt, float& am) {
  for (int o = e4; o < G; o <<= 1) {
    const float4 w = make_float4(__shfl_xor(acc.x, o), __shfl_xor(acc.y, o), __shfl_xor(acc.z, o),
                                 __shfl_xor(acc.w, o));
    const int c2 = __shfl_xor(cnt, o);
    if (comb == MML_POOL_MAX) {
      const int a0 = __shfl_xor(at[0], o), a1 = __shfl_xor(at[1], o), a2 = __shfl_xor(at[2], o),
                a3 = __shfl_xor(at[3], o);
      pool_take_max(acc.x, at[0], w.x, a0);
      pool_take_max(acc.y, at[1], w.y, a1);
      pool_take_max(acc.z, at[2], w.z, a2);
      pool_take_max(acc.w, at[3], w.w, a3);
    } else {
      acc.x += w.x; acc.y += w.y; acc.z += w.z; acc.w += w.w;
    }
    cnt += c2;
  }
  if (live && tp == 0) {
    if (comb == MML_POOL_MEAN) {
      const float dv = (float)cnt + 1e-8f;  // model/utils.py:320-322
      acc.x /= dv; acc.y /= dv; acc.z /= dv; acc.w /= dv;
    }
    *reinterpret_cast<float4*>(a.out + b * a.ldo + (int64_t)(a.F + p) * a.E + part * 4) = acc;
    if (comb == MML_POOL_MAX) {
      const uint32_t pk = (uint32_t)(at[0] & 255) | ((uint32_t)(at[1] & 255) << 8) | ((uint32_t)(at[2] & 255) << 16) |
                          ((uint32_t)(at[3] & 255) << 24);
      *reinterpret_cast<uint32_t*>(a.argmax + b * a.ldarg + p * a.E + part * 4) = pk;
    }
    if (WGMAX) amax_acc(am, acc);
  }
}

template <bool WGMAX>
__global__ __launch_bounds__(256) void gather_pool_kernel(const PoolGatherArgs a) {
  float am = 0.f;
  int bad = 0;
  const int e4 = a.E >> 2;
  int seg = 0;
  while (seg + 1 <= a.P && (int)blockIdx.x >= a.blk0[seg + 1]) ++seg;
  const int64_t bx = (int64_t)blockIdx.x - a.blk0[seg];
  if (seg == 0) {
    // ---- single-valued blocks and dense columns: gather_vec4_kernel's item, the dense pieces behind the pooled blocks
    const int nvec = a.F * e4;
    const int per_sample = nvec + ((a.Nd + 3) >> 2);
    const int64_t item = bx * 256 + threadIdx.x;
    const int64_t b = item / per_sample;
    const int c = (int)(item - b * per_sample);
    if (b < a.B) {
      if (c < nvec) {
        const int f = c / e4, part = c - f * e4;
        int64_t i = (int64_t)a.X[b * a.ldX + a.s_col[f]];  // truncates toward zero
        if (i < 0) { bad |= 1; i = 0; }
        else if (i >= a.s_vocab[f]) { bad |= 2; i = a.s_vocab[f] - 1; }
        const float4 v = *reinterpret_cast<const float4*>(a.s_tab[f] + i * a.E + part * 4);
        *reinterpret_cast<float4*>(a.out + b * a.ldo + (int64_t)c * 4) = v;
        if (WGMAX) amax_acc(am, v);
      } else {
        const int j = 4 * (c - nvec);
        const int nj = a.Nd - j;  // >= 1
        const float* src = a.X + b * a.ldX + a.dense_col0 + j;                    // (4-byte aligned only)
        float* dst = a.out + b * a.ldo + (int64_t)(a.F + a.P) * a.E + j;          // (16-byte aligned)
        float4 d = make_float4(src[0], 0.f, 0.f, 0.f);
        if (nj > 1) d.y = src[1];
        if (nj > 2) d.z = src[2];
        if (nj > 3) d.w = src[3];
        if (nj > 3) {
          *reinterpret_cast<float4*>(dst) = d;
        } else {
          dst[0] = d.x;
          if (nj > 1) dst[1] = d.y;
          if (nj > 2) dst[2] = d.z;
        }
        if (WGMAX) amax_acc(am, d);
      }
    }
  } else {
    // ---- pooled field p (workgroup-uniform): a group of G lanes per sample, lane = (position tp, row piece)
    const int p = seg - 1;
    const int T = a.p_T[p], comb = a.p_comb[p], lc = a.p_len_col[p];
    const int64_t V = a.p_vocab[p];
    const float* tab = a.p_tab[p];
    const int G = pool_group(T, e4);
    const int TP = G / e4;  // positions per pass
    const int gi = threadIdx.x / G, li = threadIdx.x - gi * G;
    const int tp = li / e4, part = li - tp * e4;
    if (T <= TP) {
      // ---- every position in ONE pass: the group takes kPoolSamples consecutive samples, their id loads, then their row
      // loads, issued before the first combine (one sample per group left a lane with a single load in flight)
      const int64_t b0 = (bx * (256 / G) + gi) * kPoolSamples;
      const int tc = tp < T ? tp : T - 1;  // a lane beyond maxlen re-reads the last position; its value is dropped
      float idf[kPoolSamples], lenf[kPoolSamples];
      float4 r[kPoolSamples];
      bool inr[kPoolSamples], valid[kPoolSamples];
#pragma unroll
      for (int j = 0; j < kPoolSamples; ++j) {
        const bool lv = b0 + j < a.B;
        const float* xr = a.X + (lv ? b0 + j : a.B - 1) * a.ldX;
        inr[j] = lv && tp < T;
        idf[j] = xr[a.p_col0[p] + tc];
        lenf[j] = xr[lc >= 0 ? lc : a.p_col0[p]];
      }
#pragma unroll
      for (int j = 0; j < kPoolSamples; ++j) {
        int64_t i = (int64_t)idf[j];
        const int64_t l = (int64_t)lenf[j];
        valid[j] = inr[j] && (lc >= 0 ? tp < (l < 0 ? 0 : (l > T ? T : (int)l)) : i != 0);
        if (i < 0) { if (valid[j]) bad |= 1; i = 0; }
        else if (i >= V) { if (valid[j]) bad |= 2; i = V - 1; }
        r[j] = *reinterpret_cast<const float4*>(tab + i * a.E + part * 4);
      }
#pragma unroll
      for (int j = 0; j < kPoolSamples; ++j) {
        float4 acc = comb == MML_POOL_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        int at[4] = {0x7fff, 0x7fff, 0x7fff, 0x7fff};
        int cnt = 0;
        pool_combine(comb, inr[j], valid[j], r[j], tp, acc, at, cnt);
        pool_finish<WGMAX>(a, p, comb, G, e4, b0 + j, b0 + j < a.B, tp, part, acc, at, cnt, am);
      }
    } else {
    const int64_t b = bx * (256 / G) + gi;
    const bool live = b < a.B;
    const int64_t bc = live ? b : a.B - 1;  // every load below has a safe address; what it returns is selected later
    const float* xrow = a.X + bc * a.ldX;
    int n = T;
    if (lc >= 0) {
      const int64_t l = (int64_t)xrow[lc];
      n = l < 0 ? 0 : (l > T ? T : (int)l);
    }
    const float* idp = xrow + a.p_col0[p];  // the maxlen ids of the sample: one contiguous segment, a position per lane
    float4 acc = comb == MML_POOL_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
    int at[4] = {0x7fff, 0x7fff, 0x7fff, 0x7fff};
    int cnt = 0;
    const int passes = (T + TP - 1) / TP;
    // Four passes per step: the four id loads, then the four row loads, are issued before the first combine -- no
    // load -> add chain.  A position beyond maxlen re-reads the last one (its value is dropped), so no load sits behind
    // a branch; a padded or out-of-length position reads the clamped row and is dropped (sum, mean) or lowered (max).
    int k = 0;
    for (; k + 4 <= passes; k += 4) {
      float idf[4];
      float4 r[4];
      bool inr[4], valid[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = tp + (k + j) * TP;
        inr[j] = live && t < T;
        idf[j] = idp[t < T ? t : T - 1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = tp + (k + j) * TP;
        int64_t i = (int64_t)idf[j];
        valid[j] = inr[j] && (lc >= 0 ? t < n : i != 0);
        if (i < 0) { if (valid[j]) bad |= 1; i = 0; }
        else if (i >= V) { if (valid[j]) bad |= 2; i = V - 1; }
        r[j] = *reinterpret_cast<const float4*>(tab + i * a.E + part * 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) pool_combine(comb, inr[j], valid[j], r[j], tp + (k + j) * TP, acc, at, cnt);
    }
    for (; k < passes; ++k) {
      const int t = tp + k * TP;
      const bool inr = live && t < T;
      int64_t i = (int64_t)idp[t < T ? t : T - 1];
      const bool valid = inr && (lc >= 0 ? t < n : i != 0);
      if (i < 0) { if (valid) bad |= 1; i = 0; }
      else if (i >= V) { if (valid) bad |= 2; i = V - 1; }
      const float4 r = *reinterpret_cast<const float4*>(tab + i * a.E + part * 4);
      pool_combine(comb, inr, valid, r, t, acc, at, cnt);
    }
    pool_finish<WGMAX>(a, p, comb, G, e4, b, live, tp, part, acc, at, cnt, am);
    }
  }
  if (bad && a.status) atomicOr(a.status, bad);
  if (WGMAX) {  // ONE plain store per workgroup (see gather_vec4_kernel)
    __shared__ float wmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = am;
    __syncthreads();
    if (threadIdx.x == 0) a.wgmax[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  }
}

// ------------------------------------------------------------------------------------------------
// K2p scatter / index-only pass
// ------------------------------------------------------------------------------------------------
struct PoolFields {  // every field, single-valued ones first
  int32_t col[MML_MAX_FIELDS];      // X column (pooled: the first of T)
  int32_t len_col[MML_MAX_FIELDS];  // -1: mask mode (pooled) / always valid (single-valued)
  int32_t blk0[MML_MAX_FIELDS + 1];
  uint16_t T[MML_MAX_FIELDS];
  uint8_t table[MML_MAX_FIELDS];
  uint8_t kind[MML_MAX_FIELDS];  // 0 single-valued, 1 + combiner pooled
  int32_t nf, F;                 // fields, single-valued fields (field f's block of dOut starts at f * E)
};

struct PoolScatterArgs {
  float* gtab[MML_MAX_FIELDS];  // per TABLE
  uint32_t* seen[MML_MAX_FIELDS];
  int64_t markbase[MML_MAX_FIELDS];
  int32_t vocab[MML_MAX_FIELDS];
  const float* X;
  const float* dOut;  // null: index-only pass
  const uint8_t* argmax;
  int64_t ldX, B, ldo, ldarg;
  uint8_t* marks;
  int32_t want_seen;
  int32_t* status;
  // deterministic mode (mml_scatter_pool_bwd_det): ONE fixed-point unit for the whole launch, from the magnitude slot of
  // dOut, and 64-bit integer totals per TABLE row (the fields of a shared table add to the same totals)
  long long* acc64[MML_MAX_FIELDS];
  const uint32_t* amax_dout;
  int32_t fix_shift;
};

// DET: see scatter_fold_kernel<..., DET> (gather_scatter.hip).  The magnitude of dOut bounds every addend: a mean
// field divides by n + 1e-8 >= 1 wherever a position is valid, a max field passes or zeroes the value, a sum field passes it.
template <int SLOTS, int E, bool DET = false>
__global__ __launch_bounds__((SLOTS / 2) * (E / 4)) void scatter_pool_fold_kernel(const PoolFields fd,
                                                                                   const PoolScatterArgs a) {
  constexpr int LPS = E / 4;        // lanes per lookup
  constexpr int CHUNK = SLOTS / 2;  // lookups per workgroup (hash load factor <= 0.5): ONE per lane group
  constexpr int PITCH = SLOTS + 1;
  extern __shared__ __attribute__((aligned(16))) long long pool_smem[];
  long long* acc = pool_smem;                                             // [E][PITCH] fixed-point sums
  int* keys = reinterpret_cast<int*>(acc + E * PITCH);                    // [SLOTS]
  int* nval = keys + SLOTS;                                               // [CHUNK] valid positions per sample (mask-mode mean)
  unsigned short* occ = reinterpret_cast<unsigned short*>(nval + CHUNK);  // [SLOTS] occupied slots
  __shared__ int n_occ;
  __shared__ unsigned mx_bits;
  int f = 0;
  while (f + 1 < fd.nf && (int)blockIdx.x >= fd.blk0[f + 1]) ++f;
  const int64_t q = (int64_t)blockIdx.x - fd.blk0[f];
  const int T = fd.T[f], kind = fd.kind[f], lc = fd.len_col[f], tb = fd.table[f];
  const int64_t V = a.vocab[tb];
  const int S = CHUNK / T;  // samples of this workgroup (T <= MML_POOL_MAX_LEN <= CHUNK)
  const int part = threadIdx.x % LPS, it = threadIdx.x / LPS;
  const int s = it / T, t = it - s * T;
  const int64_t b = q * S + s;
  const bool live = s < S && b < a.B;
  const int64_t bc = b < a.B ? b : a.B - 1;
  const int lane = threadIdx.x & 63;
  const bool direct = V <= SLOTS;  // slot = row: no compare-and-swap, no probing
  // ---- every load of this lane in flight before the first LDS operation (safe addresses, selected later)
  const float* xrow = a.X + bc * a.ldX;
  const float idf = xrow[fd.col[f] + t];
  const float lenf = lc >= 0 ? xrow[lc] : 0.f;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t am4 = 0;
  if (a.dOut) {
    // the positions of a sample sit on neighbouring lanes and ask for the same 16 bytes: one request per wave-instruction,
    // so the block of dOut leaves memory once per (sample, field)
    g = *reinterpret_cast<const float4*>(a.dOut + bc * a.ldo + (int64_t)f * E + part * 4);
    if (kind == 1 + MML_POOL_MAX)
      am4 = *reinterpret_cast<const uint32_t*>(a.argmax + bc * a.ldarg + (f - fd.F) * E + part * 4);
  }
  const int64_t row = (int64_t)idf;
  int n = T;
  if (lc >= 0) {
    const int64_t l = (int64_t)lenf;
    n = l < 0 ? 0 : (l > T ? T : (int)l);
  }
  bool valid = live && (kind == 0 || (lc >= 0 ? t < n : row != 0));
  int bad = 0;
  if (valid && row < 0) { bad |= 1; valid = false; }
  if (valid && row >= V) { bad |= 2; valid = false; }
  const int key = valid ? (int)row : -1;
  if (a.dOut)
    for (int i = threadIdx.x; i < E * PITCH / 2; i += blockDim.x)
      *reinterpret_cast<float4*>(acc + i * 2) = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) keys[i] = -1;
  for (int i = threadIdx.x; i < CHUNK; i += blockDim.x) nval[i] = 0;
  if (threadIdx.x == 0) { n_occ = 0; mx_bits = 0; }
  __syncthreads();
  const bool count_mask = a.dOut && kind == 1 + MML_POOL_MEAN && lc < 0;  // (uniform)
  if (count_mask) {
    if (valid && part == 0) atomicAdd(&nval[s], 1);
    __syncthreads();
    n = nval[s < CHUNK ? s : 0];
  }
  unsigned mx = 0;
  if (a.dOut) {
    if (kind == 1 + MML_POOL_MEAN) {
      const float dv = (float)n + 1e-8f;  // the reference's divisor (model/utils.py:320-322); n >= 1 where it is used
      g.x /= dv; g.y /= dv; g.z /= dv; g.w /= dv;
    } else if (kind == 1 + MML_POOL_MAX) {
      if ((int)(am4 & 255u) != t) g.x = 0.f;
      if ((int)((am4 >> 8) & 255u) != t) g.y = 0.f;
      if ((int)((am4 >> 16) & 255u) != t) g.z = 0.f;
      if ((int)(am4 >> 24) != t) g.w = 0.f;
    }
    if (!valid) g = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (DET) {  // the launch-wide magnitude of dOut (uniform loads: no LDS round trip)
    unsigned m = 0;
    for (int i = 0; i < MML_AMAX_WORDS; ++i) m = a.amax_dout[i] > m ? a.amax_dout[i] : m;
    mx = m;
  } else if (a.dOut) {
    // largest magnitude (as bit pattern) of the workgroup's gradient values -> the fixed-point scale
    const unsigned m0 = __float_as_uint(g.x) & 0x7fffffffu, m1 = __float_as_uint(g.y) & 0x7fffffffu;
    const unsigned m2 = __float_as_uint(g.z) & 0x7fffffffu, m3 = __float_as_uint(g.w) & 0x7fffffffu;
    mx = max(max(m0, m1), max(m2, m3));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if (lane == 0 && mx) atomicMax(&mx_bits, mx);
    __syncthreads();
    mx = mx_bits;
  }
  int emax = (int)(mx >> 23);
  // Inf / NaN reach the table as float atomics, not through the fold (fold_insert).
  // NOT scatter_fold_kernel's `emax >= 255`: under DET a NaN never raises the magnitude slot, so every addend is looked at.
  const bool nonfinite = DET || emax >= 255;
  emax = emax < 1 ? 1 : (emax > 254 ? 254 : emax);
  const int shift = DET ? a.fix_shift : 28;
  float* gt = a.gtab[tb];
  fold_insert<SLOTS, E>(acc, keys, occ, &n_occ, direct, key, part, lane, a.dOut != nullptr, g, emax, shift, nonfinite, gt);
  __syncthreads();
  // the row is marked for its TABLE
  fold_flush<SLOTS, E, DET>(acc, keys, occ, n_occ, direct, (int)V, (int)blockDim.x, a.dOut != nullptr, gt,
                            DET ? a.acc64[tb] : nullptr, emax, a.marks ? a.marks + a.markbase[tb] : nullptr,
                            a.want_seen ? a.seen[tb] : nullptr);
  if (bad && a.status) atomicOr(a.status, bad);
}

// Index-only pass with a mark map: one byte store per VALID lookup, no LDS, no atomics.  One field per workgroup range.
__global__ __launch_bounds__(256) void mark_pool_rows_kernel(const PoolFields fd, const PoolScatterArgs a) {
  int f = 0;
  while (f + 1 < fd.nf && (int)blockIdx.x >= fd.blk0[f + 1]) ++f;
  const int T = fd.T[f], kind = fd.kind[f], lc = fd.len_col[f], tb = fd.table[f];
  const int64_t V = a.vocab[tb];
  const int64_t total = a.B * T;
  const int64_t stride = (int64_t)(fd.blk0[f + 1] - fd.blk0[f]) * 256;
  int bad = 0;
  for (int64_t i = ((int64_t)blockIdx.x - fd.blk0[f]) * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / T;
    const int t = (int)(i - b * T);
    const float* xrow = a.X + b * a.ldX;
    const int64_t row = (int64_t)xrow[fd.col[f] + t];
    bool valid = true;
    if (kind != 0) {
      if (lc >= 0) {
        const int64_t l = (int64_t)xrow[lc];
        valid = t < (l < 0 ? 0 : (l > T ? T : (int)l));
      } else {
        valid = row != 0;
      }
    }
    if (!valid) continue;
    if (row < 0) bad |= 1;
    else if (row >= V) bad |= 2;
    else a.marks[a.markbase[tb] + row] = 1;
  }
  if (bad && a.status) atomicOr(a.status, bad);
}

template <int SLOTS, int E, bool DET = false>
static int launch_pool_fold(const PoolFields& fd, const PoolScatterArgs& a, int nblocks, hipStream_t stream,
                            const char* who) {
  constexpr int NT = (SLOTS / 2) * (E / 4);
  const size_t lds = (size_t)E * (SLOTS + 1) * 8 + (size_t)SLOTS * 4 + (size_t)(SLOTS / 2) * 4 + (size_t)SLOTS * 2;
  const int rc = allow_big_lds<&scatter_pool_fold_kernel<SLOTS, E, DET>>(who);
  if (rc) return rc;
  MML_LAUNCH((scatter_pool_fold_kernel<SLOTS, E, DET>), dim3((unsigned)nblocks), dim3(NT), lds, stream, fd, a);
  return check_launch(who);
}

}  // namespace mml

using namespace mml;

static int check_desc(const mml_pool_desc* d, bool need_tables, const char* who) {
  MML_REQUIRE(d != nullptr, "%s: null descriptor", who);
  MML_REQUIRE(d->E == 4 || d->E == 8 || d->E == 16, "%s: E=%d, must be 4, 8 or 16", who, d->E);
  MML_REQUIRE(d->n_tables >= 1 && d->n_tables <= MML_MAX_FIELDS, "%s: n_tables=%d outside [1,%d]", who, d->n_tables,
              MML_MAX_FIELDS);
  MML_REQUIRE(d->n_single >= 0 && d->n_pooled >= 0 && d->n_pooled <= MML_MAX_POOLED &&
                  d->n_single + d->n_pooled >= 1 && d->n_single + d->n_pooled <= MML_MAX_FIELDS,
              "%s: n_single=%d n_pooled=%d (at most %d pooled, %d fields in all)", who, d->n_single, d->n_pooled,
              MML_MAX_POOLED, MML_MAX_FIELDS);
  for (int t = 0; t < d->n_tables; ++t) {
    MML_REQUIRE(d->vocab[t] > 0 && d->vocab[t] <= 0x7fffffff, "%s: vocab[%d]=%lld", who, t, (long long)d->vocab[t]);
    MML_REQUIRE(!need_tables || (d->table[t] && aligned16(d->table[t])), "%s: table %d is null or not 16-byte aligned",
                who, t);
  }
  for (int f = 0; f < d->n_single; ++f)
    MML_REQUIRE(d->s_col[f] >= 0 && d->s_table[f] >= 0 && d->s_table[f] < d->n_tables,
                "%s: single-valued field %d malformed", who, f);
  for (int p = 0; p < d->n_pooled; ++p) {
    MML_REQUIRE(d->p_maxlen[p] >= 1 && d->p_maxlen[p] <= MML_POOL_MAX_LEN, "%s: pooled field %d: maxlen=%d outside [1,%d]",
                who, p, d->p_maxlen[p], MML_POOL_MAX_LEN);
    MML_REQUIRE(d->p_col0[p] >= 0 && d->p_table[p] >= 0 && d->p_table[p] < d->n_tables &&
                    d->p_combiner[p] >= MML_POOL_SUM && d->p_combiner[p] <= MML_POOL_MAX,
                "%s: pooled field %d malformed", who, p);
  }
  return MML_OK;
}

// widest X column any field reads (the caller's ldX must cover it)
static int64_t max_col(const mml_pool_desc* d) {
  int64_t m = -1;
  for (int f = 0; f < d->n_single; ++f) m = d->s_col[f] > m ? d->s_col[f] : m;
  for (int p = 0; p < d->n_pooled; ++p) {
    const int64_t last = (int64_t)d->p_col0[p] + d->p_maxlen[p] - 1;
    m = last > m ? last : m;
    m = d->p_len_col[p] > m ? d->p_len_col[p] : m;
  }
  return m;
}

static bool has_max(const mml_pool_desc* d) {
  for (int p = 0; p < d->n_pooled; ++p)
    if (d->p_combiner[p] == MML_POOL_MAX) return true;
  return false;
}

// workgroups per segment of gather_pool_kernel; returns their number (0: too many)
static int64_t gather_segments(const mml_pool_desc* d, int32_t Nd, int64_t B, int32_t* blk0) {
  const int e4 = d->E / 4;
  const int64_t per_sample = (int64_t)d->n_single * e4 + (Nd + 3) / 4;
  int64_t total = cdiv(B * per_sample, (int64_t)256);
  if (blk0) blk0[0] = 0;
  for (int p = 0; p < d->n_pooled; ++p) {
    if (total > 0x7fffffff) return 0;
    if (blk0) blk0[p + 1] = (int32_t)total;
    total += cdiv(B, (int64_t)pool_block_samples(d->p_maxlen[p], e4));
  }
  if (total > 0x7fffffff) return 0;
  if (blk0) blk0[d->n_pooled + 1] = (int32_t)total;
  return total;
}

extern "C" int64_t mml_gather_pool_wgmax_len(const mml_pool_desc* d, int32_t Nd, int64_t B) {
  if (check_desc(d, false, "mml_gather_pool_wgmax_len") || Nd < 0 || B <= 0) return 0;
  return gather_segments(d, Nd, B, nullptr);
}

extern "C" int mml_gather_pool_fwd(const mml_pool_desc* d, const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd,
                                   int64_t B, float* out, int64_t ldo, uint8_t* argmax, int64_t ldarg, float* wg_max,
                                   int64_t wg_max_len, int32_t* status, mml_stream_t stream) {
  const char* who = "mml_gather_pool_fwd";
  int rc = check_desc(d, true, who);
  if (rc) return rc;
  MML_REQUIRE(B >= 0 && Nd >= 0 && dense_col0 >= 0, "%s: bad sizes B=%lld Nd=%d", who, (long long)B, Nd);
  if (B == 0) return MML_OK;
  MML_REQUIRE(X && out, "%s: null X/out", who);
  const int64_t K0 = (int64_t)(d->n_single + d->n_pooled) * d->E + Nd;
  MML_REQUIRE(ldo >= K0 && ldo % 4 == 0 && aligned16(out), "%s: ldo=%lld must be >= %lld, a multiple of 4, out 16-byte aligned",
              who, (long long)ldo, (long long)K0);
  int64_t need_ld = max_col(d) + 1;
  if (Nd > 0 && dense_col0 + (int64_t)Nd > need_ld) need_ld = dense_col0 + (int64_t)Nd;
  MML_REQUIRE(ldX >= need_ld || B == 1, "%s: ldX=%lld < %lld columns the fields read", who, (long long)ldX,
              (long long)need_ld);
  if (has_max(d))
    MML_REQUIRE(argmax && ldarg >= (int64_t)d->n_pooled * d->E && ldarg % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(argmax) & 3u) == 0,
                "%s: a max field needs argmax (4-byte aligned, ldarg %% 4 == 0, ldarg >= n_pooled * E)", who);
  PoolGatherArgs a{};
  for (int f = 0; f < d->n_single; ++f) {
    a.s_tab[f] = d->table[d->s_table[f]];
    a.s_vocab[f] = (int32_t)d->vocab[d->s_table[f]];
    a.s_col[f] = d->s_col[f];
  }
  for (int p = 0; p < d->n_pooled; ++p) {
    a.p_tab[p] = d->table[d->p_table[p]];
    a.p_vocab[p] = (int32_t)d->vocab[d->p_table[p]];
    a.p_col0[p] = d->p_col0[p];
    a.p_T[p] = d->p_maxlen[p];
    a.p_len_col[p] = d->p_len_col[p] < 0 ? -1 : d->p_len_col[p];
    a.p_comb[p] = d->p_combiner[p];
  }
  const int64_t blocks = gather_segments(d, Nd, B, a.blk0);
  MML_REQUIRE(blocks > 0, "%s: grid too large", who);
  MML_REQUIRE(!wg_max || wg_max_len == blocks, "%s: wg_max_len must be mml_gather_pool_wgmax_len() = %lld", who,
              (long long)blocks);
  a.X = X; a.ldX = ldX; a.B = B; a.ldo = ldo; a.ldarg = ldarg; a.F = d->n_single; a.P = d->n_pooled; a.E = d->E;
  a.dense_col0 = dense_col0; a.Nd = Nd; a.out = out; a.argmax = argmax; a.wgmax = wg_max; a.status = status;
  if (wg_max) MML_LAUNCH(gather_pool_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, to_stream(stream), a);
  else MML_LAUNCH(gather_pool_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, to_stream(stream), a);
  return check_launch(who);
}

// fields of the scatter / index pass; chunk > 0: blocks of the fold kernel (chunk lookups each), 0: of the mark kernel
static int fill_pool_fields(const mml_pool_desc* d, int64_t B, int chunk, PoolFields& fd, const char* who) {
  int64_t total = 0;
  const int nf = d->n_single + d->n_pooled;
  for (int f = 0; f < nf; ++f) {
    const int p = f - d->n_single;
    const int T = p < 0 ? 1 : d->p_maxlen[p];
    fd.col[f] = p < 0 ? d->s_col[f] : d->p_col0[p];
    fd.len_col[f] = (p < 0 || d->p_len_col[p] < 0) ? -1 : d->p_len_col[p];
    fd.T[f] = (uint16_t)T;
    fd.table[f] = (uint8_t)(p < 0 ? d->s_table[f] : d->p_table[p]);
    fd.kind[f] = (uint8_t)(p < 0 ? 0 : 1 + d->p_combiner[p]);
    fd.blk0[f] = (int32_t)total;
    if (chunk > 0) {
      total += cdiv(B, (int64_t)(chunk / T));
    } else {
      int64_t nb = cdiv(B * T, (int64_t)256);
      total += nb > 4096 ? 4096 : nb;
    }
    MML_REQUIRE(total <= 0x7fffffff, "%s: grid too large", who);
  }
  fd.blk0[nf] = (int32_t)total;
  fd.nf = nf;
  fd.F = d->n_single;
  return MML_OK;
}

// per TABLE: gradient rows, size and the first byte of its range in the mark map (row_marks of mml_scatter_pool_bwd)
static void fill_pool_tables(const mml_pool_desc* d, PoolScatterArgs& a) {
  mark_bases(d->vocab, d->n_tables, a.markbase);
  for (int t = 0; t < d->n_tables; ++t) {
    a.gtab[t] = d->table[t];
    a.vocab[t] = (int32_t)d->vocab[t];
  }
}

static int pool_rows_impl(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B, const float* dOut,
                          int64_t ldo, const uint8_t* argmax, int64_t ldarg, uint32_t* const* seen,
                          const int64_t* rowbase, int32_t* touched, int32_t* touched_count, int32_t touched_cap,
                          uint8_t* row_marks, int32_t* status, mml_stream_t stream, const char* who) {
  MML_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
  MML_REQUIRE(!touched || (seen && rowbase && touched_count && touched_cap > 0),
              "%s: touched list needs seen/rowbase/touched_count/cap", who);
  if (touched)
    for (int t = 0; t < d->n_tables; ++t) MML_REQUIRE(seen[t] != nullptr, "%s: seen[%d] is null", who, t);
  hipStream_t st = to_stream(stream);
  if (B == 0)  // an empty batch touches no row: the list of the previous call must not survive
    return touched ? clear_touched(touched_count, st, who) : MML_OK;
  MML_REQUIRE(X != nullptr, "%s: null X", who);
  MML_REQUIRE(ldX >= max_col(d) + 1 || B == 1, "%s: ldX=%lld < %lld columns the fields read", who, (long long)ldX,
              (long long)(max_col(d) + 1));
  PoolScatterArgs a{};
  fill_pool_tables(d, a);
  for (int t = 0; t < d->n_tables; ++t) a.seen[t] = touched ? seen[t] : nullptr;
  a.X = X; a.dOut = dOut; a.argmax = argmax; a.ldX = ldX; a.B = B; a.ldo = ldo; a.ldarg = ldarg;
  a.marks = row_marks; a.want_seen = touched ? 1 : 0; a.status = status;
  PoolFields fd{};
  int rc;
  if (!dOut && row_marks) {
    rc = fill_pool_fields(d, B, 0, fd, who);
    if (rc) return rc;
    MML_LAUNCH(mark_pool_rows_kernel, dim3((unsigned)fd.blk0[fd.nf]), dim3(256), 0, st, fd, a);
    rc = check_launch(who);
  } else {
    const int slots = d->E == 16 ? 512 : 1024;
    rc = fill_pool_fields(d, B, slots / 2, fd, who);
    if (rc) return rc;
    if (d->E == 8) rc = launch_pool_fold<1024, 8>(fd, a, fd.blk0[fd.nf], st, who);
    else if (d->E == 4) rc = launch_pool_fold<1024, 4>(fd, a, fd.blk0[fd.nf], st, who);
    else rc = launch_pool_fold<512, 16>(fd, a, fd.blk0[fd.nf], st, who);
  }
  if (rc || !touched) return rc;
  // marks / bitmaps -> the touched list, per table (resets *touched_count itself)
  return mml_rows_compact(seen, d->vocab, rowbase, d->n_tables, touched, touched_count, touched_cap, row_marks, stream);
}

extern "C" int mml_scatter_pool_bwd(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B, const float* dOut,
                                    int64_t ldo, const uint8_t* argmax, int64_t ldarg, uint32_t* const* seen,
                                    const int64_t* rowbase, int32_t* touched, int32_t* touched_count,
                                    int32_t touched_cap, uint8_t* row_marks, int32_t* status, mml_stream_t stream) {
  const char* who = "mml_scatter_pool_bwd";
  int rc = check_desc(d, true, who);
  if (rc) return rc;
  if (B > 0) {
    MML_REQUIRE(dOut && aligned16(dOut) && ldo % 4 == 0 && ldo >= (int64_t)(d->n_single + d->n_pooled) * d->E,
                "%s: dOut must be 16-byte aligned with ldo %% 4 == 0 and ldo >= (n_single + n_pooled) * E", who);
    if (has_max(d))
      MML_REQUIRE(argmax && ldarg >= (int64_t)d->n_pooled * d->E && ldarg % 4 == 0 &&
                      (reinterpret_cast<uintptr_t>(argmax) & 3u) == 0,
                  "%s: a max field needs the argmax bytes of mml_gather_pool_fwd", who);
  }
  return pool_rows_impl(d, X, ldX, B, dOut, ldo, argmax, ldarg, seen, rowbase, touched, touched_count, touched_cap,
                        row_marks, status, stream, who);
}

// headroom of the deterministic totals: a row of table tb may receive B * L_tb addends at the launch-wide maximum,
// L_tb = its single-valued fields + the maxlen of its pooled fields: 24 significand bits + shift + ceil(log2(B * Lmax)) < 63
extern "C" int32_t mml_scatter_pool_det_shift(const mml_pool_desc* d, int64_t B) {
  if (check_desc(d, false, "mml_scatter_pool_det_shift") || B < 0) return -1;
  int64_t per_table[MML_MAX_FIELDS] = {0};
  for (int f = 0; f < d->n_single; ++f) per_table[d->s_table[f]] += 1;
  for (int p = 0; p < d->n_pooled; ++p) per_table[d->p_table[p]] += d->p_maxlen[p];
  int64_t lmax = 1;
  for (int t = 0; t < d->n_tables; ++t) lmax = per_table[t] > lmax ? per_table[t] : lmax;
  if (B > ((int64_t)1 << 40)) return -1;  // (lmax < 2^13: the product below stays far inside 64 bits)
  const int64_t n = (B < 1 ? 1 : B) * lmax;
  int lg = 0;
  while (((int64_t)1 << lg) < n) ++lg;
  const int shift = 62 - 24 - lg;
  if (shift < 4) return -1;
  return shift > 28 ? 28 : shift;
}

extern "C" int mml_scatter_pool_bwd_det(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B,
                                        const float* dOut, int64_t ldo, const uint8_t* argmax, int64_t ldarg,
                                        int64_t* const* acc64, uint32_t* amax_slot, uint8_t* row_marks, int32_t flags,
                                        int32_t* status, mml_stream_t stream) {
  const char* who = "mml_scatter_pool_bwd_det";
  int rc = check_desc(d, true, who);
  if (rc) return rc;
  MML_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
  MML_REQUIRE(acc64 && amax_slot && row_marks, "%s: acc64, amax_slot and row_marks are required", who);
  for (int t = 0; t < d->n_tables; ++t) MML_REQUIRE(acc64[t], "%s: acc64[%d] is null", who, t);
  bool defer;
  int clear_marks;
  rc = det_flags(flags, who, &defer, &clear_marks);
  if (rc) return rc;
  const int shift = mml_scatter_pool_det_shift(d, B);
  MML_REQUIRE(shift >= 0, "%s: B=%lld samples times the lookups of one table leave no headroom in the 64-bit totals", who,
              (long long)B);
  if (B == 0) return MML_OK;
  const int64_t ncols = (int64_t)(d->n_single + d->n_pooled) * d->E;
  MML_REQUIRE(X != nullptr, "%s: null X", who);
  MML_REQUIRE(ldX >= max_col(d) + 1 || B == 1, "%s: ldX=%lld < %lld columns the fields read", who, (long long)ldX,
              (long long)(max_col(d) + 1));
  MML_REQUIRE(dOut && aligned16(dOut) && ldo % 4 == 0 && ldo >= ncols,
              "%s: dOut must be 16-byte aligned with ldo %% 4 == 0 and ldo >= (n_single + n_pooled) * E", who);
  if (has_max(d))
    MML_REQUIRE(argmax && ldarg >= (int64_t)d->n_pooled * d->E && ldarg % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(argmax) & 3u) == 0,
                "%s: a max field needs the argmax bytes of mml_gather_pool_fwd", who);
  hipStream_t st = to_stream(stream);
  if (!(flags & MML_SCATTER_DET_AMAX_SUPPLIED)) {
    rc = measure_dout(dOut, B, ldo, ncols, amax_slot, stream);
    if (rc) return rc;
  }
  PoolScatterArgs a{};
  DetFinalArgs fa{};
  fill_pool_tables(d, a);
  for (int t = 0; t < d->n_tables; ++t) {
    a.acc64[t] = reinterpret_cast<long long*>(acc64[t]);
    fa.gtab[t] = a.gtab[t];
    fa.acc64[t] = a.acc64[t];
    fa.vocab[t] = d->vocab[t];
    fa.markbase[t] = a.markbase[t];
  }
  a.X = X; a.dOut = dOut; a.argmax = argmax; a.ldX = ldX; a.B = B; a.ldo = ldo; a.ldarg = ldarg;
  a.marks = row_marks; a.status = status; a.amax_dout = amax_slot; a.fix_shift = shift;
  PoolFields fd{};
  const int slots = d->E == 16 ? 512 : 1024;
  rc = fill_pool_fields(d, B, slots / 2, fd, who);
  if (rc) return rc;
  if (d->E == 8) rc = launch_pool_fold<1024, 8, true>(fd, a, fd.blk0[fd.nf], st, who);
  else if (d->E == 4) rc = launch_pool_fold<1024, 4, true>(fd, a, fd.blk0[fd.nf], st, who);
  else rc = launch_pool_fold<512, 16, true>(fd, a, fd.blk0[fd.nf], st, who);
  if (rc || defer) return rc;  // (deferred: mml_opt_step_dense converts the marked rows' totals, mml_opt_tensor.acc64)
  fa.marks = row_marks; fa.amax_dout = amax_slot; fa.F = d->n_tables; fa.E = d->E; fa.fix_shift = shift;
  fa.clear_marks = clear_marks;
  return launch_det_finalize(fa, st, who);
}

extern "C" int mml_index_unique_pool(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B,
                                     uint32_t* const* seen, const int64_t* rowbase, int32_t* touched,
                                     int32_t* touched_count, int32_t touched_cap, uint8_t* row_marks, int32_t* status,
                                     mml_stream_t stream) {
  const char* who = "mml_index_unique_pool";
  int rc = check_desc(d, false, who);
  if (rc) return rc;
  MML_REQUIRE(seen && rowbase && touched && touched_count && touched_cap > 0, "%s: bad arguments", who);
  return pool_rows_impl(d, X, ldX, B, nullptr, 0, nullptr, 0, seen, rowbase, touched, touched_count, touched_cap,
                        row_marks, status, stream, who);
}
