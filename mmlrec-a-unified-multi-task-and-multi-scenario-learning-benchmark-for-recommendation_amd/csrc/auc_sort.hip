// Whole-set AUC on the device: a multi-workgroup LSD radix sort plus an integer Mann-Whitney sweep (mml_auc_sorted).
//
// mml_auc_segments (metrics.hip) sorts one segment inside ONE workgroup's LDS, so it stops at 4096 rows.  evaluate()
// scores a whole validation set and fit() at batch 65 536 scores 65 536-row segments; both need a sort that spans
// workgroups.  A problem is one (segment, column) pair; every kernel below takes all problems of a call in one grid.
//
//   build     key = image(pred) << 1 | label, 64 bits, one per row and column (layout [cols][n]: a problem's keys are
//             contiguous).  image = the order-preserving 32-bit picture of the fp32 score (sign flip, -0 -> +0).  A row
//             the mask leaves out gets image 0xffffffff (above every finite score) and the SKIP bit: it sorts last and
//             counts for nothing.  A non-finite score at a participating row marks the problem bad (NaN, status bit 4).
//   4 passes  8-bit digits of the image, least significant first.  Per pass:
//               hist     every workgroup owns one block of KB consecutive keys (KB a multiple of the 4096-key tile, at
//                        most 512 blocks per problem) and counts its digits (integer LDS adds into per-wave
//                        counters): hist[problem][block][256]
//               scan     one workgroup per problem turns the counts into exclusive offsets, digit-major then block
//               scatter  the block walks its tiles in order; inside a tile every wave ranks 64 keys at a time with
//                        ballots (lanes with the same digit: rank = lower lanes among them), so the rank is STABLE; the
//                        tile is reordered in LDS first, so that the global stores run along each digit's destination
//   sweep     over the sorted keys, with B(i) = "image(i) differs from image(i-1)" and gN / gP = negatives / positives
//             in front of the tie group of i:
//                 S1 = sum over positives of gN,  S2 = sum over negatives of gP,  2U = S1 + P*N - S2
//             (sum over positives of #neg(<=) equals sum over negatives of #pos(>=) = P*N - S2: one forward direction
//             serves both halves of sklearn's half credit).  One wave sweeps one chunk of consecutive keys with ballots
//             and popcounts only; chunk summaries, one scan per problem over the chunks, then the accumulating sweep.
// Every sum is an integer sum (S1 / S2: one slot per chunk, added up per problem; no atomics besides the flag of a
// non-finite score), so the result is bitwise repeatable and does not depend on the order of the rows.  Nothing is
// allocated or synchronised: the caller owns the workspace (mml_auc_sorted_workspace_bytes), and the call can be
// captured into a HIP graph.
//
// LDS per workgroup: scatter 4096 * 8 B (tile) + 4 * 256 * 4 B (wave counters) + 3 * 256 * 4 B = 39 KiB (four fit the
// CU's 160 KiB; the registers of the 16 keys and ranks a thread holds bound the occupancy first); hist 4 KiB; the scans
// 1-2 KiB.
#include "common.hpp"

namespace mml {

constexpr int AS_THREADS = 256;
constexpr int AS_WAVES = AS_THREADS / 64;
constexpr int AS_KPT = 16;                       // keys per thread and tile
constexpr int AS_TILE = AS_THREADS * AS_KPT;     // 4096
constexpr int AS_WCHUNK = 64 * AS_KPT;           // keys of one wave inside a tile
constexpr int AS_MAX_BLOCKS = 512;               // per problem
constexpr int AS_MAX_CHUNKS = 4096;              // sweep chunks per problem (one wave each)
constexpr int AS_MIN_CHUNK = 1024;
constexpr uint64_t AS_SKIP = 1ull << 33;
constexpr int AS_STATUS_NONFINITE = 16;          // bit 4 of *status

struct AucGeom {
  int64_t n, seg;        // rows, rows per segment (1 <= seg <= n)
  int64_t nseg, nprob;   // segments, problems = nseg * cols
  int64_t KB, NB;        // keys per block (multiple of AS_TILE), blocks per problem
  int64_t CK, NC;        // keys per sweep chunk (multiple of 64), chunks per problem
  int32_t cols;
};

__device__ __forceinline__ uint32_t auc_image(float p) {
  if (p == 0.f) p = 0.f;  // -0 and +0 are one tie group
  const uint32_t u = __float_as_uint(p);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// first key and length of problem q
__device__ __forceinline__ void problem_span(const AucGeom& g, int64_t q, int64_t& base, int64_t& len) {
  const int64_t s = q / g.cols, c = q - s * g.cols;
  const int64_t r0 = s * g.seg;
  len = (g.n - r0 < g.seg) ? (g.n - r0) : g.seg;
  base = c * g.n + r0;
}

// exclusive scan over AS_THREADS values (Hillis-Steele in LDS); OP 0 = add, 1 = max.  *total = the reduction of all.
template <int OP>
__device__ __forceinline__ uint32_t as_block_scan_excl(uint32_t v, uint32_t* tmp, uint32_t* total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int d = 1; d < AS_THREADS; d <<= 1) {
    const uint32_t o = (t >= d) ? tmp[t - d] : 0u;
    __syncthreads();
    if (t >= d) tmp[t] = OP ? (tmp[t] > o ? tmp[t] : o) : tmp[t] + o;
    __syncthreads();
  }
  const uint32_t ex = t ? tmp[t - 1] : 0u;
  if (total) *total = tmp[AS_THREADS - 1];
  __syncthreads();
  return ex;
}

// ---- build ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_THREADS) void auc_build_keys_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                    const float* __restrict__ y, int64_t ldy,
                                                                    const float* __restrict__ mask, int64_t ldm,
                                                                    int mask_cols, AucGeom g, uint64_t* __restrict__ keys,
                                                                    uint32_t* bad, int32_t* status) {
  const int64_t total = g.n * g.cols;
  for (int64_t i = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * AS_THREADS) {
    const int64_t r = i / g.cols;
    const int c = (int)(i - r * g.cols);
    bool take = true;
    if (mask) take = mask[r * ldm + (mask_cols == 1 ? 0 : c)] != 0.f;
    uint64_t k = (0xffffffffull << 1) | AS_SKIP;
    if (take) {
      const float p = pred[r * ldp + c];
      const uint32_t lab = y[r * ldy + c] > 0.5f ? 1u : 0u;
      k = ((uint64_t)auc_image(p) << 1) | lab;
      if ((__float_as_uint(p) & 0x7f800000u) == 0x7f800000u) {  // NaN or infinite
        atomicOr(&bad[(r / g.seg) * g.cols + c], 1u);
        atomicOr(status, AS_STATUS_NONFINITE);
      }
    }
    keys[(int64_t)c * g.n + r] = k;
  }
}

// ---- stable rank of a wave's 64 digits ----------------------------------------------------------------------------
// cntw: this wave's 256 digit counters in LDS.  Returns the number of earlier keys of this wave (earlier calls and
// lower lanes) with the same digit, and counts the 64 keys in.  Lanes with valid == false take no part.
__device__ __forceinline__ uint32_t wave_digit_rank(uint32_t digit, bool valid, volatile uint32_t* cntw) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  const uint64_t lt = (1ull << (threadIdx.x & 63)) - 1ull;
  const uint32_t r = (uint32_t)__popcll(m & lt);
  uint32_t pre = 0;
  if (valid) pre = cntw[digit];
  __builtin_amdgcn_wave_barrier();
  if (valid && r == 0) cntw[digit] = pre + (uint32_t)__popcll(m);
  __builtin_amdgcn_wave_barrier();
  return pre + r;
}

__device__ __forceinline__ uint32_t key_digit(uint64_t k, int shift) { return (uint32_t)(k >> shift) & 255u; }

// ---- histogram of one block's digits --------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_THREADS) void auc_hist_kernel(const uint64_t* __restrict__ keys, AucGeom g, int shift,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[AS_WAVES][256];
  const int64_t q = blockIdx.x / g.NB, b = blockIdx.x - q * g.NB;
  int64_t base, len;
  problem_span(g, q, base, len);
  const int64_t k0 = b * g.KB;
  const int64_t blen = (len - k0 < g.KB) ? (len - k0) : g.KB;  // may be <= 0 (short last segment)
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (int i = 0; i < AS_WAVES; ++i) cnt[i][t] = 0u;
  __syncthreads();
  // wave w takes the 64-key groups w, w + 4, ... of the block (a count needs no order)
  for (int64_t i0 = (int64_t)w * 64; i0 < blen; i0 += AS_THREADS) {
    const int64_t i = i0 + lane;
    const bool valid = i < blen;
    // a count needs no rank: one LDS integer add per key into the wave's own counters
    if (valid) atomicAdd(&cnt[w][key_digit(keys[base + k0 + i], shift)], 1u);
  }
  __syncthreads();
  hist[((int64_t)blockIdx.x << 8) + t] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}

// ---- offsets: hist[q][b][d] -> keys of digit d in blocks < b; dbase[q][d] -> keys of digits < d ---------------------
__global__ __launch_bounds__(AS_THREADS) void auc_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ dbase,
                                                              AucGeom g) {
  __shared__ uint32_t tmp[AS_THREADS];
  const int64_t q = blockIdx.x;
  const int t = threadIdx.x;
  uint32_t* h = hist + ((q * g.NB) << 8) + t;
  uint32_t run = 0;
  int64_t b = 0;
  for (; b + 8 <= g.NB; b += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = h[(b + j) << 8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      h[(b + j) << 8] = run;
      run += v[j];
    }
  }
  for (; b < g.NB; ++b) {
    const uint32_t v = h[b << 8];
    h[b << 8] = run;
    run += v;
  }
  dbase[(q << 8) + t] = as_block_scan_excl<0>(run, tmp, nullptr);
}

// ---- stable scatter of one block ------------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_THREADS) void auc_scatter_kernel(const uint64_t* __restrict__ src,
                                                                 uint64_t* __restrict__ dst, AucGeom g, int shift,
                                                                 const uint32_t* __restrict__ hist,
                                                                 const uint32_t* __restrict__ dbase) {
  __shared__ uint64_t skeys[AS_TILE];
  __shared__ uint32_t cnt[AS_WAVES][256];
  __shared__ uint32_t tstart[256];  // first tile-local position of a digit
  __shared__ uint32_t goff[256];    // destination of a digit's first key of this tile, minus tstart (wraps)
  __shared__ uint32_t tmp[AS_THREADS];
  const int64_t q = blockIdx.x / g.NB, b = blockIdx.x - q * g.NB;
  int64_t base, len;
  problem_span(g, q, base, len);
  const int64_t k0 = b * g.KB;
  const int64_t blen = (len - k0 < g.KB) ? (len - k0) : g.KB;
  if (blen <= 0) return;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  uint32_t gbase = dbase[(q << 8) + t] + hist[((int64_t)blockIdx.x << 8) + t];  // thread t owns digit t
  for (int64_t t0 = 0; t0 < blen; t0 += AS_TILE) {
    const int tlen = (int)((blen - t0 < AS_TILE) ? (blen - t0) : AS_TILE);
    for (int i = 0; i < AS_WAVES; ++i) cnt[i][t] = 0u;
    __syncthreads();
    uint64_t key[AS_KPT];
    uint32_t rank[AS_KPT];
#pragma unroll
    for (int it = 0; it < AS_KPT; ++it) {
      const int i = w * AS_WCHUNK + it * 64 + lane;  // tile-local, in the order of the source
      const bool valid = i < tlen;
      key[it] = valid ? src[base + k0 + t0 + i] : 0ull;
      rank[it] = wave_digit_rank(key_digit(key[it], shift), valid, cnt[w]);
    }
    __syncthreads();
    {  // digit t: counts of the waves -> exclusive over waves; tile start of the digit
      uint32_t c[AS_WAVES], tot = 0;
      for (int i = 0; i < AS_WAVES; ++i) {
        c[i] = cnt[i][t];
        cnt[i][t] = tot;
        tot += c[i];
      }
      const uint32_t ts = as_block_scan_excl<0>(tot, tmp, nullptr);
      tstart[t] = ts;
      goff[t] = gbase - ts;
      gbase += tot;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < AS_KPT; ++it) {
      const int i = w * AS_WCHUNK + it * 64 + lane;
      if (i < tlen) {
        const uint32_t d = key_digit(key[it], shift);
        const uint32_t pos = tstart[d] + cnt[w][d] + rank[it];
        if (pos < (uint32_t)AS_TILE) skeys[pos] = key[it];
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < AS_KPT; ++it) {
      const int i = it * AS_THREADS + t;
      if (i < tlen) {
        const uint64_t k = skeys[i];
        const uint32_t at = goff[key_digit(k, shift)] + (uint32_t)i;  // position inside the problem
        if ((int64_t)at < len) dst[base + at] = k;
      }
    }
    __syncthreads();
  }
}

// ---- sweep over the sorted keys -------------------------------------------------------------------------------------
// One wave walks [i0, i1) of a problem's sorted keys.  State: cn / cp = negatives / positives seen, gN / gP = their
// values at the start of the current tie group.  ACCUM == false: starts from zero and reports the chunk's summary
// (counts; whether a group starts inside; gN / gP at the last group start, relative to the chunk).  ACCUM == true:
// starts from the scanned values and adds up S1 / S2.
template <bool ACCUM>
__device__ __forceinline__ void wave_sweep(const uint64_t* __restrict__ keys, int64_t i0, int64_t i1, uint32_t& cn,
                                           uint32_t& cp, uint32_t& gN, uint32_t& gP, bool& any_start, uint64_t& s1,
                                           uint64_t& s2) {
  const int lane = threadIdx.x & 63;
  const uint64_t le = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
  for (int64_t j0 = i0; j0 < i1; j0 += 64) {
    const int64_t i = j0 + lane;
    const bool valid = i < i1;
    const uint64_t k = valid ? keys[i] : 0ull;
    const bool live = valid && !(k & AS_SKIP);
    const bool start = valid && (i == 0 || (keys[i - 1] >> 1) != (k >> 1));
    const bool pos = live && (k & 1ull), neg = live && !(k & 1ull);
    const uint64_t mN = __ballot(neg), mP = __ballot(pos), mB = __ballot(start);
    if (ACCUM) {
      const uint64_t m = mB & le;
      uint32_t myN = gN, myP = gP;
      if (m) {
        const uint64_t below = (1ull << (63 - __clzll((long long)m))) - 1ull;
        myN = cn + (uint32_t)__popcll(mN & below);
        myP = cp + (uint32_t)__popcll(mP & below);
      }
      if (pos) s1 += myN;
      if (neg) s2 += myP;
    }
    if (mB) {
      const uint64_t below = (1ull << (63 - __clzll((long long)mB))) - 1ull;
      gN = cn + (uint32_t)__popcll(mN & below);
      gP = cp + (uint32_t)__popcll(mP & below);
      any_start = true;
    }
    cn += (uint32_t)__popcll(mN);
    cp += (uint32_t)__popcll(mP);
  }
}

// chunk arrays, each [nprob * NC]: 0 negatives, 1 positives, 2 group start inside, 3 / 4 gN / gP at the last start
__global__ __launch_bounds__(AS_THREADS) void auc_chunk_summary_kernel(const uint64_t* __restrict__ keys, AucGeom g,
                                                                       uint32_t* __restrict__ summ) {
  const int64_t wid = (int64_t)blockIdx.x * AS_WAVES + (threadIdx.x >> 6);
  const int64_t total = g.nprob * g.NC;
  if (wid >= total) return;
  const int64_t q = wid / g.NC, c = wid - q * g.NC;
  int64_t base, len;
  problem_span(g, q, base, len);
  const int64_t i0 = c * g.CK, i1 = (len < i0 + g.CK) ? len : i0 + g.CK;
  uint32_t cn = 0, cp = 0, gN = 0, gP = 0;
  bool any = false;
  uint64_t s1 = 0, s2 = 0;
  if (i0 < i1) wave_sweep<false>(keys + base, i0, i1, cn, cp, gN, gP, any, s1, s2);
  if ((threadIdx.x & 63) == 0) {
    summ[wid] = cn;
    summ[total + wid] = cp;
    summ[2 * total + wid] = any ? 1u : 0u;
    summ[3 * total + wid] = gN;
    summ[4 * total + wid] = gP;
  }
}

// per problem: summaries -> what each chunk starts from (arrays 0 / 1: negatives / positives in front of the chunk,
// 3 / 4: gN / gP in front of it); pn[q] = {P, N}
__global__ __launch_bounds__(AS_THREADS) void auc_chunk_scan_kernel(uint32_t* __restrict__ summ, AucGeom g,
                                                                    uint64_t* __restrict__ pn) {
  __shared__ uint32_t tmp[AS_THREADS];
  const int64_t q = blockIdx.x, total = g.nprob * g.NC;
  const int t = threadIdx.x;
  const int64_t per = (g.NC + AS_THREADS - 1) / AS_THREADS;
  const int64_t c0 = (int64_t)t * per, c1 = (c0 + per < g.NC) ? c0 + per : g.NC;
  uint32_t *sn = summ + q * g.NC, *sp = sn + total, *sf = sp + total, *sgn = sf + total, *sgp = sgn + total;
  uint32_t an = 0, ap = 0;
  for (int64_t c = c0; c < c1; ++c) {
    an += sn[c];
    ap += sp[c];
  }
  uint32_t N, P;
  uint32_t bn = as_block_scan_excl<0>(an, tmp, &N);
  uint32_t bp = as_block_scan_excl<0>(ap, tmp, &P);
  // counts are monotone along the keys, so the value at the LAST group start is the maximum over all starts so far
  uint32_t mN = 0, mP = 0;
  {
    uint32_t rn = bn, rp = bp;
    for (int64_t c = c0; c < c1; ++c) {
      if (sf[c]) {
        mN = rn + sgn[c];
        mP = rp + sgp[c];
      }
      rn += sn[c];
      rp += sp[c];
    }
  }
  uint32_t gN = as_block_scan_excl<1>(mN, tmp, nullptr);
  uint32_t gP = as_block_scan_excl<1>(mP, tmp, nullptr);
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t n_c = sn[c], p_c = sp[c], f = sf[c], rn_c = sgn[c], rp_c = sgp[c];
    sn[c] = bn;
    sp[c] = bp;
    sgn[c] = gN;
    sgp[c] = gP;
    if (f) {
      gN = bn + rn_c;
      gP = bp + rp_c;
    }
    bn += n_c;
    bp += p_c;
  }
  if (t == 0) {
    pn[2 * q] = P;
    pn[2 * q + 1] = N;
  }
}

// part[2 * (q * NC + c) + {0, 1}] = the chunk's share of S1 / S2 (every chunk writes its own slot: no atomics)
__global__ __launch_bounds__(AS_THREADS) void auc_chunk_accum_kernel(const uint64_t* __restrict__ keys, AucGeom g,
                                                                     const uint32_t* __restrict__ summ,
                                                                     uint64_t* __restrict__ part) {
  const int64_t wid = (int64_t)blockIdx.x * AS_WAVES + (threadIdx.x >> 6);
  const int64_t total = g.nprob * g.NC;
  if (wid >= total) return;
  const int64_t q = wid / g.NC, c = wid - q * g.NC;
  int64_t base, len;
  problem_span(g, q, base, len);
  const int64_t i0 = c * g.CK, i1 = (len < i0 + g.CK) ? len : i0 + g.CK;
  uint64_t s1 = 0, s2 = 0;
  if (i0 < i1) {
    uint32_t cn = summ[wid], cp = summ[total + wid], gN = summ[3 * total + wid], gP = summ[4 * total + wid];
    bool any = false;
    wave_sweep<true>(keys + base, i0, i1, cn, cp, gN, gP, any, s1, s2);
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_down(s1, o);
      s2 += __shfl_down(s2, o);
    }
  }
  if ((threadIdx.x & 63) == 0) {
    part[2 * wid] = s1;
    part[2 * wid + 1] = s2;
  }
}

// one workgroup per problem: S1 / S2 = the sums of the chunks' shares (integers: any order gives the same bits)
__global__ __launch_bounds__(AS_THREADS) void auc_finalize_kernel(const uint64_t* __restrict__ part,
                                                                  const uint64_t* __restrict__ pn,
                                                                  const uint32_t* __restrict__ bad, AucGeom g,
                                                                  double* __restrict__ auc, int64_t* __restrict__ counts) {
  __shared__ uint64_t red[2][AS_THREADS];
  const int64_t q = blockIdx.x;
  const int t = threadIdx.x;
  uint64_t s1 = 0, s2 = 0;
  for (int64_t c = t; c < g.NC; c += AS_THREADS) {
    s1 += part[2 * (q * g.NC + c)];
    s2 += part[2 * (q * g.NC + c) + 1];
  }
  red[0][t] = s1;
  red[1][t] = s2;
  __syncthreads();
  for (int d = AS_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      red[0][t] += red[0][t + d];
      red[1][t] += red[1][t + d];
    }
    __syncthreads();
  }
  if (t != 0) return;
  const uint64_t P = pn[2 * q], N = pn[2 * q + 1];
  const uint64_t u2 = red[0][0] + P * N - red[1][0];
  const double npos = (double)P, nn = (double)N;
  auc[q] = (P == 0 || N == 0 || bad[q]) ? __longlong_as_double(0x7ff8000000000000ll) : (double)u2 / (2.0 * npos * nn);
  if (counts) {
    counts[3 * q] = (int64_t)u2;
    counts[3 * q + 1] = (int64_t)P;
    counts[3 * q + 2] = (int64_t)N;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static inline int64_t round_up(int64_t a, int64_t m) { return cdiv(a, m) * m; }

static AucGeom auc_geometry(int64_t n, int32_t cols, int64_t seg) {
  AucGeom g;
  g.n = n;
  g.cols = cols;
  g.seg = (seg <= 0 || seg >= n) ? n : seg;
  g.nseg = cdiv(n, g.seg);
  g.nprob = g.nseg * cols;
  g.KB = round_up(cdiv(g.seg, (int64_t)AS_MAX_BLOCKS), AS_TILE);
  g.NB = cdiv(g.seg, g.KB);
  const int64_t ck = round_up(cdiv(g.seg, (int64_t)AS_MAX_CHUNKS), 64);
  g.CK = ck < AS_MIN_CHUNK ? AS_MIN_CHUNK : ck;
  g.NC = cdiv(g.seg, g.CK);
  return g;
}

struct AucWorkspace {
  int64_t keys_a, keys_b, hist, dbase, summ, part, bad, pn, end;  // byte offsets; `bad` is cleared per call
};

static AucWorkspace auc_workspace(const AucGeom& g) {
  AucWorkspace w;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += round_up(bytes, 256);
    return at;
  };
  const int64_t K = g.n * g.cols;
  w.keys_a = take(K * 8);
  w.keys_b = take(K * 8);
  w.hist = take(g.nprob * g.NB * 256 * 4);
  w.dbase = take(g.nprob * 256 * 4);
  w.summ = take(5 * g.nprob * g.NC * 4);
  w.part = take(g.nprob * g.NC * 16);
  w.bad = take(g.nprob * 4);
  w.pn = take(g.nprob * 16);
  w.end = o;
  return w;
}

static bool auc_extents_ok(int64_t n, int32_t cols) {
  return n >= 0 && cols >= 1 && (n == 0 || n <= (int64_t)0x7fffffff / cols) && n * (int64_t)cols < (int64_t)0x80000000ll;
}

}  // namespace mml

using namespace mml;

extern "C" int32_t mml_auc_sorted_tile(void) { return AS_TILE; }

extern "C" int64_t mml_auc_sorted_workspace_bytes(int64_t n, int32_t cols, int64_t seg) {
  if (!auc_extents_ok(n, cols) || seg < 0) return -1;
  if (n == 0) return 0;
  return auc_workspace(auc_geometry(n, cols, seg)).end;
}

extern "C" int mml_auc_sorted(const float* pred, int64_t ldp, const float* y, int64_t ldy, const float* mask,
                              int64_t ldm, int32_t mask_cols, int64_t n, int32_t cols, int64_t seg, void* workspace,
                              int64_t workspace_bytes, double* auc, int64_t* counts, int32_t* status,
                              mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && cols >= 1 && seg >= 0, "mml_auc_sorted: bad extents n=%lld cols=%d seg=%lld", (long long)n, cols,
              (long long)seg);
  MML_REQUIRE(auc_extents_ok(n, cols), "mml_auc_sorted: n * cols = %lld * %d keys, the call takes fewer than 2^31",
              (long long)n, cols);
  if (mask) MML_REQUIRE(mask_cols == 1 || mask_cols == cols, "mml_auc_sorted: mask_cols = %d, expected 1 or cols = %d",
                        mask_cols, cols);
  if (n == 0) return MML_OK;
  MML_REQUIRE(pred && y && auc && status && ldp >= cols && ldy >= cols,
              "mml_auc_sorted: null pointer or leading dimension < cols");
  if (mask) MML_REQUIRE(ldm >= mask_cols, "mml_auc_sorted: mask leading dimension < mask_cols");
  const AucGeom g = auc_geometry(n, cols, seg);
  const AucWorkspace w = auc_workspace(g);
  MML_REQUIRE(workspace && workspace_bytes >= w.end, "mml_auc_sorted: workspace of %lld bytes, %lld needed",
              (long long)workspace_bytes, (long long)w.end);
  MML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "mml_auc_sorted: workspace not 8-byte aligned");
  const int64_t nblocks = g.nprob * g.NB, nchunkwg = cdiv(g.nprob * g.NC, (int64_t)AS_WAVES);
  MML_REQUIRE(nblocks <= 0x7fffffff && nchunkwg <= 0x7fffffff && g.nprob <= 0x7fffffff, "mml_auc_sorted: grid too large");
  hipStream_t st = to_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint64_t* ka = reinterpret_cast<uint64_t*>(ws + w.keys_a);
  uint64_t* kb = reinterpret_cast<uint64_t*>(ws + w.keys_b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + w.hist);
  uint32_t* dbase = reinterpret_cast<uint32_t*>(ws + w.dbase);
  uint32_t* summ = reinterpret_cast<uint32_t*>(ws + w.summ);
  uint64_t* part = reinterpret_cast<uint64_t*>(ws + w.part);
  uint32_t* bad = reinterpret_cast<uint32_t*>(ws + w.bad);
  uint64_t* pn = reinterpret_cast<uint64_t*>(ws + w.pn);
  (void)hipGetLastError();
  if (hipMemsetAsync(bad, 0, (size_t)(w.pn - w.bad), st) != hipSuccess) return check_launch("mml_auc_sorted");
  const int64_t total = n * cols;
  const unsigned bgrid = (unsigned)(cdiv(total, (int64_t)AS_THREADS) < 4096 ? cdiv(total, (int64_t)AS_THREADS) : 4096);
  MML_LAUNCH(auc_build_keys_kernel, dim3(bgrid), dim3(AS_THREADS), 0, st, pred, ldp, y, ldy, mask, ldm, (int)mask_cols, g,
             ka, bad, status);
  uint64_t *src = ka, *dst = kb;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 1 + 8 * pass;
    MML_LAUNCH(auc_hist_kernel, dim3((unsigned)nblocks), dim3(AS_THREADS), 0, st, src, g, shift, hist);
    MML_LAUNCH(auc_scan_kernel, dim3((unsigned)g.nprob), dim3(AS_THREADS), 0, st, hist, dbase, g);
    MML_LAUNCH(auc_scatter_kernel, dim3((unsigned)nblocks), dim3(AS_THREADS), 0, st, src, dst, g, shift, hist, dbase);
    uint64_t* x = src;
    src = dst;
    dst = x;
  }
  // four passes: the sorted keys are back in the first buffer
  MML_LAUNCH(auc_chunk_summary_kernel, dim3((unsigned)nchunkwg), dim3(AS_THREADS), 0, st, src, g, summ);
  MML_LAUNCH(auc_chunk_scan_kernel, dim3((unsigned)g.nprob), dim3(AS_THREADS), 0, st, summ, g, pn);
  MML_LAUNCH(auc_chunk_accum_kernel, dim3((unsigned)nchunkwg), dim3(AS_THREADS), 0, st, src, g, summ, part);
  MML_LAUNCH(auc_finalize_kernel, dim3((unsigned)g.nprob), dim3(AS_THREADS), 0, st, part, pn, bad, g, auc, counts);
  return check_launch("mml_auc_sorted");
}
