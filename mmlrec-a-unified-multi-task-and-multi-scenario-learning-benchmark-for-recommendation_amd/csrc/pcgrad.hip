// PCGrad gradient surgery (reference model/optimizer.py:10-138) over T per-objective gradients, each the flattened
// gradient of every parameter.  The reference's projection loop makes O(T^2) passes over those vectors; every projected
// gradient stays in the span of the T originals, pc_i = sum_k c_ik g_k, so here
//   gram    : ONE pass reads every bank once and accumulates all T (T + 1) / 2 products per element, in double,
//   weights : the loop itself as a recursion on T x T coefficients (one thread, double),
//   combine : one more pass writes out = sum_k w'[k] g_k (fp32, one fma per term, k ascending).
// gram and combine are streaming and HBM-bound (4 T bytes / element read; combine writes 4 more): blockIdx.y = segment,
// blockIdx.x strides over the segment's rows in 16-byte pieces (plus a scalar piece for the cols % 4 tail of a row), or
// over single elements where the pitch or a pointer is not 16-byte aligned.  A segment with row marks reads the row's
// byte first and skips the row when it is 0.  Padding columns [cols, ld) are never touched.
// gram's sums: lane -> wave (xor butterfly) -> workgroup (wave order) -> one partial per workgroup and pair in the
// workspace -> a second kernel adds the partials in index order.  No float atomics: the bits depend on the launch
// geometry (the device's CU count and the shapes) only.
#include "common.hpp"

namespace mml {

constexpr int PCG_BATCH = 24;     // segments per launch (the descriptors travel as kernel arguments: 24 x 104 B)
constexpr int PCG_MAX_GX = 1024;  // most workgroups per segment: the partials of one segment in the workspace
constexpr int PCG_MAXT = MML_PCGRAD_MAX_TASKS;

struct PcgBatch {
  mml_pcgrad_seg s[PCG_BATCH];
  int8_t mean[PCG_BATCH];  // 1: every bank of the segment is non-NULL (combine: the mean weights)
};

__host__ __device__ constexpr int pcg_pairs(int T) { return T * (T + 1) / 2; }

template <int T>
__device__ __forceinline__ bool pcg_vec(const mml_pcgrad_seg& S, bool with_out) {
  bool v = (S.rows <= 1 || S.ld % 4 == 0) && (!with_out || aligned16(S.out));
#pragma unroll
  for (int k = 0; k < T; ++k) v = v && aligned16(S.bank[k]);  // (a NULL bank is aligned)
  return v;
}

// One segment's walk: every stored element of a marked (or every) row is seen exactly once.  f4(r, c): the 16-byte
// piece at columns c .. c + 3 of row r; f1(r, c): one element.
template <class F4, class F1>
__device__ __forceinline__ void pcg_walk(const mml_pcgrad_seg& S, bool vec, F4 f4, F1 f1) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint8_t* marks = S.row_marks;
  const int cols = S.cols;
  if (vec) {
    const int c4 = cols >> 2, tail = cols & 3;
    const int upr = c4 + (tail ? 1 : 0);  // pieces per row
    const int64_t total = S.rows * upr;
    const bool small = total < 0x7fffffff;
    for (int64_t i = tid; i < total; i += stride) {
      const int64_t r = small ? (int64_t)((uint32_t)i / (uint32_t)upr) : i / upr;
      const int u = (int)(i - r * upr);
      if (marks && !marks[r]) continue;
      if (u < c4) {
        f4(r, u << 2);
      } else {
        for (int c = c4 << 2; c < cols; ++c) f1(r, c);
      }
    }
  } else {
    const int64_t total = S.rows * cols;
    const bool small = total < 0x7fffffff;
    for (int64_t i = tid; i < total; i += stride) {
      const int64_t r = small ? (int64_t)((uint32_t)i / (uint32_t)cols) : i / cols;
      if (marks && !marks[r]) continue;
      f1(r, (int)(i - r * cols));
    }
  }
}

template <int T>
__device__ __forceinline__ void pcg_acc(double (&acc)[pcg_pairs(T)], const float (&v)[T]) {
  int p = 0;
#pragma unroll
  for (int a = 0; a < T; ++a)
#pragma unroll
    for (int b = a; b < T; ++b, ++p) acc[p] = fma((double)v[a], (double)v[b], acc[p]);
}

// part[((seg0 + blockIdx.y) * gridDim.x + blockIdx.x) * P + p], pairs p in the order (0,0), (0,1), .., (1,1), ..
template <int T>
__global__ __launch_bounds__(256) void pcgrad_gram_kernel(const PcgBatch Bt, double* part, int seg0) {
  constexpr int P = pcg_pairs(T);
  const mml_pcgrad_seg& S = Bt.s[blockIdx.y];
  double acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.0;
  const bool vec = pcg_vec<T>(S, false);
  pcg_walk(
      S, vec,
      [&](int64_t r, int c) __attribute__((always_inline)) {
        float4 q[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
          q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (S.bank[k]) q[k] = *reinterpret_cast<const float4*>(S.bank[k] + r * S.ld + c);  // (uniform)
        }
        float v[T];
#pragma unroll
        for (int k = 0; k < T; ++k) v[k] = q[k].x;
        pcg_acc<T>(acc, v);
#pragma unroll
        for (int k = 0; k < T; ++k) v[k] = q[k].y;
        pcg_acc<T>(acc, v);
#pragma unroll
        for (int k = 0; k < T; ++k) v[k] = q[k].z;
        pcg_acc<T>(acc, v);
#pragma unroll
        for (int k = 0; k < T; ++k) v[k] = q[k].w;
        pcg_acc<T>(acc, v);
      },
      [&](int64_t r, int c) __attribute__((always_inline)) {
        float v[T];
#pragma unroll
        for (int k = 0; k < T; ++k) v[k] = S.bank[k] ? S.bank[k][r * S.ld + c] : 0.f;
        pcg_acc<T>(acc, v);
      });
  // lane sums -> wave -> workgroup, always in the same order
  __shared__ double wsum[4][P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double s = acc[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][p] = s;
  }
  __syncthreads();
  if (threadIdx.x < P) {
    const int p = threadIdx.x;
    part[((int64_t)(seg0 + blockIdx.y) * gridDim.x + blockIdx.x) * P + p] =
        (wsum[0][p] + wsum[1][p]) + (wsum[2][p] + wsum[3][p]);
  }
}

// blockIdx.x = pair: thread t owns the partials t, t + 256, ... of its pair, then the same wave / workgroup order
__global__ __launch_bounds__(256) void pcgrad_gram_final_kernel(const double* part, int64_t count, int T, double* gram) {
  const int P = pcg_pairs(T), p = blockIdx.x;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < count; k += 256) s += part[k * P + p];
  __shared__ double wsum[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, left = p;
    while (left >= T - a) {
      left -= T - a;
      ++a;
    }
    const int b = a + left;
    const double g = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    gram[a * T + b] = g;
    gram[b * T + a] = g;
  }
}

// The projection loop on coefficients: thread 0 of one small workgroup (T <= 8: at most 64 x 8 multiply-adds).  Products
// and sums are rounded one by one (__dmul_rn / __dadd_rn: never contracted), k ascending.
__global__ __launch_bounds__(64) void pcgrad_weights_kernel(const double* gram, const int32_t* order, int T, float* w,
                                                             int32_t* fired) {
  __shared__ double G[PCG_MAXT * PCG_MAXT], c[PCG_MAXT], tot[PCG_MAXT];
  __shared__ int32_t ord[PCG_MAXT * PCG_MAXT];
  const int t = threadIdx.x;
  if (t < T * T) {
    G[t] = gram[t];
    ord[t] = order[t];
    if (fired) fired[t] = 0;
  }
  if (t < T) tot[t] = 0.0;
  __syncthreads();
  if (t != 0) return;
  for (int i = 0; i < T; ++i) {
    for (int k = 0; k < T; ++k) c[k] = k == i ? 1.0 : 0.0;
    for (int q = 0; q < T; ++q) {
      const int j = ord[i * T + q];
      if (j < 0 || j >= T) continue;
      double d = 0.0;
      for (int k = 0; k < T; ++k) d = __dadd_rn(d, __dmul_rn(c[k], G[k * T + j]));
      if (d < 0.0 && G[j * T + j] > 0.0) {
        c[j] -= d / G[j * T + j];
        if (fired) fired[i * T + j] = 1;
      }
    }
    for (int k = 0; k < T; ++k) tot[k] = __dadd_rn(tot[k], c[k]);
  }
  for (int k = 0; k < T; ++k) {
    w[k] = (float)(tot[k] / (double)T);
    w[T + k] = (float)tot[k];
  }
}

template <int T>
__global__ __launch_bounds__(256) void pcgrad_combine_kernel(const PcgBatch Bt, const float* w) {
  const mml_pcgrad_seg& S = Bt.s[blockIdx.y];
  float wk[T];
  const float* ws = w + (Bt.mean[blockIdx.y] ? 0 : T);
#pragma unroll
  for (int k = 0; k < T; ++k) wk[k] = ws[k];
  const bool vec = pcg_vec<T>(S, true);
  pcg_walk(
      S, vec,
      [&](int64_t r, int c) __attribute__((always_inline)) {
        float4 q[T];
#pragma unroll
        for (int k = 0; k < T; ++k)
          if (S.bank[k]) q[k] = *reinterpret_cast<const float4*>(S.bank[k] + r * S.ld + c);  // (uniform)
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < T; ++k)
          if (S.bank[k]) {
            o.x = __fmaf_rn(wk[k], q[k].x, o.x); o.y = __fmaf_rn(wk[k], q[k].y, o.y);
            o.z = __fmaf_rn(wk[k], q[k].z, o.z); o.w = __fmaf_rn(wk[k], q[k].w, o.w);
          }
        *reinterpret_cast<float4*>(S.out + r * S.ld + c) = o;  // (out may be a bank: every bank's piece is read above)
      },
      [&](int64_t r, int c) __attribute__((always_inline)) {
        float o = 0.f;
#pragma unroll
        for (int k = 0; k < T; ++k)
          if (S.bank[k]) o = __fmaf_rn(wk[k], S.bank[k][r * S.ld + c], o);
        S.out[r * S.ld + c] = o;
      });
}

// One objective's gradient leaves the accumulating buffers: out = bank[0] over the (marked) rows, and with clear != 0 the
// rows of bank[0] are zeroed behind the copy (the table accumulators the scatter adds into).
__global__ __launch_bounds__(256) void pcgrad_stash_kernel(const PcgBatch Bt, int clear) {
  const mml_pcgrad_seg& S = Bt.s[blockIdx.y];
  float* src = const_cast<float*>(S.bank[0]);
  const bool vec = pcg_vec<1>(S, true);
  pcg_walk(
      S, vec,
      [&](int64_t r, int c) __attribute__((always_inline)) {
        float4* q = reinterpret_cast<float4*>(src + r * S.ld + c);
        *reinterpret_cast<float4*>(S.out + r * S.ld + c) = *q;
        if (clear) *q = make_float4(0.f, 0.f, 0.f, 0.f);
      },
      [&](int64_t r, int c) __attribute__((always_inline)) {
        S.out[r * S.ld + c] = src[r * S.ld + c];
        if (clear) src[r * S.ld + c] = 0.f;
      });
}

// workgroups per segment: enough 256-thread workgroups to fill every CU (8 each: 32 waves) over the m segments of a
// launch, no more than the largest segment has 16-byte pieces for
static unsigned pcg_grid(int64_t most, int m) {
  int64_t want = cdiv(most, (int64_t)256 * 4);
  int64_t fill = cdiv((int64_t)device_cus() * 8, (int64_t)m);
  if (fill < 16) fill = 16;
  if (want > fill) want = fill;
  if (want > PCG_MAX_GX) want = PCG_MAX_GX;
  return (unsigned)(want < 1 ? 1 : want);
}

static int pcg_check(const mml_pcgrad_seg* s, int32_t n, int32_t T, bool need_out, const char* who, int64_t* most) {
  MML_REQUIRE(T >= 1 && T <= PCG_MAXT, "%s: T = %d (1 .. %d)", who, T, PCG_MAXT);
  MML_REQUIRE(s != nullptr && n >= 1, "%s: null segment array or n < 1", who);
  *most = 0;
  for (int i = 0; i < n; ++i) {
    const mml_pcgrad_seg& S = s[i];
    MML_REQUIRE(S.rows >= 0 && S.cols >= 1 && S.ld >= S.cols, "%s: segment %d: rows < 0, cols < 1 or ld < cols", who, i);
    bool any = false;
    for (int k = 0; k < T; ++k) any = any || S.bank[k] != nullptr;
    MML_REQUIRE(any, "%s: segment %d: every bank is NULL", who, i);
    MML_REQUIRE(!need_out || S.out != nullptr, "%s: segment %d: null out", who, i);
    const int64_t e = S.rows * S.cols;
    *most = e > *most ? e : *most;
  }
  return MML_OK;
}

template <class F>
static void pcg_batches(const mml_pcgrad_seg* s, int32_t n, int32_t T, F launch) {
  for (int i0 = 0; i0 < n; i0 += PCG_BATCH) {
    const int m = n - i0 < PCG_BATCH ? n - i0 : PCG_BATCH;
    PcgBatch Bt{};
    for (int i = 0; i < m; ++i) {
      Bt.s[i] = s[i0 + i];
      bool all = true;
      for (int k = 0; k < PCG_MAXT; ++k) {
        if (k >= T) Bt.s[i].bank[k] = nullptr;
        else all = all && Bt.s[i].bank[k] != nullptr;
      }
      Bt.mean[i] = all ? 1 : 0;
    }
    launch(Bt, i0, m);
  }
}

#define PCG_DISPATCH(T, CALL) \
  switch (T) {                \
    case 1: { CALL(1); } break; \
    case 2: { CALL(2); } break; \
    case 3: { CALL(3); } break; \
    case 4: { CALL(4); } break; \
    case 5: { CALL(5); } break; \
    case 6: { CALL(6); } break; \
    case 7: { CALL(7); } break; \
    default: { CALL(8); } break; \
  }

}  // namespace mml

using namespace mml;

extern "C" int64_t mml_pcgrad_workspace_bytes(const mml_pcgrad_seg* s, int32_t n, int32_t T) {
  (void)s;
  if (n < 1 || T < 1 || T > PCG_MAXT) return 0;
  return (int64_t)n * PCG_MAX_GX * pcg_pairs(T) * (int64_t)sizeof(double);
}

extern "C" int mml_pcgrad_gram(const mml_pcgrad_seg* s, int32_t n, int32_t T, double* gram, void* workspace,
                               int64_t workspace_bytes, mml_stream_t stream) {
  int64_t most = 0;
  if (int rc = pcg_check(s, n, T, false, "mml_pcgrad_gram", &most)) return rc;
  MML_REQUIRE(gram != nullptr, "mml_pcgrad_gram: null gram");
  MML_REQUIRE(workspace && workspace_bytes >= mml_pcgrad_workspace_bytes(s, n, T), "mml_pcgrad_gram: workspace too small");
  double* part = static_cast<double*>(workspace);
  const unsigned gx = pcg_grid(most, n < PCG_BATCH ? n : PCG_BATCH);  // (one geometry for every launch: one partial layout)
  hipStream_t st = to_stream(stream);
  pcg_batches(s, n, T, [&](const PcgBatch& Bt, int i0, int m) {
#define PCG_GRAM(TT) MML_LAUNCH(pcgrad_gram_kernel<TT>, dim3(gx, (unsigned)m), dim3(256), 0, st, Bt, part, i0)
    PCG_DISPATCH(T, PCG_GRAM)
#undef PCG_GRAM
  });
  MML_LAUNCH(pcgrad_gram_final_kernel, dim3((unsigned)pcg_pairs(T)), dim3(256), 0, st, (const double*)part,
             (int64_t)n * gx, (int)T, gram);
  return check_launch("mml_pcgrad_gram");
}

extern "C" int mml_pcgrad_weights(const double* gram, const int32_t* order, int32_t T, float* w, int32_t* fired,
                                  mml_stream_t stream) {
  MML_REQUIRE(T >= 1 && T <= PCG_MAXT, "mml_pcgrad_weights: T = %d (1 .. %d)", T, PCG_MAXT);
  MML_REQUIRE(gram && order && w, "mml_pcgrad_weights: null gram, order or w");
  MML_LAUNCH(pcgrad_weights_kernel, dim3(1), dim3(64), 0, to_stream(stream), gram, order, (int)T, w, fired);
  return check_launch("mml_pcgrad_weights");
}

extern "C" int mml_pcgrad_combine(const mml_pcgrad_seg* s, int32_t n, int32_t T, const float* w, mml_stream_t stream) {
  int64_t most = 0;
  if (int rc = pcg_check(s, n, T, true, "mml_pcgrad_combine", &most)) return rc;
  MML_REQUIRE(w != nullptr, "mml_pcgrad_combine: null w");
  if (most == 0) return MML_OK;
  hipStream_t st = to_stream(stream);
  pcg_batches(s, n, T, [&](const PcgBatch& Bt, int i0, int m) {
    (void)i0;
    const unsigned gx = pcg_grid(most, m);
#define PCG_COMBINE(TT) MML_LAUNCH(pcgrad_combine_kernel<TT>, dim3(gx, (unsigned)m), dim3(256), 0, st, Bt, w)
    PCG_DISPATCH(T, PCG_COMBINE)
#undef PCG_COMBINE
  });
  return check_launch("mml_pcgrad_combine");
}

extern "C" int mml_pcgrad_stash(const mml_pcgrad_seg* s, int32_t n, int32_t clear, mml_stream_t stream) {
  int64_t most = 0;
  if (int rc = pcg_check(s, n, 1, true, "mml_pcgrad_stash", &most)) return rc;
  for (int i = 0; i < n; ++i)
    MML_REQUIRE(s[i].out != s[i].bank[0], "mml_pcgrad_stash: segment %d: out is bank[0]", i);
  if (most == 0) return MML_OK;
  hipStream_t st = to_stream(stream);
  pcg_batches(s, n, 1, [&](const PcgBatch& Bt, int i0, int m) {
    (void)i0;
    MML_LAUNCH(pcgrad_stash_kernel, dim3(pcg_grid(most, m), (unsigned)m), dim3(256), 0, st, Bt, (int)clear);
  });
  return check_launch("mml_pcgrad_stash");
}
