// The K6/K7 elementwise and copy helpers for STAR (model/utils.py:214-218) and PepNet (model/pepnet.py:31-32, :72-78,
// :139-140), and the device counter.  Pure streaming kernels: 16-byte accesses per lane where the operands allow it,
// grid-stride, HBM-bound.
#include "common.hpp"

namespace mml {

__global__ void counter_kernel(int32_t* c, int32_t delta, int32_t reset) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *c = reset ? 0 : (*c + delta);
}

// ---- elementwise -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ew_mul_kernel(const float* a, const float* b, float* out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = a[i] * b[i];
}

// act_a / act_b: the operand is the OUTPUT of that activation and this product is its only consumer, so the
// activation's derivative (from the output value, like mml_act_bwd) is folded into the gradient written here.
// (The same function as common.hpp's act_bwd in another spelling: SIGMOID2 as y (1 - y / 2) = 2 s (1 - s), s = y / 2.  The
// two round differently, so this one keeps its own text and the kernels here their bits.)
__device__ __forceinline__ float act_deriv_from_output(float y, int act) {
  if (act == MML_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (act == MML_ACT_SIGMOID) return y * (1.f - y);
  if (act == MML_ACT_SIGMOID2) return y * (1.f - 0.5f * y);
  return 1.f;
}
__global__ __launch_bounds__(256) void ew_mul_bwd_kernel(const float* dout, const float* a, const float* b, float* da,
                                                         float* db, int acc_a, int acc_b, int64_t n, int act_a,
                                                         int act_b) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = dout[i];
    const float av = (db || act_a) ? a[i] : 0.f;
    const float bv = (da || act_b) ? b[i] : 0.f;
    if (da) {
      const float v = d * bv * act_deriv_from_output(av, act_a);
      da[i] = acc_a ? da[i] + v : v;
    }
    if (db) {
      const float v = d * av * act_deriv_from_output(bv, act_b);
      db[i] = acc_b ? db[i] + v : v;
    }
  }
}

struct AddN {
  const float* in[16];
  int32_t n_in;
};
__global__ __launch_bounds__(256) void ew_add_n_kernel(const AddN A, float* out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int k = 0; k < A.n_in; ++k) s += A.in[k][i];
    out[i] = s;
  }
}

// n independent items in ONE launch: out[i] (+)= sum_k x_k[i] * (y_k ? y_k[i] : 1).  STAR's derived parameters
// (W_spec * W_shared, b_spec + b_shared for every head and layer, model/utils.py:214-216) and their gradients were
// ~60 launches of a few KB each per step; they are two launches each way now.
struct SumProdBatch {
  mml_sumprod_desc d[MML_SUMPROD_BATCH];
};
// (act_deriv_from_output is defined further up with the mul_bwd kernel; deriv_of = the OUTPUT of the activation whose
// derivative multiplies the sum -- PepNet's gate products, where the factor is 2*sigmoid(.) or relu(.) and this product
// its only consumer)
__global__ __launch_bounds__(256) void sumprod_batch_kernel(const SumProdBatch Bt) {
  const mml_sumprod_desc& D = Bt.d[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool vec = (D.n & 3) == 0 && aligned16(D.out) && (!D.deriv_of || aligned16(D.deriv_of));
  for (int k = 0; k < D.n_terms; ++k) vec = vec && aligned16(D.x[k]) && (!D.y[k] || aligned16(D.y[k]));
  float am = 0.f;  // operand magnitude of what this thread stores (D.amax_out)
  if (vec) {  // 16 bytes per lane and operand
    const int64_t n4 = D.n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      float4 s = D.accumulate ? reinterpret_cast<const float4*>(D.out)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < D.n_terms; ++k) {
        const float4 x = reinterpret_cast<const float4*>(D.x[k])[i];
        if (D.y[k]) {
          const float4 y = reinterpret_cast<const float4*>(D.y[k])[i];
          s.x += x.x * y.x; s.y += x.y * y.y; s.z += x.z * y.z; s.w += x.w * y.w;
        } else {
          s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
      }
      if (D.act != MML_ACT_NONE) {
        const float4 o = reinterpret_cast<const float4*>(D.deriv_of)[i];
        s.x *= act_deriv_from_output(o.x, D.act); s.y *= act_deriv_from_output(o.y, D.act);
        s.z *= act_deriv_from_output(o.z, D.act); s.w *= act_deriv_from_output(o.w, D.act);
      }
      reinterpret_cast<float4*>(D.out)[i] = s;
      amax_acc(am, s);
    }
    amax_flush(am, D.amax_out);
    return;
  }
  for (int64_t i = tid; i < D.n; i += stride) {
    float s = D.accumulate ? D.out[i] : 0.f;
    for (int k = 0; k < D.n_terms; ++k) s += D.x[k][i] * (D.y[k] ? D.y[k][i] : 1.f);
    if (D.act != MML_ACT_NONE) s *= act_deriv_from_output(D.deriv_of[i], D.act);
    D.out[i] = s;
    amax_acc(am, s);
  }
  amax_flush(am, D.amax_out);
}

__global__ __launch_bounds__(256) void copy2d_kernel(const float* src, int64_t lds_, float* dst, int64_t ldd, int64_t rows,
                                                     int cols, int accumulate) {
  const int64_t total = rows * cols;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    const float v = src[r * lds_ + c];
    float* d = dst + r * ldd + c;
    *d = accumulate ? *d + v : v;
  }
}

constexpr int COPY2D_BATCH = 32;
struct Copy2dBatch {
  mml_copy2d_desc d[COPY2D_BATCH];
};
// blockIdx.y = item; blockIdx.x strides over that item's elements.  Round 6: 16-byte pieces, four in flight per thread, where
// the item allows it (PepNet's [65 536, 64] concat blocks: one scalar element and a 64-bit division per trip before), and
// an item that raises a magnitude slot is walked by at most 256 workgroups -- every workgroup ends with a look at (and
// possibly an atomic on) the slot's one line, and 2 048 of them finishing together cost more than the magnitude pass the
// slot replaces (measured: +25 us per copy launch).
__global__ __launch_bounds__(256) void copy2d_batch_kernel(const Copy2dBatch Bt) {
  const mml_copy2d_desc& D = Bt.d[blockIdx.y];
  const int nb = D.amax_out ? ((int)gridDim.x < 256 ? (int)gridDim.x : 256) : (int)gridDim.x;
  const bool mine = (int)blockIdx.x < nb;  // (uniform)
  float amf = 0.f;
  if (mine) {
    const int64_t stride = (int64_t)nb * 256;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool vec = D.cols % 4 == 0 && D.lds % 4 == 0 && D.ldd % 4 == 0 && aligned16(D.src) && aligned16(D.dst);
    if (vec) {
      const int c4 = D.cols >> 2;
      const int64_t total = D.rows * c4;
      const bool small = total < 0x7fffffff;
      auto off = [&](int64_t i, int64_t& so, int64_t& dof) __attribute__((always_inline)) {
        const int64_t r = small ? (int64_t)((uint32_t)i / (uint32_t)c4) : i / c4;
        const int64_t c = (i - r * c4) << 2;
        so = r * D.lds + c;
        dof = r * D.ldd + c;
      };
      auto fin = [&](float4 v, int64_t dof) __attribute__((always_inline)) {
        float4* q = reinterpret_cast<float4*>(D.dst + dof);
        if (D.accumulate) {
          const float4 o = *q;
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        *q = v;
        amax_acc(amf, v);
      };
      int64_t i = tid;
      for (; i + 3 * stride < total; i += 4 * stride) {
        int64_t s0, s1, s2, s3, d0, d1, d2, d3;
        off(i, s0, d0); off(i + stride, s1, d1); off(i + 2 * stride, s2, d2); off(i + 3 * stride, s3, d3);
        const float4 v0 = *reinterpret_cast<const float4*>(D.src + s0), v1 = *reinterpret_cast<const float4*>(D.src + s1);
        const float4 v2 = *reinterpret_cast<const float4*>(D.src + s2), v3 = *reinterpret_cast<const float4*>(D.src + s3);
        fin(v0, d0); fin(v1, d1); fin(v2, d2); fin(v3, d3);
      }
      for (; i < total; i += stride) {
        int64_t s0, d0;
        off(i, s0, d0);
        fin(*reinterpret_cast<const float4*>(D.src + s0), d0);
      }
    } else {
      const int64_t total = D.rows * D.cols;
      for (int64_t i = tid; i < total; i += stride) {
        const int64_t r = i / D.cols;
        const int c = (int)(i - r * D.cols);
        float v = D.src[r * D.lds + c];
        float* q = D.dst + r * D.ldd + c;
        if (D.accumulate) v += *q;
        *q = v;
        amax_acc(amf, v);
      }
    }
  }
  amax_flush<true>(amf, mine ? D.amax_out : nullptr);  // (uniform per workgroup; a null slot returns at once)
}

struct ColSegs {
  const float* src[MML_MAX_FIELDS];
  float* dst[MML_MAX_FIELDS];
  int64_t lds_[MML_MAX_FIELDS], ldd[MML_MAX_FIELDS];
  int32_t width[MML_MAX_FIELDS];
  int32_t start[MML_MAX_FIELDS + 1];  // prefix sum of widths
  int32_t n;
};
// One thread per (row, packed column): consecutive lanes walk the packed columns of one row, so each segment is
// read and written in runs of `width` contiguous floats.
__global__ __launch_bounds__(256) void copy_cols_kernel(const ColSegs S, int64_t rows, int accumulate) {
  const int W = S.start[S.n];
  const int64_t total = rows * W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / W;
    const int c = (int)(i - r * W);
    int s = 0;
    while (c >= S.start[s + 1]) ++s;
    const int cc = c - S.start[s];
    const float v = S.src[s][r * S.lds_[s] + cc];
    float* d = S.dst[s] + r * S.ldd[s] + cc;
    *d = accumulate ? *d + v : v;
  }
}

// The same copy in 16-byte pieces (every segment start, width, leading dimension and base pointer a multiple of four
// floats -- the row / row-gradient exchange buffers with E % 4 == 0): segment tables and the column -> segment map are
// staged in LDS once per workgroup, so the inner loop is one LDS lookup + one float4 load + one float4 store.
constexpr int COPY_COLS_MAX_W4 = 1024;
__global__ __launch_bounds__(256) void copy_cols_vec4_kernel(const ColSegs S, int64_t rows, int accumulate) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  __shared__ const float* s_src[MML_MAX_FIELDS];
  __shared__ float* s_dst[MML_MAX_FIELDS];
  __shared__ int64_t s_lds[MML_MAX_FIELDS], s_ldd[MML_MAX_FIELDS];
  __shared__ int32_t s_start[MML_MAX_FIELDS + 1];
  __shared__ uint8_t seg_of[COPY_COLS_MAX_W4];
  const int W4 = S.start[S.n] >> 2;
  for (int k = threadIdx.x; k < S.n; k += 256) {
    s_src[k] = S.src[k]; s_dst[k] = S.dst[k]; s_lds[k] = S.lds_[k]; s_ldd[k] = S.ldd[k];
  }
  for (int k = threadIdx.x; k <= S.n; k += 256) s_start[k] = S.start[k];
  __syncthreads();
  for (int c = threadIdx.x; c < W4; c += 256) {
    int lo = 0, hi = S.n - 1;  // last segment whose start <= 4c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_start[mid] <= 4 * c) lo = mid; else hi = mid - 1;
    }
    seg_of[c] = (uint8_t)lo;
  }
  __syncthreads();
  const int64_t total = rows * W4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r;
    int c;
    if (total < 0x7fffffff) {  // 32-bit division when it fits
      const uint32_t ri = (uint32_t)i / (uint32_t)W4;
      r = ri;
      c = (int)((uint32_t)i - ri * (uint32_t)W4);
    } else {
      r = i / W4;
      c = (int)(i - r * W4);
    }
    const int sg = seg_of[c];
    const int cc = 4 * c - s_start[sg];
    const f4 v = *reinterpret_cast<const f4*>(s_src[sg] + r * s_lds[sg] + cc);
    f4* d = reinterpret_cast<f4*>(s_dst[sg] + r * s_ldd[sg] + cc);
    *d = accumulate ? *d + v : v;
  }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float* y, const float* dy, float* dst, int64_t n, int act) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = y[i];
    float d = 1.f;
    if (act == MML_ACT_RELU) d = v > 0.f ? 1.f : 0.f;
    else if (act == MML_ACT_SIGMOID) d = v * (1.f - v);
    else if (act == MML_ACT_SIGMOID2) d = v * (1.f - 0.5f * v);  // y = 2s: dy/dx = 2 s (1-s) = y (1 - y/2)
    dst[i] = d * dy[i];
  }
}

static unsigned ew_grid(int64_t n) {
  int64_t b = cdiv(n, 256);
  if (b > 256 * 8) b = 256 * 8;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace mml

using namespace mml;

extern "C" int mml_counter_update(int32_t* counter, int32_t delta, int32_t reset, mml_stream_t stream) {
  MML_REQUIRE(counter, "mml_counter_update: null counter");
  mml_opt_step_unbind(counter);  // (constants kept for this counter by mml_opt_step_begin would go stale)
  MML_LAUNCH(counter_kernel, dim3(1), dim3(64), 0, to_stream(stream), counter, delta, reset);
  return check_launch("mml_counter_update");
}

extern "C" int mml_ew_mul(const float* a, const float* b, float* out, int64_t n, mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && (n == 0 || (a && b && out)), "mml_ew_mul: null argument");
  if (n == 0) return MML_OK;
  MML_LAUNCH(ew_mul_kernel, dim3(ew_grid(n)), dim3(256), 0, to_stream(stream), a, b, out, n);
  return check_launch("mml_ew_mul");
}

extern "C" int mml_ew_mul_bwd_act(const float* dout, const float* a, const float* b, float* da, float* db,
                                  int32_t acc_a, int32_t acc_b, int64_t n, int32_t act_a, int32_t act_b,
                                  mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && (n == 0 || dout), "mml_ew_mul_bwd: null dout");
  MML_REQUIRE(!da || b, "mml_ew_mul_bwd: da needs b");
  MML_REQUIRE(!db || a, "mml_ew_mul_bwd: db needs a");
  MML_REQUIRE(act_a >= MML_ACT_NONE && act_a <= MML_ACT_SIGMOID2 && act_b >= MML_ACT_NONE && act_b <= MML_ACT_SIGMOID2,
              "mml_ew_mul_bwd: unknown activation");
  MML_REQUIRE((!act_a || (a && da && !acc_a)) && (!act_b || (b && db && !acc_b)),
              "mml_ew_mul_bwd: a folded activation derivative needs the operand, its gradient, and no accumulation");
  if (n == 0) return MML_OK;
  MML_LAUNCH(ew_mul_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, to_stream(stream), dout, a, b, da, db, acc_a,
                     acc_b, n, act_a, act_b);
  return check_launch("mml_ew_mul_bwd");
}

extern "C" int mml_ew_mul_bwd(const float* dout, const float* a, const float* b, float* da, float* db, int32_t acc_a,
                              int32_t acc_b, int64_t n, mml_stream_t stream) {
  return mml_ew_mul_bwd_act(dout, a, b, da, db, acc_a, acc_b, n, MML_ACT_NONE, MML_ACT_NONE, stream);
}

extern "C" int mml_ew_add_n(const float* const* in, int32_t n_in, float* out, int64_t n, mml_stream_t stream) {
  MML_REQUIRE(in && n_in >= 1 && n_in <= 16 && out && n >= 0, "mml_ew_add_n: bad arguments");
  if (n == 0) return MML_OK;
  AddN A{};
  A.n_in = n_in;
  for (int i = 0; i < n_in; ++i) {
    MML_REQUIRE(in[i], "mml_ew_add_n: input %d null", i);
    A.in[i] = in[i];
  }
  MML_LAUNCH(ew_add_n_kernel, dim3(ew_grid(n)), dim3(256), 0, to_stream(stream), A, out, n);
  return check_launch("mml_ew_add_n");
}

extern "C" int mml_copy2d(const float* src, int64_t lds_, float* dst, int64_t ldd, int64_t rows, int32_t cols,
                          int32_t accumulate, mml_stream_t stream) {
  MML_REQUIRE(rows >= 0 && cols >= 0, "mml_copy2d: negative extent");
  if (rows == 0 || cols == 0) return MML_OK;
  MML_REQUIRE(src && dst && lds_ >= cols && ldd >= cols, "mml_copy2d: null pointer or leading dimension < cols");
  MML_LAUNCH(copy2d_kernel, dim3(ew_grid(rows * cols)), dim3(256), 0, to_stream(stream), src, lds_, dst, ldd,
                     rows, cols, accumulate);
  return check_launch("mml_copy2d");
}

extern "C" int mml_copy2d_batch(const mml_copy2d_desc* d, int32_t n, mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && (n == 0 || d), "mml_copy2d_batch: null descriptor array");
  for (int i0 = 0; i0 < n; i0 += COPY2D_BATCH) {
    Copy2dBatch Bt{};
    int m = 0;
    int64_t most = 0;
    for (int i = i0; i < n && m < COPY2D_BATCH; ++i) {
      const mml_copy2d_desc& D = d[i];
      MML_REQUIRE(D.rows >= 0 && D.cols >= 0, "mml_copy2d_batch: item %d has a negative extent", i);
      if (D.rows == 0 || D.cols == 0) continue;
      MML_REQUIRE(D.src && D.dst && D.lds >= D.cols && D.ldd >= D.cols,
                  "mml_copy2d_batch: item %d: null pointer or leading dimension < cols", i);
      Bt.d[m++] = D;
      most = D.rows * D.cols > most ? D.rows * D.cols : most;
    }
    if (m == 0) continue;
    MML_LAUNCH(copy2d_batch_kernel, dim3(ew_grid(most), (unsigned)m), dim3(256), 0, to_stream(stream), Bt);
    int rc = check_launch("mml_copy2d_batch");
    if (rc) return rc;
  }
  return MML_OK;
}

extern "C" int mml_copy_cols(const float* const* src, const int64_t* lds_, float* const* dst, const int64_t* ldd,
                             const int32_t* width, int32_t n_seg, int64_t rows, int32_t accumulate,
                             mml_stream_t stream) {
  MML_REQUIRE(n_seg >= 0 && rows >= 0, "mml_copy_cols: negative extent");
  if (n_seg == 0 || rows == 0) return MML_OK;
  MML_REQUIRE(src && lds_ && dst && ldd && width, "mml_copy_cols: null array");
  for (int i0 = 0; i0 < n_seg; i0 += MML_MAX_FIELDS) {
    ColSegs S{};
    S.n = (n_seg - i0 < MML_MAX_FIELDS) ? (n_seg - i0) : MML_MAX_FIELDS;
    int acc = 0;
    for (int s = 0; s < S.n; ++s) {
      const int k = i0 + s;
      MML_REQUIRE(src[k] && dst[k] && width[k] > 0 && lds_[k] >= width[k] && ldd[k] >= width[k],
                  "mml_copy_cols: segment %d malformed", k);
      S.src[s] = src[k]; S.dst[s] = dst[k]; S.lds_[s] = lds_[k]; S.ldd[s] = ldd[k]; S.width[s] = width[k];
      S.start[s] = acc;
      acc += width[k];
    }
    S.start[S.n] = acc;
    bool v4 = (acc >> 2) <= COPY_COLS_MAX_W4;
    for (int s = 0; s < S.n && v4; ++s)
      v4 = S.width[s] % 4 == 0 && S.lds_[s] % 4 == 0 && S.ldd[s] % 4 == 0 && aligned16(S.src[s]) && aligned16(S.dst[s]);
    if (v4)
      MML_LAUNCH(copy_cols_vec4_kernel, dim3(ew_grid(rows * (acc >> 2))), dim3(256), 0, to_stream(stream), S, rows,
                 accumulate);
    else
      MML_LAUNCH(copy_cols_kernel, dim3(ew_grid(rows * acc)), dim3(256), 0, to_stream(stream), S, rows, accumulate);
    int rc = check_launch("mml_copy_cols");
    if (rc) return rc;
  }
  return MML_OK;
}

extern "C" int mml_act_bwd(const float* y, const float* dy, float* dst, int64_t n, int32_t act, mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && (n == 0 || (y && dy && dst)), "mml_act_bwd: null argument");
  MML_REQUIRE(act >= MML_ACT_NONE && act <= MML_ACT_SIGMOID2, "mml_act_bwd: unknown activation %d", act);
  if (n == 0) return MML_OK;
  MML_LAUNCH(act_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, to_stream(stream), y, dy, dst, n, act);
  return check_launch("mml_act_bwd");
}

extern "C" int mml_sumprod_batch(const mml_sumprod_desc* d, int32_t n, mml_stream_t stream) {
  MML_REQUIRE(n >= 0 && (n == 0 || d), "mml_sumprod_batch: bad descriptor array");
  // the whole array before the first launch: a malformed item behind the first block of 16 must not be reported after
  // the blocks in front of it have overwritten their outputs
  for (int i = 0; i < n; ++i) {
    const mml_sumprod_desc& D = d[i];
    MML_REQUIRE(D.out && D.n >= 0 && D.n_terms >= 0 && D.n_terms <= MML_SUMPROD_TERMS, "mml_sumprod_batch: item %d malformed", i);
    for (int k = 0; k < D.n_terms; ++k) MML_REQUIRE(D.x[k], "mml_sumprod_batch: item %d term %d is null", i, k);
    MML_REQUIRE(D.act >= MML_ACT_NONE && D.act <= MML_ACT_SIGMOID2 && (D.act == MML_ACT_NONE || (D.deriv_of && !D.accumulate)),
                "mml_sumprod_batch: item %d: a folded activation derivative needs deriv_of and no accumulation", i);
  }
  for (int i0 = 0; i0 < n; i0 += MML_SUMPROD_BATCH) {
    SumProdBatch Bt{};
    const int m = (n - i0 < MML_SUMPROD_BATCH) ? n - i0 : MML_SUMPROD_BATCH;
    int64_t nmax = 0;
    for (int i = 0; i < m; ++i) {
      const mml_sumprod_desc& D = d[i0 + i];
      Bt.d[i] = D;
      nmax = D.n > nmax ? D.n : nmax;
    }
    if (nmax == 0) continue;
    // about 2048 workgroups in all (8 per CU: every wave slot) walking their item grid-stride: items that publish their
    // magnitude end with one atomic per workgroup, and 30 000 of those on eight words cost more than the pass itself
    unsigned gx = ew_grid(nmax);
    const unsigned cap = (unsigned)(2048 / m > 64 ? 2048 / m : 64);
    if (gx > cap) gx = cap;
    MML_LAUNCH(sumprod_batch_kernel, dim3(gx, (unsigned)m), dim3(256), 0, to_stream(stream), Bt);
    int rc = check_launch("mml_sumprod_batch");
    if (rc) return rc;
  }
  return MML_OK;
}
