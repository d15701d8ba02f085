// PReLU with ONE learnable slope per layer (reference model/utils.py:25-26 `nn.PReLU()` inside DNN, :153-159
// fc -> bn -> activation -> dropout), torch's semantics:
//   forward : y  = z > 0 ? z  : a * z          (one fp32 multiply; z = +-0 takes the a * z branch)
//   backward: dz = z > 0 ? dy : a * dy,   da = sum over the elements with z <= 0 of dy * z
// The backward reads z, not y: for a <= 0 the sign of y no longer tells the sign of z, and a trained slope may get there.
// The slope is read from DEVICE memory by the kernels, so a replayed HIP graph sees what the optimizer left.
//
// Both kernels are streaming and HBM-bound (8 B / element forward, 12 B / element backward): blockIdx.y = item,
// blockIdx.x strides over the item's rows in 16-byte pieces (plus a scalar piece for the cols % 4 tail of a row), or over
// single elements where the pitch or a pointer is not 16-byte aligned.  Padding columns [cols, ld) are never touched.
// da: lane sums -> wave (xor butterfly) -> workgroup (wave order) -> one partial per workgroup in the workspace -> a
// second kernel adds the partials of every item that names one dalpha in item order, in double.  No float atomics: the
// bits depend on the launch geometry (the device's CU count and the shapes) only.
#include "common.hpp"

namespace mml {

constexpr int PRELU_BATCH = 32;    // items per launch (the descriptors travel as kernel arguments: 32 x 96 B backward)
constexpr int PRELU_MAX_GX = 2048; // most workgroups per item: the partials of one item in the workspace
constexpr int PRELU_AMAX_GX = 256; // an item that raises a magnitude slot: see copy2d_batch_kernel (csrc/ew.hip)

struct PreluFwdBatch {
  mml_prelu_desc d[PRELU_BATCH];
};
struct PreluBwdBatch {
  mml_prelu_bwd_desc d[PRELU_BATCH];
  int8_t first[PRELU_BATCH];  // 1: no earlier item names this dalpha
  int8_t next[PRELU_BATCH];   // the next item that names the same dalpha, or -1
};

// One item's walk: every stored element is seen exactly once.  16-byte pieces go through ld4 (the loads of a piece) and
// st4 (arithmetic + store), four pieces in flight per thread: loads first, stores after -- the compiler cannot move a load
// above a store through pointers it must assume to alias, and one 16-byte load per thread at a time leaves HBM idle.
template <class LD4, class ST4, class F1>
__device__ __forceinline__ void prelu_walk(int64_t rows, int cols, bool vec, int nb, LD4 ld4, ST4 st4, F1 f1) {
  const int64_t stride = (int64_t)nb * 256;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    const int c4 = cols >> 2, tail = cols & 3;
    const int upr = c4 + (tail ? 1 : 0);  // pieces per row
    const int64_t total = rows * upr;
    const bool small = total < 0x7fffffff;
    auto where = [&](int64_t i, int64_t& r, int& u) __attribute__((always_inline)) {
      r = small ? (int64_t)((uint32_t)i / (uint32_t)upr) : i / upr;
      u = (int)(i - r * upr);
    };
    auto piece = [&](int64_t r, int u) __attribute__((always_inline)) {
      if (u < c4) {
        st4(r, u << 2, ld4(r, u << 2));
      } else {
        for (int c = c4 << 2; c < cols; ++c) f1(r, c);
      }
    };
    int64_t i = tid;
    for (; i + 3 * stride < total; i += 4 * stride) {
      int64_t r0, r1, r2, r3;
      int u0, u1, u2, u3;
      where(i, r0, u0); where(i + stride, r1, u1); where(i + 2 * stride, r2, u2); where(i + 3 * stride, r3, u3);
      if (u0 < c4 && u1 < c4 && u2 < c4 && u3 < c4) {
        const auto v0 = ld4(r0, u0 << 2), v1 = ld4(r1, u1 << 2), v2 = ld4(r2, u2 << 2), v3 = ld4(r3, u3 << 2);
        st4(r0, u0 << 2, v0); st4(r1, u1 << 2, v1); st4(r2, u2 << 2, v2); st4(r3, u3 << 2, v3);
      } else {
        piece(r0, u0); piece(r1, u1); piece(r2, u2); piece(r3, u3);
      }
    }
    for (; i < total; i += stride) {
      int64_t r;
      int u;
      where(i, r, u);
      piece(r, u);
    }
  } else {
    const int64_t total = rows * cols;
    const bool small = total < 0x7fffffff;
    for (int64_t i = tid; i < total; i += stride) {
      const int64_t r = small ? (int64_t)((uint32_t)i / (uint32_t)cols) : i / cols;
      f1(r, (int)(i - r * cols));
    }
  }
}

// (__fmul_rn: the product is rounded on its own -- never contracted into the accumulate_dz add)
__device__ __forceinline__ float prelu_pick(float z, float v, float a) { return z > 0.f ? v : __fmul_rn(a, v); }

__global__ __launch_bounds__(256) void prelu_fwd_kernel(const PreluFwdBatch Bt) {
  const mml_prelu_desc& D = Bt.d[blockIdx.y];
  const int nb = D.amax_out ? ((int)gridDim.x < PRELU_AMAX_GX ? (int)gridDim.x : PRELU_AMAX_GX) : (int)gridDim.x;
  const bool mine = (int)blockIdx.x < nb;  // (uniform)
  float amf = 0.f;
  if (mine) {
    const float a = *D.alpha;
    const bool vec = D.ldz % 4 == 0 && D.ldy % 4 == 0 && aligned16(D.z) && aligned16(D.y);
    prelu_walk(
        D.rows, D.cols, vec, nb,
        [&](int64_t r, int c) __attribute__((always_inline)) {
          return *reinterpret_cast<const float4*>(D.z + r * D.ldz + c);
        },
        [&](int64_t r, int c, const float4 z) __attribute__((always_inline)) {
          float4 y;
          y.x = prelu_pick(z.x, z.x, a); y.y = prelu_pick(z.y, z.y, a);
          y.z = prelu_pick(z.z, z.z, a); y.w = prelu_pick(z.w, z.w, a);
          *reinterpret_cast<float4*>(D.y + r * D.ldy + c) = y;
          amax_acc(amf, y);
        },
        [&](int64_t r, int c) __attribute__((always_inline)) {
          const float z = D.z[r * D.ldz + c];
          const float y = prelu_pick(z, z, a);
          D.y[r * D.ldy + c] = y;
          amax_acc(amf, y);
        });
  }
  amax_flush<true>(amf, mine ? D.amax_out : nullptr);  // (uniform per workgroup; a null slot returns at once)
}

struct Bwd4 {
  float4 z, dy, o;
};

__global__ __launch_bounds__(256) void prelu_bwd_kernel(const PreluBwdBatch Bt, float* part) {
  const mml_prelu_bwd_desc& D = Bt.d[blockIdx.y];
  const int nb = D.amax_out ? ((int)gridDim.x < PRELU_AMAX_GX ? (int)gridDim.x : PRELU_AMAX_GX) : (int)gridDim.x;
  const bool mine = (int)blockIdx.x < nb;  // (uniform)
  float amf = 0.f, s = 0.f;
  if (mine) {
    const float a = *D.alpha;
    const bool acc = D.accumulate_dz != 0;
    const bool vec = D.lddy % 4 == 0 && D.ldz % 4 == 0 && D.lddz % 4 == 0 && aligned16(D.dy) && aligned16(D.z) &&
                     aligned16(D.dz);
    auto one = [&](float z, float dy, float old) __attribute__((always_inline)) {
      s += z > 0.f ? 0.f : dy * z;
      const float g = prelu_pick(z, dy, a);
      return acc ? old + g : g;
    };
    prelu_walk(
        D.rows, D.cols, vec, nb,
        [&](int64_t r, int c) __attribute__((always_inline)) {
          Bwd4 v;
          v.z = *reinterpret_cast<const float4*>(D.z + r * D.ldz + c);
          v.dy = *reinterpret_cast<const float4*>(D.dy + r * D.lddy + c);  // (read before dz, which may be dy)
          v.o = make_float4(0.f, 0.f, 0.f, 0.f);
          if (acc) v.o = *reinterpret_cast<const float4*>(D.dz + r * D.lddz + c);
          return v;
        },
        [&](int64_t r, int c, const Bwd4 v) __attribute__((always_inline)) {
          const float4 z = v.z, dy = v.dy, o = v.o;
          float4* q = reinterpret_cast<float4*>(D.dz + r * D.lddz + c);
          float4 g;
          g.x = one(z.x, dy.x, o.x); g.y = one(z.y, dy.y, o.y); g.z = one(z.z, dy.z, o.z); g.w = one(z.w, dy.w, o.w);
          *q = g;
          amax_acc(amf, g);
        },
        [&](int64_t r, int c) __attribute__((always_inline)) {
          float* q = D.dz + r * D.lddz + c;
          const float dy = D.dy[r * D.lddy + c];
          const float g = one(D.z[r * D.ldz + c], dy, acc ? *q : 0.f);
          *q = g;
          amax_acc(amf, g);
        });
  }
  // lane sums -> wave -> workgroup, always in the same order
  __shared__ float wsum[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  amax_flush<true>(amf, mine ? D.amax_out : nullptr);
}

// blockIdx.x = item; only the FIRST item that names a dalpha works: it adds the partials of every item of its chain, item
// after item.  Thread t owns the partials t, t + 256, ... (double), then the same wave / workgroup order as above.
__global__ __launch_bounds__(256) void prelu_final_kernel(const PreluBwdBatch Bt, const float* part, int gx) {
  if (!Bt.first[blockIdx.x]) return;  // (uniform)
  double s = 0.0;
  for (int j = blockIdx.x; j >= 0; j = Bt.next[j])
    for (int k = threadIdx.x; k < gx; k += 256) s += (double)part[(int64_t)j * gx + k];
  __shared__ double wsum[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const mml_prelu_bwd_desc& D = Bt.d[blockIdx.x];
    const float da = (float)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    *D.dalpha = D.accumulate_dalpha ? *D.dalpha + da : da;
  }
}

// workgroups per item: enough 256-thread workgroups to fill every CU (8 each: 32 waves) over the m items of the launch,
// no more than the largest item has 16-byte pieces for
static unsigned prelu_grid(int64_t most, int m) {
  int64_t want = cdiv(most, (int64_t)256 * 4);
  int64_t fill = cdiv((int64_t)device_cus() * 8, (int64_t)m);
  if (fill < 32) fill = 32;
  if (want > fill) want = fill;
  if (want > PRELU_MAX_GX) want = PRELU_MAX_GX;
  return (unsigned)(want < 1 ? 1 : want);
}

}  // namespace mml

using namespace mml;

extern "C" int32_t mml_prelu_max_batch(void) { return PRELU_BATCH; }

extern "C" int mml_prelu_batch_fwd(const mml_prelu_desc* d, int32_t n, mml_stream_t stream) {
  MML_REQUIRE(d != nullptr, "mml_prelu_batch_fwd: null descriptor array");
  MML_REQUIRE(n >= 1 && n <= PRELU_BATCH, "mml_prelu_batch_fwd: %d items (1 .. %d per launch)", n, PRELU_BATCH);
  PreluFwdBatch Bt{};
  int64_t most = 0;
  for (int i = 0; i < n; ++i) {
    const mml_prelu_desc& D = d[i];
    MML_REQUIRE(D.rows >= 0 && D.cols >= 1, "mml_prelu_batch_fwd: item %d: rows < 0 or cols < 1", i);
    MML_REQUIRE(D.z && D.y && D.alpha && D.ldz >= D.cols && D.ldy >= D.cols,
                "mml_prelu_batch_fwd: item %d: null pointer or leading dimension < cols", i);
    Bt.d[i] = D;
    most = D.rows * D.cols > most ? D.rows * D.cols : most;
  }
  if (most == 0) return MML_OK;
  MML_LAUNCH(prelu_fwd_kernel, dim3(prelu_grid(most, n), (unsigned)n), dim3(256), 0, to_stream(stream), Bt);
  return check_launch("mml_prelu_batch_fwd");
}

extern "C" int64_t mml_prelu_workspace_bytes(int32_t n) {
  if (n < 1) return 0;
  return (int64_t)n * PRELU_MAX_GX * 4;
}

extern "C" int mml_prelu_batch_bwd(const mml_prelu_bwd_desc* d, int32_t n, void* workspace, int64_t workspace_bytes,
                                   mml_stream_t stream) {
  MML_REQUIRE(d != nullptr, "mml_prelu_batch_bwd: null descriptor array");
  MML_REQUIRE(n >= 1 && n <= PRELU_BATCH, "mml_prelu_batch_bwd: %d items (1 .. %d per launch)", n, PRELU_BATCH);
  PreluBwdBatch Bt{};
  int64_t most = 0;
  for (int i = 0; i < n; ++i) {
    const mml_prelu_bwd_desc& D = d[i];
    MML_REQUIRE(D.rows >= 0 && D.cols >= 1, "mml_prelu_batch_bwd: item %d: rows < 0 or cols < 1", i);
    MML_REQUIRE(D.dy && D.z && D.dz && D.alpha && D.dalpha && D.lddy >= D.cols && D.ldz >= D.cols && D.lddz >= D.cols,
                "mml_prelu_batch_bwd: item %d: null pointer or leading dimension < cols", i);
    Bt.d[i] = D;
    Bt.first[i] = 1;
    Bt.next[i] = -1;
    for (int j = i - 1; j >= 0; --j)
      if (d[j].dalpha == D.dalpha) {  // the latest earlier item of the chain
        MML_REQUIRE((d[j].accumulate_dalpha != 0) == (D.accumulate_dalpha != 0),
                    "mml_prelu_batch_bwd: items %d and %d share dalpha but not accumulate_dalpha", j, i);
        Bt.first[i] = 0;
        Bt.next[j] = (int8_t)i;
        break;
      }
    most = D.rows * D.cols > most ? D.rows * D.cols : most;
  }
  MML_REQUIRE(workspace && workspace_bytes >= mml_prelu_workspace_bytes(n), "mml_prelu_batch_bwd: workspace too small");
  float* part = static_cast<float*>(workspace);
  const unsigned gx = prelu_grid(most, n);  // (an all-empty launch still writes its zero sums)
  hipStream_t st = to_stream(stream);
  MML_LAUNCH(prelu_bwd_kernel, dim3(gx, (unsigned)n), dim3(256), 0, st, Bt, part);
  MML_LAUNCH(prelu_final_kernel, dim3((unsigned)n), dim3(256), 0, st, Bt, (const float*)part, (int)gx);
  return check_launch("mml_prelu_batch_bwd");
}
