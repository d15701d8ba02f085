// The LDS row fold shared by scatter_fold_kernel (gather_scatter.hip) and scatter_pool_fold_kernel (pooled_rows.hip):
// a workgroup folds the duplicate rows of ONE field's chunk of lookups in LDS in 64-bit fixed point (fold_fixed.hpp),
// then issues E contiguous atomics per distinct row.  Each kernel keeps its own load phase, its emax / shift and its
// `nonfinite` predicate; the insert and the flush are the two functions below.
//
// LDS layout (SLOTS slots, CHUNK = SLOTS / 2 lookups per chunk: hash load factor <= 0.5):
//   long long acc[E][PITCH]   fixed-point sums, plane-major with PITCH = SLOTS + 1: the lanes of an insert differ in
//                             slot (random banks) and the lanes of a flush in e (consecutive banks)
//   int keys[SLOTS]           row of the slot, or -1
//   unsigned short occ[SLOTS] occupied slots in first-claim order (a kernel may put arrays of its own in front of it)
// Tables with V <= SLOTS rows are direct-mapped (slot = row: no compare-and-swap, no probing, the flush walks V rows).
// Why it looks like this (tools/lab/micro/lds_atomic.hip, per wave-instruction and CU): ds_add_f32 = 195 cycles
// whatever the address pattern, ds_add_u64 = 15, ds_add_u32 = 9, ds_cmpst_rtn_b32 = 15; a same-address integer atomic
// costs ~4 cycles per lane.  So the sums are integer, the occupied slots are listed with ONE counter atomic per wave
// (ballot), and the flush walks that list instead of all SLOTS x E cells.
#pragma once
#include "fold_fixed.hpp"

#include <atomic>

namespace mml {
#ifdef __HIPCC__
// One lookup's insert.  A lane owns one 16-byte piece (`part`) of a gradient row, E / 4 lanes per lookup; key < 0: no
// lookup (the lane still takes part in the ballot and the shuffle).  add: gradients are folded (false: index-only pass).
template <int SLOTS, int E>
__device__ __forceinline__ void fold_insert(long long* acc, int* keys, unsigned short* occ, int* n_occ, bool direct,
                                            int key, int part, int lane, bool add, const float4& g, int emax, int shift,
                                            bool nonfinite, float* table_rows) {
  constexpr int LPS = E / 4;
  constexpr int PITCH = SLOTS + 1;
  unsigned slot = 0;
  bool is_new = false;
  if (direct) {
    if (key >= 0) {
      slot = (unsigned)key;
      if (part == 0 && keys[slot] != key) keys[slot] = key;  // racing writers store the same value
    }
  } else {
    if (key >= 0 && part == 0) {  // one lane per lookup claims the slot ...
      slot = (((unsigned)key * 2654435761u) >> 16) & (SLOTS - 1);
      while (true) {
        const int old = atomicCAS(&keys[slot], -1, key);
        if (old == -1) { is_new = true; break; }
        if (old == key) break;
        slot = (slot + 1) & (SLOTS - 1);
      }
    }
    // new slots of this wave join the occupied list with ONE counter atomic
    const unsigned long long nm = __ballot(is_new);
    if (nm) {
      const int leader = __ffsll((long long)nm) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(n_occ, __popcll(nm));
      base = __shfl(base, leader);
      if (is_new) occ[base + __popcll(nm & ((1ull << lane) - 1ull))] = (unsigned short)slot;
    }
    if (LPS > 1) slot = (unsigned)__shfl((int)slot, lane & ~(LPS - 1));  // ... its lanes follow
  }
  if (add && key >= 0) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(acc) + (part * 4) * PITCH + slot;
    atomicAdd(p, (unsigned long long)to_fixed(g.x, emax, shift));
    atomicAdd(p + PITCH, (unsigned long long)to_fixed(g.y, emax, shift));
    atomicAdd(p + 2 * PITCH, (unsigned long long)to_fixed(g.z, emax, shift));
    atomicAdd(p + 3 * PITCH, (unsigned long long)to_fixed(g.w, emax, shift));
    // A diverged backward (Inf / NaN in dOut) must reach the table like it does in the reference (index_add of a NaN is
    // NaN), not be turned into a finite fixed-point value: such elements skip the fold (to_fixed gives 0) and go to
    // HBM as float atomics.
    if (nonfinite) {
      float* dst = table_rows + (int64_t)key * E + part * 4;
      const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((__float_as_uint(gv[i]) & 0x7f800000u) == 0x7f800000u) atomicAdd(dst + i, gv[i]);
    }
  }
}

// The flush, after a barrier behind the last insert: E contiguous atomics per distinct row -- float atomics on the
// table's gradient rows, or (DET) 64-bit integer atomics on its row totals -- and the row is marked: a byte of
// marks_of_table (the table's own range of the mark map) or, without one, a bit of seen_of_table; both may be null.
template <int SLOTS, int E, bool DET>
__device__ __forceinline__ void fold_flush(const long long* acc, const int* keys, const unsigned short* occ, int n_occ,
                                           bool direct, int V, int nthreads, bool add, float* table_rows,
                                           long long* acc64_rows, int emax, uint8_t* marks_of_table,
                                           uint32_t* seen_of_table) {
  constexpr int PITCH = SLOTS + 1;
  const int n_items = (direct ? V : n_occ) * E;
  for (int item = threadIdx.x; item < n_items; item += nthreads) {
    const int i = item / E, e = item - i * E;
    const int slot = direct ? i : (int)occ[i];
    const int key = keys[slot];
    if (key < 0) continue;  // (direct-mapped: a row no lookup of this workgroup touched)
    if (DET) {
      const long long v = acc[e * PITCH + slot];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(acc64_rows) + (int64_t)key * E + e, (unsigned long long)v);
    } else if (add) {
      atomicAdd(table_rows + (int64_t)key * E + e, from_fixed(acc[e * PITCH + slot], emax));
    }
    // touched-row bookkeeping: only MARK the row here (a non-returning atomic: they run at the float-atomic request
    // rate, while the returning form that told "first time seen" cost the index-only pass 0.5 ms); the list is built
    // from the bitmaps by rows_compact_kernel
    if (e == 0) {
      if (marks_of_table) marks_of_table[key] = 1;  // plain store: hot rows cost nothing (see mark_rows_kernel)
      else if (seen_of_table) atomicOr(seen_of_table + (key >> 5), 1u << (key & 31));
    }
  }
}
#endif

// ---- host side ----

// Mark map layout (row_marks of mml_scatter_bwd; ops.marks_bytes states the size): entry f of n owns the bytes
// [out[f], out[f] + vocab[f]), out[f] = 32 * (prefix sum of ceil(vocab / 32)) -- every range starts 32-byte aligned,
// one bitmap word per 32 bytes.  Returns the size of the map in 32-byte words.
inline int64_t mark_bases(const int64_t* vocab, int n, int64_t* out) {
  int64_t words = 0;
  for (int f = 0; f < n; ++f) {
    out[f] = words * 32;
    words += (vocab[f] + 31) / 32;
  }
  return words;
}

// The fold kernels use more dynamic LDS than the 64 KiB a kernel may use by default.  The attribute is per kernel and
// per DEVICE (a process may drive several): set once for each, not per launch.
template <auto Kernel>
inline int allow_big_lds(const char* who) {
  static std::atomic<uint64_t> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !((attr_set.load(std::memory_order_relaxed) >> dev) & 1ull)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
    if (e != hipSuccess) {
      set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
      return MML_ERR_HIP;
    }
    if (dev >= 0 && dev < 64) attr_set.fetch_or(1ull << dev, std::memory_order_relaxed);
  }
  return MML_OK;
}

// *count = 0 on the stream: a call that touches no row (or whose kernels only append) must not keep the previous list
inline int clear_touched(int32_t* count, hipStream_t stream, const char* who) {
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) {
    set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return MML_ERR_HIP;
  }
  return MML_OK;
}

}  // namespace mml
