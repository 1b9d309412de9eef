// Workgroup reductions of the per-clip / per-sample kernels (heads.hip, al.hip, spanprob.h, topk.hip, optim.hip), the level above
// wave.h: a wave reduction, one LDS slot per wave, a barrier, a serial fold over the slots in ascending wave order.  The wave
// primitive, that order and the tie rule below ARE the numbers these kernels promise bit for bit (span indices, top-1 == argmax,
// observe / new_idx): written once, here.  Included by common.h.
//
// Not here, on purpose: cq_wgmax_put / get (cqimg.h) and att_wave_max2_put (attn.hip) are split-phase forms that own no barrier and
// ride on barriers their kernels have anyway; the __shfl_up / __shfl_down scans of heads_kernel are scans; the (k + 2)-column fold of
// spanconf.hip is folded by k + 2 threads over a run-time number of columns, not by every thread over 1 to 3 values.
#pragma once
#include "wave.h"

// ---- what is reduced: the type, the wave primitive the callers are compiled with (wave.h says why each keeps its own), the fold
struct BlockSumF {
  typedef float T;
  static __device__ __forceinline__ float wave(float v) { return wave_sum64(v); }
  static __device__ __forceinline__ float identity() { return 0.f; }
  static __device__ __forceinline__ float fold(float a, float b) { return a + b; }
};
struct BlockMaxF {
  typedef float T;
  static __device__ __forceinline__ float wave(float v) { return wave_max64_bperm(v); }
  static __device__ __forceinline__ float identity() { return -INFINITY; }
  static __device__ __forceinline__ float fold(float a, float b) { return fmaxf(a, b); }
};
// double-precision block sum (the span selection's softmax denominator: the sum of <= 256 floats in double is exact
// to ~2^-53, so its float rounding does not depend on the order of the additions)
struct BlockSumD {
  typedef double T;
  static __device__ __forceinline__ double wave(double v) { return wave_sum64_f64_desc(v); }
  static __device__ __forceinline__ double identity() { return 0.0; }
  static __device__ __forceinline__ double fold(double a, double b) { return a + b; }
};
struct BlockMaxD {
  typedef double T;
  static __device__ __forceinline__ double wave(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
  }
  static __device__ __forceinline__ double identity() { return -INFINITY; }
  static __device__ __forceinline__ double fold(double a, double b) { return fmax(a, b); }
};

// ---- a <- its reduction over the workgroup, in every thread; with b (and c) two (three) reductions share the one pair of barriers.
// Called by all threads of a workgroup of whole waves.  sm: LDS, one slot per wave and value - value i of wave w in [i * nw + w].
// NW: the wave count where the kernel knows it at compile time, 0: blockDim.x / 64 read at run time.
// LEAD: the barrier in front of the stores, which protects `sm` against its previous use; false only for slots nobody has read yet.
// Three plain overloads: the form over an array of N values gave loss_tail_kernel and match_bwd_kernel another register allocation
// (profiles/block_reductions_isa.txt).
template <int NW>
__device__ __forceinline__ int block_waves() { return NW ? NW : (int)(blockDim.x >> 6); }
template <class Op, int NW = 0, bool LEAD = true>
__device__ __forceinline__ typename Op::T block_reduce(typename Op::T a, typename Op::T* sm) {
  a = Op::wave(a);
  const int w = threadIdx.x >> 6;
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = a;
  __syncthreads();
  a = Op::identity();
  for (int q = 0; q < block_waves<NW>(); ++q) a = Op::fold(a, sm[q]);
  return a;
}
template <class Op, int NW = 0, bool LEAD = true>
__device__ __forceinline__ void block_reduce(typename Op::T& a, typename Op::T& b, typename Op::T* sm) {
  a = Op::wave(a); b = Op::wave(b);
  const int w = threadIdx.x >> 6, nw = block_waves<NW>();
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0) { sm[w] = a; sm[nw + w] = b; }
  __syncthreads();
  a = Op::identity(); b = Op::identity();
  for (int q = 0; q < nw; ++q) { a = Op::fold(a, sm[q]); b = Op::fold(b, sm[nw + q]); }
}
template <class Op, int NW = 0, bool LEAD = true>
__device__ __forceinline__ void block_reduce(typename Op::T& a, typename Op::T& b, typename Op::T& c, typename Op::T* sm) {
  a = Op::wave(a); b = Op::wave(b); c = Op::wave(c);
  const int w = threadIdx.x >> 6, nw = block_waves<NW>();
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0) { sm[w] = a; sm[nw + w] = b; sm[2 * nw + w] = c; }
  __syncthreads();
  a = Op::identity(); b = Op::identity(); c = Op::identity();
  for (int q = 0; q < nw; ++q) { a = Op::fold(a, sm[q]); b = Op::fold(b, sm[nw + q]); c = Op::fold(c, sm[2 * nw + q]); }
}

// ---- first-index best-of: the (value, index) pair that `better` prefers, value float or double.  The default order is the argmax
// with first-index ties: greater, or equal and lower index (a NaN is never better).
struct FirstIndexMax {
  template <class V>
  __device__ __forceinline__ bool operator()(V v1, int i1, V v2, int i2) const { return v1 > v2 || (v1 == v2 && i1 < i2); }
};
// over the wave, in every lane
template <class V, class Better = FirstIndexMax>
__device__ __forceinline__ void wave_best(V& v, int& i, Better better = Better()) {
  for (int off = 32; off >= 1; off >>= 1) {
    const V ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}
// over the nw slots the waves' lanes 0 stored (the caller owns the stores and the barrier behind them), by the same order
template <class V, class Better = FirstIndexMax>
__device__ __forceinline__ void best_of_waves(const V* sv, const int* si, int nw, V& v, int& i, Better better = Better()) {
  v = sv[0]; i = si[0];
  for (int q = 1; q < nw; ++q)
    if (better(sv[q], si[q], v, i)) { v = sv[q]; i = si[q]; }
}
