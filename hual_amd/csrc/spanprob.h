// The span distribution's probability stage, shared by the per-clip span kernels (topk.hip, spanconf.hip): the masked softmaxes of
// the start / end logits exactly as the span stage of heads_kernel computes them (same masking, same max / double-sum reduction
// trees, same rounding), so every kernel that includes this sees the numbers of hual_span_argmax bit for bit.
#pragma once
#include "common.h"

constexpr int SPAN_THREADS = 1024;      // one workgroup per clip, 16 waves: four per SIMD hide each other's LDS latency
constexpr int SPAN_WAVES = SPAN_THREADS / 64;

// video_seq_len as the span kernels read it: > T reads as T, < 1 as an empty clip
__device__ __forceinline__ int span_clip_len(int vr, int T) { return vr < 1 ? 0 : (vr > T ? T : vr); }

// (uniform) a NaN logit at some t < v: the poison rule of hual_span_argmax.  One barrier.
__device__ __forceinline__ int span_row_poisoned(const float* __restrict__ zs_, const float* __restrict__ ze_, size_t row, int v) {
  const int t = threadIdx.x;
  return __syncthreads_or(t < v && (zs_[row + t] != zs_[row + t] || ze_[row + t] != ze_[row + t]));
}

// ps / pe [256] (LDS) <- softmax of the masked logits of the clip at `row`, 1 <= v <= T <= 256; smf [2 * SPAN_WAVES] floats and smd
// [2 * SPAN_WAVES] doubles of LDS scratch.  Called by all SPAN_THREADS threads; ends on a barrier, after which ps / pe are readable.
// heads_kernel's span stage (mask_logits, reproducible softmax; oracle/seqpan_ref.py::softmax_cr)
__device__ __forceinline__ void span_probabilities(const float* __restrict__ zs_, const float* __restrict__ ze_, size_t row, int T, int v,
                                                   float* ps, float* pe, float* smf, double* smd) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const bool in = t < T;
  float zs = -INFINITY, ze = -INFINITY;
  if (in) {
    zs = t < v ? zs_[row + t] : HUAL_MASK_VALUE;      // (= x * 0 + HUAL_MASK_VALUE for a finite padding logit, never read here)
    ze = t < v ? ze_[row + t] : HUAL_MASK_VALUE;
  }
  float mxs = wave_max64_bperm(zs), mxe = wave_max64_bperm(ze);
  if (lane == 0) { smf[w] = mxs; smf[SPAN_WAVES + w] = mxe; }
  __syncthreads();
  mxs = -INFINITY; mxe = -INFINITY;
  for (int q = 0; q < SPAN_WAVES; ++q) { mxs = fmaxf(mxs, smf[q]); mxe = fmaxf(mxe, smf[SPAN_WAVES + q]); }
  const float xs = in ? (float)exp((double)(zs - mxs)) : 0.f;
  const float xe = in ? (float)exp((double)(ze - mxe)) : 0.f;
  double dss = (double)xs, dse = (double)xe;
  for (int off = 32; off >= 1; off >>= 1) { dss += __shfl_xor(dss, off); dse += __shfl_xor(dse, off); }
  if (lane == 0) { smd[w] = dss; smd[SPAN_WAVES + w] = dse; }
  __syncthreads();
  dss = 0.0; dse = 0.0;
  for (int q = 0; q < SPAN_WAVES; ++q) { dss += smd[q]; dse += smd[SPAN_WAVES + q]; }      // (waves 4.. add exact zeros, as in heads_kernel)
  if (t < 256) {
    ps[t] = __fdiv_rn(xs, (float)dss);
    pe[t] = __fdiv_rn(xe, (float)dse);
  }
  __syncthreads();
}
