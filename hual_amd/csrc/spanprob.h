// The span distribution's probability stage, shared by every span kernel outside the forward - the per-clip launches through spanclip.h
// (topk.hip, spanconf.hip, spanhit.hip), the span-posterior launches through spanpost.h -: the masked softmaxes of
// the start / end logits exactly as the span stage of heads_kernel computes them (same masking, the same code for the max and the
// double-sum reductions - block.h -, same rounding), so every kernel that includes this sees the numbers of hual_span_argmax bit for bit.
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

// (uniform) the live rule of every launch that normalises by the triangle's mass Z: every weight underflowed (Z == 0), or an infinite
// logit made Z Inf or NaN - as a poisoned row.  Each launch sums its own Z (float32 products in spanconf.hip, float64 ones in
// spanhit.hip and spanpost.h): they can differ where a float32 product underflows.
__device__ __forceinline__ bool span_mass_live(double Z) { return Z > 0.0 && Z < INFINITY; }

// ps / pe [256] (LDS) <- softmax of the masked logits of one clip, 1 <= v <= T <= 256, thread t's start / end logit given by start() /
// end() (called at t < v only): read from memory by span_probabilities below, a register's value scaled by 1 / tau in
// hual_al_evidence_grid (spancalib.hip) - one body, so the same logits give the same bits.  smf [2 * SPAN_WAVES] floats and smd
// [2 * SPAN_WAVES] doubles of LDS scratch, FRESH: a caller that has read them, or ps / pe, puts a barrier in front.  Called by all
// SPAN_THREADS threads; ends on a barrier, after which ps / pe are readable.
// NW: the waves of the calling workgroup - SPAN_WAVES, or 4 in a 256-thread workgroup (gradembed.hip): waves 4.. of the wide form
// hold no frame and add -inf to the max and exact zeros to the sum, in the same ascending fold, so both widths give the same bits.
// heads_kernel's span stage (mask_logits, reproducible softmax; oracle/seqpan_ref.py::softmax_cr)
template <int NW = SPAN_WAVES, class Start, class End>
__device__ __forceinline__ void span_probabilities_of(Start start, End end, int T, int v, float* ps, float* pe, float* smf, double* smd) {
  const int t = threadIdx.x;
  const bool in = t < T;
  float zs = -INFINITY, ze = -INFINITY;
  if (in) {
    zs = t < v ? start() : HUAL_MASK_VALUE;           // (= x * 0 + HUAL_MASK_VALUE for a finite padding logit, never read here)
    ze = t < v ? end() : HUAL_MASK_VALUE;
  }
  // (smf / smd are fresh: no barrier in front.  Waves 4.. contribute -inf and exact zeros, as waves 4 - 7 of heads_kernel do)
  float mxs = zs, mxe = ze;
  block_reduce<BlockMaxF, NW, false>(mxs, mxe, smf);
  const float xs = in ? (float)exp((double)(zs - mxs)) : 0.f;
  const float xe = in ? (float)exp((double)(ze - mxe)) : 0.f;
  double dss = (double)xs, dse = (double)xe;
  block_reduce<BlockSumD, NW, false>(dss, dse, smd);
  if (t < 256) {
    ps[t] = __fdiv_rn(xs, (float)dss);
    pe[t] = __fdiv_rn(xe, (float)dse);
  }
  __syncthreads();
}

// the same of the logits of the clip at `row` of zs_ / ze_
__device__ __forceinline__ void span_probabilities(const float* __restrict__ zs_, const float* __restrict__ ze_, size_t row, int T, int v,
                                                   float* ps, float* pe, float* smf, double* smd) {
  const int t = threadIdx.x;
  span_probabilities_of([&] { return zs_[row + t]; }, [&] { return ze_[row + t]; }, T, v, ps, pe, smf, smd);
}
