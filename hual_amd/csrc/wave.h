// Wave-level and LDS primitives of the HIP kernels (gfx950, wave64): the one definition of the LDS-only workgroup barrier, the lane
// exchanges and the butterfly reductions built on them.  Included by common.h.
#pragma once
#include <hip/hip_runtime.h>

// ---- workgroup barrier for LDS hand-offs only.  __syncthreads() is a workgroup-scope fence + s_barrier, and the fence makes hipcc
// wait for every outstanding global store of the wave (s_waitcnt vmcnt(0)): at one workgroup per CU that puts a store round trip in
// front of every barrier of an epilogue / every phase of a staged kernel (in the attention backward: the stores of the job before).
// The kernels that use it never read back their own global stores, so they wait for their LDS operations only.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- lane exchanges on the VALU: no ds_bpermute round trip through the LDS crossbar (~100+ cycles each, which is what __shfl_xor
// costs: at one workgroup per CU the fused kernels are latency bound and a row reduction per ds_bpermute chain was measured to
// dominate them - 15 us per conv_block layer).
// partner lane ^ step inside a 16-lane DPP row, step = 1, 2, 4, 8
__device__ __forceinline__ float dpp_xor_partner(float v, int step) {
  const int x = __builtin_bit_cast(int, v);
  int r;
  if (step == 1) r = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);          // quad_perm [1,0,3,2]
  else if (step == 2) r = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
  else if (step == 4) {
    r = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);                       // row_shl:4 -> lanes 0-3, 8-11 read lane + 4
    r = __builtin_amdgcn_update_dpp(r, x, 0x114, 0xF, 0xA, false);                       // row_shr:4 -> lanes 4-7, 12-15 read lane - 4
  } else {
    r = __builtin_amdgcn_update_dpp(x, x, 0x108, 0xF, 0x3, false);                       // row_shl:8 -> lanes 0-7 read lane + 8
    r = __builtin_amdgcn_update_dpp(r, x, 0x118, 0xF, 0xC, false);                       // row_shr:8 -> lanes 8-15 read lane - 8
  }
  return __builtin_bit_cast(float, r);
}
// partners lane ^ 16 / lane ^ 32 across the 16-lane rows (v_permlane16_swap / v_permlane32_swap, one instruction each).  `lane`: any
// value that carries the lane's bits 4 and 5 - threadIdx.x (workgroups are one-dimensional), or the lane index a kernel already holds
// in a register: with the caller's own value every kernel compiles to the instruction stream it had with its private copy
// (profiles/wave_primitives_isa.txt)
__device__ __forceinline__ float lane_xor16(float v, int lane = threadIdx.x) {
  const unsigned x = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);    // r[0]: odd rows <- even rows, r[1]: even rows <- odd rows
  return __builtin_bit_cast(float, (lane & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float lane_xor32(float v, int lane = threadIdx.x) {
  const unsigned x = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return __builtin_bit_cast(float, (lane & 32) ? r[0] : r[1]);
}

// ---- reductions: butterflies over xor 1, 2, 4, 8, 16, 32 in that order - every lane of the group gets the result, sums are
// bit-identical between lanes
// sum / maximum over the 16 lanes that share lane >> 4 (one DPP row)
__device__ __forceinline__ float fast_sum16(float v) {
  v += dpp_xor_partner(v, 1);
  v += dpp_xor_partner(v, 2);
  v += dpp_xor_partner(v, 4);
  v += dpp_xor_partner(v, 8);
  return v;
}
__device__ __forceinline__ float fast_max16(float v) {
  v = fmaxf(v, dpp_xor_partner(v, 1));
  v = fmaxf(v, dpp_xor_partner(v, 2));
  v = fmaxf(v, dpp_xor_partner(v, 4));
  v = fmaxf(v, dpp_xor_partner(v, 8));
  return v;
}
// maximum / sum over the four lanes (j, 0..3) = j + 16 g that hold one row's slice in the T-form accumulator layout (tilecore.h) and
// one query's scores in the attention tiles
__device__ __forceinline__ float slice16_max(float v, int lane = threadIdx.x) {
  v = fmaxf(v, lane_xor16(v, lane));
  return fmaxf(v, lane_xor32(v, lane));
}
__device__ __forceinline__ float slice16_sum(float v, int lane = threadIdx.x) {
  v += lane_xor16(v, lane);
  return v + lane_xor32(v, lane);
}
// sum / max across the 32 lanes sharing lane >> 5 (the row of 128 floats a half wave holds as one float4 per lane)
__device__ __forceinline__ float fast_sum32(float v) {
  v = fast_sum16(v);
  return v + lane_xor16(v);
}
__device__ __forceinline__ float fast_max32(float v) {
  v = fast_max16(v);
  return fmaxf(v, lane_xor16(v));
}
// ... and across the whole wave
__device__ __forceinline__ float wave_sum64(float v) {
  v = fast_sum32(v);
  return v + lane_xor32(v);
}
__device__ __forceinline__ float wave_max64(float v) {
  v = fast_max32(v);
  return fmaxf(v, lane_xor32(v));
}
// float64 sum across the wave: the same butterfly, each exchange moving the two halves of the partner's value
__device__ __forceinline__ double wave_sum64_f64(double v, int lane = threadIdx.x) {
#pragma unroll
  for (int step = 1; step <= 32; step <<= 1) {
    const uint2 x = __builtin_bit_cast(uint2, v);
    const float lo = __builtin_bit_cast(float, x.x), hi = __builtin_bit_cast(float, x.y);
    float plo, phi;
    if (step <= 8) { plo = dpp_xor_partner(lo, step); phi = dpp_xor_partner(hi, step); }
    else if (step == 16) { plo = lane_xor16(lo, lane); phi = lane_xor16(hi, lane); }
    else { plo = lane_xor32(lo, lane); phi = lane_xor32(hi, lane); }
    v += __builtin_bit_cast(double, make_uint2(__builtin_bit_cast(unsigned, plo), __builtin_bit_cast(unsigned, phi)));
  }
  return v;
}
// The same sum over xor 32, 16, .. 1 (ds_bpermute): another summation order, so other last bits - both stay.  Pinned to this one: the
// double sums of block.h (heads.hip, spanprob.h and its span kernels, al.hip); to the ascending one above: the column sums of spanconf.hip.
__device__ __forceinline__ double wave_sum64_f64_desc(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// The same maximum (max is exact and commutative: identical results) with its last step through the LDS crossbar (ds_bpermute): the
// form the workgroup maxima of the context-query kernels (cq_wgmax_put), of block.h (BlockMaxF: heads.hip, al.hip, and spanprob.h for
// topk.hip and spanconf.hip) and the V maximum of the attention backward are compiled with.  Ending them on lane_xor32 gives 15
// kernels another instruction stream, 11 of them outside the benchmark step (profiles/wave_primitives_isa.txt: instruction counts in
// both forms); a caller moves to wave_max64 together with a timing of its kernels against this form.  New code uses wave_max64.
__device__ __forceinline__ float wave_max64_bperm(float v) {
  v = fast_max32(v);
  return fmaxf(v, __shfl_xor(v, 32));
}
