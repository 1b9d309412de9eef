// Building blocks of the fused multi-layer kernels (convblock.hip, dablock.hip, mproj.hip): a workgroup of 512 threads keeps a tile of
// activation rows in LDS as pre-split fp16 operand planes (bf16x3.h "f16x3"); the weights never touch LDS - wave w holds the
// fragments of ITS 16 output columns of the current [128,128] weight in registers, loaded one step ahead straight from the
// fragment-major T / N images in L2 ("T-form", tf_* below), and multiplies them against all row tiles of the workgroup.
#pragma once
#include "common.h"
#include "rowops.h"
#include "bf16x3.h"
#include "philox.h"

// ---- kernel arguments (what round 3 measured).  A scalar load of a kernel-argument line that is not in the
// scalar cache yet is a full memory round trip (~1.5 us), and the compiler sinks those loads to the first use: a kernel that WALKS
// a large argument struct pays one per step - mproj copies its step descriptors to LDS once (vector loads) and reads them back with
// readfirstlane.  A pointer that went through LDS / readfirstlane / an asm barrier has lost its address space: loads and stores
// through it are FLAT instructions, which count in lgkmcnt as well as vmcnt (every LDS wait then waits for them too) - use
// ld4_global / st4_global (common.h) with such pointers.

// ---- debug: in-kernel phase timestamps (-DHUAL_STAMPS, scripts/exp/stamps.py).  Thread 0 of every workgroup writes the
// shader clock at phase boundaries into a device-global table read back through hual_debug_stamps().
#ifdef HUAL_STAMPS
#define HUAL_STAMP_SLOTS 64
static __device__ unsigned long long g_hual_stamps[512 * HUAL_STAMP_SLOTS];      // one table per translation unit
// HUAL_STAMPS selects the kernel that writes: 2 conv_block_fwd_kernel, 3 conv_block_bwd_kernel, 9 mproj kernels carry stamps (build:
// HUAL_STAMPS=<n> python -m hual_amd.build), 4 ln_proj_bwd_kernel (round 5) and the ln_proj tail of conv_block_fwd (id 2, slots 26 ..) too; ids 1 / 5 / 6 are reserved for da_post / da_mid_bwd / ln_proj, whose stamps
// are put in for a measurement with HUAL_STAMP_K(id, slot) at the phase boundaries and taken out again
// -DHUAL_STAMPS_FIRST: a slot keeps its FIRST stamp since hual_debug_stamps_reset() - the first launch of the kernel in the step that
// follows the reset instead of the last one
#ifdef HUAL_STAMPS_FIRST
#define HUAL_STAMP_KEEP(slot) ((slot) == 0ull)
#else
#define HUAL_STAMP_KEEP(slot) true
#endif
#define HUAL_STAMP_K(k, i) do { if (HUAL_STAMPS == (k) && threadIdx.x == 0 && blockIdx.x < 512 && (i) < HUAL_STAMP_SLOTS && HUAL_STAMP_KEEP(g_hual_stamps[blockIdx.x * HUAL_STAMP_SLOTS + (i)])) g_hual_stamps[blockIdx.x * HUAL_STAMP_SLOTS + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define HUAL_STAMP_K(k, i) do { } while (0)
#endif
#define HUAL_STAMP(i) HUAL_STAMP_K(1, i)

#define LN_EPS 1e-6f   // models/layers.py:15
#define CB_THREADS 512

__device__ __forceinline__ float4 cb_fma(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 cb_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 cb_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float cb_hsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// ---- dropout with the Philox key / offset held in registers ---------------------------------------------------------------
// philox.h's drop_mask4 reads the three state words from global memory on every call; in a latency-bound fused kernel that
// is a memory round trip per call (and, next to an LDS-DMA in flight, a vmcnt(0) that also waits for every store issued
// before it).  The fused kernels read the state once at entry.
struct DropRegs { uint32_t k0, k1, off, thresh, t16; float scale; int enabled; };
__device__ __forceinline__ DropRegs drop_load(const hual::DropCfg& d) {
  DropRegs r;
  r.enabled = d.enabled; r.thresh = d.thresh; r.scale = d.scale; r.k0 = 0; r.k1 = 0; r.off = 0;
  // 16-bit threshold of the row-local sites (oracle/philox.py keep_threshold16): round(keep_prob * 65536) in [1, 65536]
  const uint32_t t = (uint32_t)(((uint64_t)d.thresh + (1ull << 15)) >> 16);
  r.t16 = t < 1u ? 1u : (t > 65536u ? 65536u : t);
  if (d.enabled) {
    // scalar loads (constant address space: the state is only written by the optimizer launch): a vector load + readfirstlane
    // here is waited for on the spot - a memory round trip at the top of every fused kernel before its operand loads are issued
    const __attribute__((address_space(4))) uint32_t* sp = (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)d.state;
    r.k0 = sp[0]; r.k1 = sp[1]; r.off = sp[2];
  }
  return r;
}
// Dropout decisions of the row-local sites inside the fused kernels: ONE Philox call decides the 8 consecutive columns
// 8 col8 .. 8 col8 + 7 of a row from its eight 16-bit halves (element e = col & 7: word e >> 1, half e & 1; kept iff half <
// t16) - bit e of the result.  Half the generator work per element of the 32-bit scheme of philox.h, keep probability
// t16 / 65536 (0.800003 for rate 0.2; tf.nn.dropout's own float32 uniform is no finer than 2^-23).
__device__ __forceinline__ uint32_t drop_bits8_r(const DropRegs& d, uint32_t site, uint32_t row, uint32_t col8) {
  const uint4_ r = philox4x32(col8, row, site, d.off, d.k0, d.k1);
  const uint32_t t = d.t16;
  return ((r.x & 0xffffu) < t ? 1u : 0u) | ((r.x >> 16) < t ? 2u : 0u) | ((r.y & 0xffffu) < t ? 4u : 0u) | ((r.y >> 16) < t ? 8u : 0u) |
         ((r.z & 0xffffu) < t ? 16u : 0u) | ((r.z >> 16) < t ? 32u : 0u) | ((r.w & 0xffffu) < t ? 64u : 0u) | ((r.w >> 16) < t ? 128u : 0u);
}
__device__ __forceinline__ uint32_t dpp_xor1_u32(uint32_t v) { return __builtin_bit_cast(uint32_t, dpp_xor_partner(__builtin_bit_cast(float, v), 1)); }
// Keep nibbles (bit c = column 4 col4 + c) of this lane's four columns for the TWO rows rowA and rowB.  The lanes col4 and
// col4 ^ 1 (DPP neighbours in both layouts of the fused kernels: the 32-lane row layout, col4 = lane & 31, and the
// accumulator layout, col4 = 16 ch + (lane & 15)) share an 8-column group: the even one draws rowA's call, the odd one
// rowB's, and they swap the halves.  All lanes of the wave must be active.
__device__ __forceinline__ uint32_t drop_nib2_r(const DropRegs& d, uint32_t site, uint32_t rowA, uint32_t rowB, uint32_t col4, uint32_t& nibA,
                                                uint32_t& nibB) {
  const bool odd = (col4 & 1u) != 0u;
  const uint32_t b = drop_bits8_r(d, site, odd ? rowB : rowA, col4 >> 1);
  const uint32_t o = dpp_xor1_u32(b);
  nibA = odd ? (o >> 4) : (b & 15u);
  nibB = odd ? (b >> 4) : (o & 15u);
  return b;        // the whole byte of the bit plane for (odd ? rowB : rowA, col4 >> 1)
}
// the same pairing for two (site, row) pairs - the two roles of a row at the trilinear sites (ops.py:104), or two rows of different sites
__device__ __forceinline__ void drop_nib2_sites_r(const DropRegs& d, uint32_t siteA, uint32_t rowA, uint32_t siteB, uint32_t rowB, uint32_t col4,
                                                  uint32_t& nibA, uint32_t& nibB) {
  const bool odd = (col4 & 1u) != 0u;
  const uint32_t b = drop_bits8_r(d, odd ? siteB : siteA, odd ? rowB : rowA, col4 >> 1);
  const uint32_t o = dpp_xor1_u32(b);
  nibA = odd ? (o >> 4) : (b & 15u);
  nibB = odd ? (b >> 4) : (o & 15u);
}
// the same + the keep bytes stored into `plane` (rows are indices into the plane; rowoff = RNG row - plane row)
__device__ __forceinline__ void drop_nib2_store_r(const DropRegs& d, uint32_t site, uint32_t rowoff, int rowA, int rowB, bool okA, bool okB,
                                                  uint32_t col4, uint8_t* plane, uint32_t& nibA, uint32_t& nibB) {
  const uint32_t b = drop_nib2_r(d, site, rowoff + (uint32_t)rowA, rowoff + (uint32_t)rowB, col4, nibA, nibB);
  const bool odd = (col4 & 1u) != 0u;
  if (plane && (odd ? okB : okA)) plane[(size_t)(odd ? rowB : rowA) * 16 + (col4 >> 1)] = (uint8_t)b;
}

// ---- bit planes of a [R,128] tensor (dropout keep bits, relu active sets): byte [row * 16 + (col >> 3)], bit col & 7 - 16 bytes
// per row.  In both layouts of the fused kernels a lane holds 4 consecutive columns of a row (col4 = col >> 2) and its DPP
// neighbour col4 ^ 1 the other half of the byte.
__device__ __forceinline__ uint32_t bits_nibble(const uint8_t* plane, int row, int col4) {
  return ((uint32_t)plane[(size_t)row * 16 + (col4 >> 1)] >> (4 * (col4 & 1))) & 15u;
}
// nibbles of TWO rows -> bytes: the even lane of a pair stores rowA's byte, the odd lane rowB's (okA / okB: row is stored)
__device__ __forceinline__ void bits_store2(uint8_t* plane, int rowA, int rowB, bool okA, bool okB, int col4, uint32_t nibA, uint32_t nibB) {
  const bool odd = (col4 & 1) != 0;
  const uint32_t mine = nibA | (nibB << 4);                  // even lane: [A lo | B lo], odd lane: [A hi | B hi]
  const uint32_t other = dpp_xor1_u32(mine);
  const uint32_t byte = odd ? ((other >> 4) | (mine & 0xf0u)) : ((mine & 15u) | ((other & 15u) << 4));
  if (odd ? okB : okA) plane[(size_t)(odd ? rowB : rowA) * 16 + (col4 >> 1)] = (uint8_t)byte;
}
__device__ __forceinline__ float4 f4_select(uint32_t nib, float4 v) {
  return make_float4((nib & 1u) ? v.x : 0.f, (nib & 2u) ? v.y : 0.f, (nib & 4u) ? v.z : 0.f, (nib & 8u) ? v.w : 0.f);
}
// dropout of a lane's four columns: keep nibble `nib`, survivors scaled by `scale` = 1 / keep probability (f4scale1, bf16x3.h)
__device__ __forceinline__ float4 drop_scale(uint32_t nib, float4 v, float scale) { return f4_select(nib, f4scale1(v, scale)); }
__device__ __forceinline__ uint32_t f4_posbits(float4 v) {
  return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
}

// clip segment [lo, hi) of unified row `row` (rowops.h RowSpace)
__device__ __forceinline__ void cb_segment(int row, const hual::RowSpace& rs, int& lo, int& hi) {
  const bool v = row < rs.Nv;
  const int n = v ? rs.T : rs.L, base = v ? 0 : rs.Nv;
  lo = base + __mul24(small_div(row - base, n), n);
  hi = lo + n;
}

// ---- "T-form" tile product: register-resident weights -----------------------------------------------------------------
// Y^T = W^T . X^T: the weight block is the MFMA's A operand (M = output columns), the activation rows are its B operand
// (N = rows).  Wave `ws` of a workgroup owns the 16 output columns 16 ws .. 16 ws + 15 for ALL row tiles of the workgroup:
//   * its weight fragments (16 columns x 128 k, hi + lo = 32 registers) come STRAIGHT from the L2-resident image into
//     registers with 16-byte global loads - requested a whole step ahead, no LDS staging, no DMA wait, no barrier for weights;
//   * the activation fragments are plain ds_read_b128 of the row-major operand planes (lane (j, g): row j, k 8 g .. 8 g + 7
//     of a 32-deep step) - no transposed reads; every wave reads all rows (24 KB per 48 rows and step);
//   * accumulator rt, element r of lane (j, g) = row 16 rt + j, column 16 ws + 4 g + r: four ADJACENT columns of one row.
// Images (pack_weights_kernel, one 64 KB block per 128 contraction indices): fp16 high parts and residuals of element [output
// column c][contraction index i] in the fragment-major byte order of tf_img_off below.  For a forward product the block is W^T (c = n, i = k: "T image"),
// for dX = dY . W^T it is W itself (c = k, i = n: "N image").  Values are scaled by 2^HUAL_F16_WSCALE_LOG2 as in the LDS images.
// Byte order inside a block ("fragment major"): the 16 bytes lane (j, g) = lane j + 16 g of wave ws loads for k-step ks - column
// 16 ws + j, indices 32 ks + 8 g .. + 7 - sit at ((ws * 4 + ks) * 2 + plane) * 1024 + 16 * lane, plane 0 = high parts, 1 = residuals:
// every load instruction of tf_load_w reads ONE contiguous KB (8 full cache lines).  In the [column][index] order of the first
// version an instruction touched 16 half lines 256 B apart, and the halves were fetched again by the next k-step (8 waves x 8 KB
// of fragments thrash the 32 KB L1): 8.1 M L1 requests per da_post launch against 1.8 M of an ln_proj launch (TCP_UTCL1_REQUEST).
#define TF_BLOCK 65536
__host__ __device__ __forceinline__ int tf_img_off(int c, int i) {      // byte offset of the high part of element (column c, index i)
  return (((c >> 4) * 4 + (i >> 5)) * 2) * 1024 + ((((i >> 3) & 3) * 16 + (c & 15)) * 16) + 2 * (i & 7);
}
#define TF_LO_OFF 1024                                                   // ... its residual
struct TfW { f16x8 h[4], l[4]; };
__device__ __forceinline__ f16x8 tf_ld16(const char* p) { return __builtin_bit_cast(f16x8, ld4_global(p)); }
__device__ __forceinline__ void tf_load_w(TfW& w, const void* img, int ws, int lane) {
  const char* p = reinterpret_cast<const char*>(img) + 8192 * ws + 16 * lane;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    w.h[ks] = tf_ld16(p + 2048 * ks);
    w.l[ks] = tf_ld16(p + 2048 * ks + TF_LO_OFF);
  }
}
// the same through a buffer resource: `live` false gives a resource of zero bytes - the eight loads are issued (straight-line code, the
// compiler counts them) but touch no memory and return zeros.  For "prefetch the NEXT weights, if there are any" without a branch
__device__ __forceinline__ void tf_load_w_if(TfW& w, const void* img, bool live, int ws, int lane) {
  const __amdgpu_buffer_rsrc_t r = row_rsrc(img, live ? (uint32_t)TF_BLOCK : 0u);
  const uint32_t off = 8192u * (uint32_t)ws + 16u * (uint32_t)lane;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    w.h[ks] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off + 2048u * ks, 0, 0));
    w.l[ks] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off + 2048u * ks + TF_LO_OFF, 0, 0));
  }
}
// acc[rt] = (this wave's columns of) rows 16 rt .. 16 rt + 15 of the operand planes (hi at Ahi, lo at Ahi + ALO) . block
template <int NT, int ALO>
__device__ __forceinline__ void tf_mma(const char* Ahi, const TfW& w, int lane, f32x4 (&acc)[NT]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f16x8 xh[NT], xl[NT];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      const int off = tile256_off(16 * rt + j, 4 * ks + g);
      xh[rt] = *reinterpret_cast<const f16x8*>(Ahi + off);
      xl[rt] = *reinterpret_cast<const f16x8*>(Ahi + ALO + off);
    }
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], xh[rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], xl[rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[ks], xh[rt], acc[rt], 0, 0, 0);
    }
  }
}

// the same with the activation fragments of at most two k-steps live (the fully unrolled form above lets the scheduler hoist the
// reads of all four: 32 registers per row tile) - for kernels that hold many tiles in registers across the product
template <int NT, int ALO>
__device__ __forceinline__ void tf_mma_lean(const char* Ahi, const TfW& w, int lane, f32x4 (&acc)[NT]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f16x8 xh[2][NT], xl[2][NT];
  auto rd = [&](int b, int ks) {
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      const int off = tile256_off(16 * rt + j, 4 * ks + g);
      xh[b][rt] = *reinterpret_cast<const f16x8*>(Ahi + off);
      xl[b][rt] = *reinterpret_cast<const f16x8*>(Ahi + ALO + off);
    }
  };
  rd(0, 0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (ks < 3) rd((ks + 1) & 1, ks + 1);
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], xh[ks & 1][rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], xl[ks & 1][rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[ks], xh[ks & 1][rt], acc[rt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the activation fragments of ALL four k-steps in registers (32 per row tile), for a run of products that read the same operand slot:
// every wave reads the whole slot per product (8 waves x 24 KB at three row tiles = 1536 cycles of the CU's LDS bandwidth, more than the
// 1152 cycles its MFMAs take), so projections that share a source read it once
template <int NT> struct TfA { f16x8 h[4][NT], l[4][NT]; };
template <int NT, int ALO>
__device__ __forceinline__ void tf_load_a(TfA<NT>& x, const char* Ahi, int lane) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      const int off = tile256_off(16 * rt + j, 4 * ks + g);
      x.h[ks][rt] = *reinterpret_cast<const f16x8*>(Ahi + off);
      x.l[ks][rt] = *reinterpret_cast<const f16x8*>(Ahi + ALO + off);
    }
}
template <int NT>
__device__ __forceinline__ void tf_mma_regs(const TfA<NT>& x, const TfW& w, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], x.h[ks][rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[ks], x.l[ks][rt], acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[ks], x.h[ks][rt], acc[rt], 0, 0, 0);
    }
}

// drop_nib2_store_r for the T-form accumulator layout: col4 = 4 wave + (lane >> 4), the lane with the other half of the 8-column group
// is lane ^ 16.  The even lane of the pair draws rowA's call, the odd one rowB's (rowB = rowA with okB = false: a single row - both
// draw the same call); all lanes of the wave must be active
__device__ __forceinline__ void drop_nib2_store_t(const DropRegs& d, uint32_t site, uint32_t rowoff, int rowA, int rowB, bool okA, bool okB,
                                                  uint32_t col4, uint8_t* plane, uint32_t& nibA, uint32_t& nibB, int lane) {
  const bool odd = (col4 & 1u) != 0u;
  const uint32_t b = drop_bits8_r(d, site, rowoff + (uint32_t)(odd ? rowB : rowA), col4 >> 1);
  const uint32_t o = __builtin_bit_cast(uint32_t, lane_xor16(__builtin_bit_cast(float, b), lane));
  nibA = odd ? (o >> 4) : (b & 15u);
  nibB = odd ? (b >> 4) : (o & 15u);
  if (plane && (odd ? okB : okA)) plane[(size_t)(odd ? rowB : rowA) * 16 + (col4 >> 1)] = (uint8_t)b;
}
// bits_store2 for the T-form accumulator layout (col4 = 4 wave + (lane >> 4): the other half of the byte lives in lane ^ 16)
__device__ __forceinline__ void bits_store2_t(uint8_t* plane, int rowA, int rowB, bool okA, bool okB, int col4, uint32_t nibA, uint32_t nibB, int lane) {
  const bool odd = (col4 & 1) != 0;
  const uint32_t mine = nibA | (nibB << 4);                  // even lane: [A lo | B lo], odd lane: [A hi | B hi]
  const uint32_t other = __builtin_bit_cast(uint32_t, lane_xor16(__builtin_bit_cast(float, mine), lane));
  const uint32_t byte = odd ? ((other >> 4) | (mine & 0xf0u)) : ((mine & 15u) | ((other & 15u) << 4));
  if (odd ? okB : okA) plane[(size_t)(odd ? rowB : rowA) * 16 + (col4 >> 1)] = (uint8_t)byte;
}
// keep nibbles of the lane's NT rows row0 + 16 rt (row0 = first row of the workgroup + lane & 15) at a dropout site of the T-form
// accumulator layout, + the keep bytes of the rows < RE into the plane: ceil(NT / 2) calls per lane
template <int NT>
__device__ __forceinline__ void drop_rows_t(const DropRegs& d, uint32_t site, uint32_t rowoff, int row0, int RE, uint32_t col4, uint8_t* plane,
                                            uint32_t (&nib)[NT], int lane) {
#pragma unroll
  for (int c = 0; c < (NT + 1) / 2; ++c) {
    const bool two = 2 * c + 1 < NT;
    const int ra = row0 + 32 * c, rb = two ? ra + 16 : ra;
    uint32_t na, nb;
    drop_nib2_store_t(d, site, rowoff, ra, rb, ra < RE, two && rb < RE, col4, plane, na, nb, lane);
    nib[2 * c] = na;
    if (two) nib[2 * c + 1] = nb;
  }
}

// row of the operand planes: scale to fp16 range, split, store (8 bytes per lane and plane); returns the inverse scale
// the same with a FIXED power-of-two scale (2^4) for rows whose magnitude is bounded by construction (layer-norm outputs and depthwise
// taps of them: |x| < 2^12 - beyond it the fp16 image overflows to inf and the losses come out NaN): no row maximum, no butterfly
#define CB_FIXED_SCALE 16.0f
__device__ __forceinline__ float cb_store_operand_fx(char* Ahi, char* Alo, int arow, int l32, float4 v) {
  uint2 h, l;
  f16_split4(f4scale1(v, CB_FIXED_SCALE), h, l);
  const int off = tile256_off(arow, l32 >> 1) + 8 * (l32 & 1);
  *reinterpret_cast<uint2*>(Ahi + off) = h;
  *reinterpret_cast<uint2*>(Alo + off) = l;
  return 1.0f / (CB_FIXED_SCALE * HUAL_F16_WSCALE);
}
__device__ __forceinline__ float cb_store_operand(char* Ahi, char* Alo, int arow, int l32, float4 v) {
  float inv;
  const float sc = f16_row_scale(fast_max32(f4absmax(v)), inv);
  uint2 h, l;
  f16_split4(f4scale1(v, sc), h, l);
  const int off = tile256_off(arow, l32 >> 1) + 8 * (l32 & 1);
  *reinterpret_cast<uint2*>(Ahi + off) = h;
  *reinterpret_cast<uint2*>(Alo + off) = l;
  return inv;
}

