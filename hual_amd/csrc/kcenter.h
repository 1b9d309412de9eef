// The k-center step shared by hual_kcenter_greedy and hual_kcenter_sample (kcenter.hip, include/hual_seqpan.h): core-set selection
// in a feature space, weighted by a per-row score.  Step s picks the eligible row of maximal (score, w[i], -i); the score is
// w[i] * mind[i] (greedy), or that divided by a unit exponential drawn per (step, row) (SAMPLE: the argmax is then a draw
// proportional to w * mind - D^2 sampling, k-means++ seeding), mind[i] the squared distance of row i to its nearest center so far.
// With ORIGIN the zero vector is a center before the first pick.  The whole selection is one C call: an opening launch, one
// update-only launch per init row, one launch per step and one closing update, all on the caller's stream, no host synchronisation
// in between.
//
// A step is ONE launch over cdiv(N, 16) workgroups of four waves.  Every workgroup
//   1. stages the newest center's row in LDS - its index is read from picked[s - 1] in device memory and range-checked: anything
//      outside [0, N) (the -1 of an exhausted selection) makes the update a no-op;
//   2. updates mind / assign of its 16 rows: one wave per row, the row's chunks of four floats dealt to the lanes (chunk c to lane
//      c % 64, in ascending c), the lanes' sums folded by wave_sum64 - an order that depends on D alone, so bit-equal rows get
//      bit-equal distances wherever they sit;
//   3. reduces its rows' keys to one partial, publishes it (plain store, agent-scope release) and draws a ticket from a device-scope
//      counter.  The workgroup that draws the last ticket (agent-scope acquire) reduces the partials, writes picked[s] and
//      pick_dist[s], marks the row taken and returns the counter to zero.
// No workgroup ever waits for another one: the ticket is a fetch-add whose value decides who reduces, nothing polls.  The keys are a
// total order (the row index is unique), so the pick does not depend on which workgroup arrives last or in what order partials are
// folded: a second launch returns equal bits.  The exponentials are a function of (seed, offset, step, row) alone.
#pragma once
#include "common.h"
#include "philox.h"

namespace {

constexpr int KC_THREADS = 256;      // four waves
constexpr int KC_ROWS = 16;          // rows per workgroup: four per wave, their loads in flight together
constexpr int KC_MAXD = 4096;

struct KcKey {                       // (score, w, -idx): idx < 0 is "no eligible row"
  float score, w;
  int idx;
  float mind;                        // the row's mind, carried for pick_dist
};

__device__ __forceinline__ bool kc_better(const KcKey& a, const KcKey& b) {
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  if (a.score != b.score) return a.score > b.score;
  if (a.w != b.w) return a.w > b.w;
  return a.idx < b.idx;
}

struct KcArgs {
  const float* x;
  const float* weight;               // null: every weight 1
  int N, D, ld, vec;                 // vec: rows are 16-byte aligned and D % 4 == 0 -> float4 loads
  float* mind;
  int32_t* assign;
  int32_t* taken;                    // workspace: 0 free, 1 center (init or picked), 2 a row with a non-finite feature
  uint32_t* counter;                 // workspace: [0] the ticket counter, [1] "a center exists"
  float4* partial;                   // workspace: one key per workgroup
  int32_t* picked;
  float* pick_dist;
};

struct KcRng {                       // SAMPLE: the Philox key (the seed's two halves) and counter word c3
  uint32_t k0, k1, offset;
};

// the four floats of chunk c of a row (columns 4c .. 4c + 3; beyond D: zeros, which add an exact +0 to the sum)
__device__ __forceinline__ float4 kc_chunk(const float* row, int c, int D, int vec) {
  if (vec) return ld4(row + 4 * c);
  const int k = 4 * c;
  return make_float4(row[k], k + 1 < D ? row[k + 1] : 0.f, k + 2 < D ? row[k + 2] : 0.f, k + 3 < D ? row[k + 3] : 0.f);
}

// d + the squared differences of one chunk, in the distance routine's order (x, y, z, w): a rounded product and a rounded sum each,
// never a fused multiply-add - as the step kernel has always been compiled, now said, so that the opening launch of ORIGIN (the
// same routine against a zero center) cannot be contracted differently
__device__ __forceinline__ float kc_chunk_dist(float d, const float4 v, const float4 cv) {
  const float dx = v.x - cv.x, dy = v.y - cv.y, dz = v.z - cv.z, dw = v.w - cv.w;
  d = __fadd_rn(d, __fmul_rn(dx, dx));
  d = __fadd_rn(d, __fmul_rn(dy, dy));
  d = __fadd_rn(d, __fmul_rn(dz, dz));
  d = __fadd_rn(d, __fmul_rn(dw, dw));
  return d;
}

// SAMPLE: the unit exponential of row i at step s, E = float32(-ln((k + 0.5) 2^-24)) evaluated in float64, k the top 24 bits of word x
// of the call (c0 = s, c1 = i, c2 = HUAL_SITE_SELECT, c3 = offset; key = seed): (k + 0.5) 2^-24 lies in (0, 1), so 0 < E < 17.4
__device__ __forceinline__ float kc_exponential(const KcRng& rng, int s, int i) {
  const uint4_ r = philox4x32((uint32_t)s, (uint32_t)i, (uint32_t)HUAL_SITE_SELECT, rng.offset, rng.k0, rng.k1);
  return (float)(-log(((double)(r.x >> 8) + 0.5) * (1.0 / 16777216.0)));
}

// opening launch: mind = +inf, assign = -1, taken = 0 (2 for a row that holds a NaN or an infinity: d(i, i) is then NaN, and such a
// row is never eligible), the counter and the center flag zero.  ORIGIN: the zero vector is a center - mind = |x_i|^2 in the distance
// routine's own order (chunk to lane, one butterfly: d(i, 0) bit for bit), assign stays -1 ("the origin"), the center flag is set
template <bool ORIGIN>
__global__ __launch_bounds__(KC_THREADS) void kcenter_open_kernel(KcArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = (a.D + 3) >> 2;
  if (blockIdx.x == 0 && threadIdx.x < 2) a.counter[threadIdx.x] = ORIGIN && threadIdx.x == 1 ? 1u : 0u;
  for (int r = 0; r < KC_ROWS / 4; ++r) {
    const int row = blockIdx.x * KC_ROWS + wave * (KC_ROWS / 4) + r;
    if (row >= a.N) break;                                   // (wave-uniform)
    const float* p = a.x + (size_t)row * a.ld;
    float acc = 0.f, d = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
      const float4 v = kc_chunk(p, c, a.D, a.vec);
      acc += (v.x - v.x) + (v.y - v.y) + (v.z - v.z) + (v.w - v.w);      // 0, or NaN for a NaN or an infinity
      if (ORIGIN) d = kc_chunk_dist(d, v, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    acc = wave_sum64(acc);
    if (ORIGIN) d = wave_sum64(d);
    if (lane == 0) {
      a.mind[row] = ORIGIN ? d : __builtin_huge_valf();
      a.assign[row] = -1;
      a.taken[row] = acc == 0.f ? 0 : 2;
    }
  }
}

// update with the center whose index stands at *csrc (null: none), then - select - the pick of step s
template <bool SAMPLE, bool ORIGIN>
__global__ __launch_bounds__(KC_THREADS) void kcenter_step_kernel(KcArgs a, const int32_t* csrc, int mark, int select, int s, KcRng rng) {
  __shared__ __attribute__((aligned(16))) float smem[KC_MAXD + 4 * 4 + 4];
  float* cen = smem;
  float* wkey = smem + KC_MAXD;                              // four waves' keys, then the "I am last" word
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = (a.D + 3) >> 2;
  int c_idx = csrc ? csrc[0] : -1;
  if (c_idx < 0 || c_idx >= a.N) c_idx = -1;                 // range check: an index from memory never becomes an address unchecked
  const bool has_center = ORIGIN || c_idx >= 0 || a.counter[1] != 0u;  // (counter[1] is only ever set to 1: by the opening launch with ORIGIN, else only in launches where c_idx >= 0)
  if (c_idx >= 0) {
    const float* cp = a.x + (size_t)c_idx * a.ld;
    for (int k = tid; k < 4 * nchunk; k += KC_THREADS) cen[k] = k < a.D ? cp[k] : 0.f;
    if (blockIdx.x == 0 && tid == 0) {
      a.counter[1] = 1u;
      if (mark) a.taken[c_idx] = 1;
    }
    __syncthreads();
  }
  // ---- the wave's four rows: distances to the center, loads of the four rows in flight together
  const int row0 = blockIdx.x * KC_ROWS + wave * 4;
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (c_idx >= 0) {
    const float* p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = a.x + (size_t)min(row0 + r, a.N - 1) * a.ld;      // rows beyond the end read the last row, and are dropped below
    for (int c = lane; c < nchunk; c += 64) {
      const float4 cv = *reinterpret_cast<const float4*>(cen + 4 * c);
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r] = kc_chunk_dist(d[r], kc_chunk(p[r], c, a.D, a.vec), cv);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = wave_sum64(d[r]);
  }
  KcKey best{0.f, 0.f, -1, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + r;
    if (row >= a.N) break;                                   // (wave-uniform)
    float m = a.mind[row];
    if (c_idx >= 0) {
      const bool closer = d[r] < m;                          // a strictly smaller distance replaces: the first center that attains the minimum stays
      if (closer || d[r] != d[r]) {                          // (a NaN distance makes mind NaN and keeps assign)
        m = d[r];
        if (lane == 0) {
          a.mind[row] = m;
          if (closer) a.assign[row] = c_idx;
        }
      }
    }
    if (select) {
      const float w = a.weight ? a.weight[row] : 1.f;
      float score = has_center ? w * m : w;
      // the key of a draw proportional to w * mind: an exact zero stays zero (probability 0), a NaN stays NaN
      if (SAMPLE) score = __fdiv_rn(score, kc_exponential(rng, s, row));
      const KcKey k{score, w, row, m};
      if (a.taken[row] == 0 && w >= 0.f && score == score && kc_better(k, best)) best = k;
    }
  }
  if (!select) return;
  // ---- the workgroup's partial, the ticket, and in the workgroup that arrives last the pick
  if (lane == 0) {
    wkey[4 * wave] = best.score; wkey[4 * wave + 1] = best.w; wkey[4 * wave + 2] = __int_as_float(best.idx); wkey[4 * wave + 3] = best.mind;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < 4; ++v) {
      const KcKey k{wkey[4 * v], wkey[4 * v + 1], __float_as_int(wkey[4 * v + 2]), wkey[4 * v + 3]};
      if (kc_better(k, best)) best = k;
    }
    a.partial[blockIdx.x] = make_float4(best.score, best.w, __int_as_float(best.idx), best.mind);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ticket = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = ticket == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    wkey[16] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (wkey[16] == 0.f) return;                               // (workgroup-uniform)
  best = KcKey{0.f, 0.f, -1, 0.f};
  for (int g = tid; g < (int)gridDim.x; g += KC_THREADS) {
    const float4 v = a.partial[g];
    const KcKey k{v.x, v.y, __float_as_int(v.z), v.w};
    if (kc_better(k, best)) best = k;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const KcKey k{__shfl_xor(best.score, off), __shfl_xor(best.w, off), __shfl_xor(best.idx, off), __shfl_xor(best.mind, off)};
    if (kc_better(k, best)) best = k;
  }
  __syncthreads();                                           // (wkey[16] has been read by everyone)
  if (lane == 0) {
    wkey[4 * wave] = best.score; wkey[4 * wave + 1] = best.w; wkey[4 * wave + 2] = __int_as_float(best.idx); wkey[4 * wave + 3] = best.mind;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < 4; ++v) {
      const KcKey k{wkey[4 * v], wkey[4 * v + 1], __float_as_int(wkey[4 * v + 2]), wkey[4 * v + 3]};
      if (kc_better(k, best)) best = k;
    }
    const bool found = best.idx >= 0 && best.idx < a.N;
    a.picked[s] = found ? best.idx : -1;
    a.pick_dist[s] = found ? best.mind : -1.f;
    if (found) a.taken[best.idx] = 1;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace
