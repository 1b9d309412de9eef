// train_op of /root/reference/models/ops.py:119-204: clip_by_global_norm(1.0) + AdamWeightDecayOptimizer
// (beta .9/.999, eps 1e-6, NO bias correction, decoupled weight decay 0.01 on every variable whose name does not
// contain LayerNorm|layer_norm|bias) as two launches over the flat parameter / gradient buffers.
#include "optim.h"
#include "prof.h"

using namespace hual;

// ema_count (optional): the update counter of the averaged weights, bumped HERE and only read by the adamw launch behind this one.
// Every block of that launch needs the same k, and blocks of one launch start at different times: a thread of the adamw launch that
// incremented the counter would race the blocks that have not read it yet.  This launch never reads the counter, the adamw launch never
// writes it, and the two are consecutive launches of one stream (consecutive nodes of one chain in a captured graph): all of this
// launch's writes are visible before the first block of the next one starts, and the previous step's adamw launch - the last reader of
// the old value - has finished before this one starts.  One thread, one plain vector store.
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, size_t n, float prescale, float* out, uint32_t* ema_count) {
  __shared__ float sm[4];
  if (ema_count && blockIdx.x == 0 && threadIdx.x == 0) ema_count[0] += 1u;
  float s = 0.f;
  const size_t n4 = n >> 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 v = ld4(g + 4 * i);
    v = make_float4(v.x * prescale, v.y * prescale, v.z * prescale, v.w * prescale);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  s = block_reduce<BlockSumF, 4, false>(s, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = s;     // per-block partial: no zeroing, no atomics
}

__global__ __launch_bounds__(256) void zero_kernel(float* p, size_t n) {
  const size_t n4 = n >> 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
    st4(p + 4 * i, f4zero());
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) p[4 * n4 + threadIdx.x] = 0.f;
}

// EMA: the averaged weights ride in this launch - s <- s + (1 - d_k) (p_new - s) while p_new is still in registers: one more 16-byte
// load and store per four elements, p is not read again.  k (1-based) comes from the device counter that the sqnorm launch in front
// of this one has already bumped (see there) - the arguments of a replayed step graph are frozen.  1 - d_k is formed directly:
// 1 - min(decay, (1 + k) / (10 + k)) = max(1 - decay, 9 / (10 + k)), one rounding.  EMA false is the kernel as it was.
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel_t(float* p, const float* g, float* m, float* v, const float* decay,
                                                      size_t n, const float* lr_dev, float clip_norm, float prescale,
                                                      const float* sqnorm, float b1, float b2, float eps, uint32_t* rng_state,
                                                      int64_t* cursor, const int64_t* spans, int64_t* bank, int span_words, int sel_inc,
                                                      int bank_inc, float* ema, const uint32_t* ema_count, float ema_decay,
                                                      int ema_warmup) {
  const float lr = lr_dev[0];
  float omd = 0.f;      // 1 - d_k
  if (EMA) {
    omd = 1.0f - ema_decay;
    if (ema_warmup) omd = fmaxf(omd, 9.0f / (10.0f + (float)ema_count[0]));
  }
  if (rng_state && blockIdx.x == 0 && threadIdx.x == 0) rng_state[2] += 1u;     // nothing in this launch reads it
  if (cursor && blockIdx.x == gridDim.x - 1) {      // the epoch loop's position: bank this step's spans, move on (one block: ordered by its barrier)
    const int64_t bp = cursor[1];
    for (int i = threadIdx.x; i < span_words; i += blockDim.x) bank[bp + i] = spans[i];
    __syncthreads();
    if (threadIdx.x == 0) { cursor[0] += sel_inc; cursor[1] = bp + bank_inc; }
  }
  float part = 0.f;
  for (int i = threadIdx.x & 63; i < HUAL_SQNORM_SLOTS; i += 64) part += sqnorm[i];     // same order in every wave
  const float gn = sqrtf(wave_sum64(part));
  const float sc = prescale * (clip_norm / fmaxf(gn, clip_norm));     // tf.clip_by_global_norm
  const size_t n4 = n >> 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 gg = ld4(g + 4 * i), mm = ld4(m + 4 * i), vv = ld4(v + 4 * i), pp = ld4(p + 4 * i), dd = ld4(decay + 4 * i);
    float* gp = &gg.x; float* mp = &mm.x; float* vp = &vv.x; float* ppp = &pp.x; const float* dp = &dd.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gp[k] * sc;
      const float nm = b1 * mp[k] + (1.0f - b1) * gr;
      const float nv = b2 * vp[k] + (1.0f - b2) * gr * gr;
      float upd = nm / (sqrtf(nv) + eps);          // ops.py:166-168
      upd += dp[k] * ppp[k];                       // ops.py:169-170 (decay[k] = 0 for excluded variables)
      ppp[k] = ppp[k] - lr * upd;
      mp[k] = nm;
      vp[k] = nv;
    }
    st4(p + 4 * i, pp);
    if (EMA) {
      float4 ss = ld4(ema + 4 * i);
      float* sp = &ss.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) sp[k] = sp[k] + omd * (ppp[k] - sp[k]);
      st4(ema + 4 * i, ss);
    }
    st4(m + 4 * i, mm);
    st4(v + 4 * i, vv);
  }
}

namespace hual {

int launch_adamw(const AdamArgs& a, hipStream_t s) {
  HUAL_REQUIRE(a.p && a.g && a.m && a.v && a.decay && a.lr_dev && a.sqnorm, "adamw: null pointer");
  HUAL_REQUIRE((a.n % 4) == 0, "adamw: flat size must be a multiple of 4");
  HUAL_REQUIRE(!a.cursor || (a.span_words == 0 || (a.spans && a.bank)), "adamw: loop cursor needs the span source and the bank");
  HUAL_REQUIRE((a.ema != nullptr) == (a.ema_count != nullptr), "adamw: ema and ema_count go together (both or neither)");
  HUAL_REQUIRE(a.ema_decay >= 0.f && a.ema_decay < 1.f, "adamw: ema_decay must lie in [0, 1)");
  HUAL_REQUIRE(!a.ema || (((uintptr_t)a.ema & 15) == 0 && a.ema != a.p), "adamw: ema must be 16-byte aligned and not the parameters");
  HUAL_LAUNCH(0.0, 4.0 * a.n, sqnorm_kernel, dim3(HUAL_SQNORM_SLOTS), dim3(256), 0, s, (const float*)a.g, a.n, a.prescale, a.sqnorm,
              a.ema_count);
  // one name for both instantiations: the launch is "adamw_kernel" to the profiler with and without the averaged weights
  auto adamw_kernel = a.ema ? adamw_kernel_t<true> : adamw_kernel_t<false>;
  HUAL_LAUNCH(0.0, (a.ema ? 40.0 : 32.0) * a.n, adamw_kernel, dim3(512), dim3(256), 0, s, a.p, (const float*)a.g, a.m, a.v, a.decay, a.n,
                     a.lr_dev, a.clip_norm, a.prescale, (const float*)a.sqnorm, 0.9f, 0.999f, 1e-6f, a.rng_state,
                     a.cursor, a.spans, a.bank, a.span_words, a.sel_inc, a.bank_inc, a.ema, (const uint32_t*)a.ema_count, a.ema_decay,
                     a.ema_warmup);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_zero(float* p, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  size_t g = (n / 4 + 255) / 256;
  g = g < 2048 ? (g > 0 ? g : 1) : 2048;
  HUAL_LAUNCH(0.0, 4.0 * n, zero_kernel, dim3((unsigned)g), dim3(256), 0, s, p, n);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual
