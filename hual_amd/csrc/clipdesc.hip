// hual_clip_mean_features (include/hual_seqpan.h): one descriptor per video of a resident feature bank - the mean over its frames of
// the raw features, optionally scaled to unit L2 norm - for the core-set selection of kcenter.hip.
//
// One workgroup per video.  Thread t owns the columns t, t + 256, ...: every frame is read as consecutive 1 KB segments (coalesced
// along vdim), the bank exactly once, and a column's frames are added in float32 in ascending frame order - a fixed order, so a second
// launch returns equal bits.  The norm is summed in float64 (per thread in ascending column order, then wave_sum64_f64 and the four
// waves in their order) and a zero row stays zero.  Bandwidth bound: nothing but the loads and one add per element.
#include "common.h"
#include "prof.h"

namespace {

constexpr int CD_THREADS = 256;

template <int NC>      // columns per thread
__global__ __launch_bounds__(CD_THREADS) void clip_mean_kernel(const float* __restrict__ bank, const int64_t* __restrict__ feat_off, int vdim,
                                                               int normalize, float* __restrict__ out, int ld_out) {
  __shared__ double wsum[CD_THREADS / 64];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = feat_off[v], f1 = feat_off[v + 1];
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t f = f0; f < f1; ++f) {
    const float* p = bank + (size_t)f * vdim;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int k = tid + CD_THREADS * j;
      if (k < vdim) acc[j] += p[k];
    }
  }
  const float T = (float)(f1 - f0);
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    acc[j] = f1 > f0 ? acc[j] / T : 0.f;                     // (a video without frames: a zero row)
    ss += (double)acc[j] * (double)acc[j];
  }
  float scale = 1.f;
  if (normalize) {                                           // (launch-uniform)
    ss = wave_sum64_f64(ss);
    if ((tid & 63) == 0) wsum[tid >> 6] = ss;
    __syncthreads();
    const double tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (tot > 0.0) scale = (float)(1.0 / sqrt(tot));         // a zero row stays zero (and a NaN row NaN: tot > 0 is false, acc is NaN)
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int k = tid + CD_THREADS * j;
    if (k < vdim) out[(size_t)v * ld_out + k] = acc[j] * scale;
  }
}

}  // namespace

extern "C" int hual_clip_mean_features(const float* feat_bank, const int64_t* feat_off, int V, int vdim, int normalize, float* out, int ld_out,
                                       void* stream) {
  HUAL_REQUIRE(feat_bank && feat_off && out, "hual_clip_mean_features: null pointer (feat_bank, feat_off, out)");
  HUAL_REQUIRE(V >= 1, "hual_clip_mean_features: V >= 1");
  HUAL_REQUIRE(vdim >= 1 && vdim <= 4096, "hual_clip_mean_features: 1 <= vdim <= 4096");
  HUAL_REQUIRE(ld_out >= vdim, "hual_clip_mean_features: ld_out >= vdim");
  hipStream_t st = (hipStream_t)stream;
  const int nc = hual::cdiv(vdim, CD_THREADS);
  const double bytes = 4.0 * vdim * V;                       // (the output; the bank's bytes depend on feat_off, which lives on the device)
#define CD_LAUNCH(NC) HUAL_LAUNCH(0.0, bytes, clip_mean_kernel<NC>, dim3(V), dim3(CD_THREADS), 0, st, feat_bank, feat_off, vdim, normalize, out, ld_out)
  if (nc <= 1) CD_LAUNCH(1);
  else if (nc <= 2) CD_LAUNCH(2);
  else if (nc <= 4) CD_LAUNCH(4);
  else if (nc <= 8) CD_LAUNCH(8);
  else CD_LAUNCH(16);
#undef CD_LAUNCH
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
