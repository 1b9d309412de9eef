// Expected temporal IoU of proposed spans under the clip's own span distribution, and that distribution's entropy
// (hual_span_expected_iou, include/hual_seqpan.h): a confidence in the evaluation's own metric for the proposals of hual_span_topk /
// hual_span_argmax, and their minimum-Bayes-risk order.  Beside topk.hip, not in the forward.
//
// One 1024-thread workgroup per clip.  The probabilities are those of topk.hip (spanprob.h); the triangle of up to 32,896 spans
// (i <= j < vlen) is cut into 1024 contiguous stretches of the row-major order, one per thread (at most 33 spans).  A thread walks its
// stretch once for Z and the entropy sum and once per valid candidate for the IoU-weighted sum, every sum in float64 in a fixed order;
// the k + 2 sums are reduced by one wave64 butterfly each and one pass over the 16 waves through LDS.  The stable sort of the k <= 16
// slots is a rank count, one slot per thread.  No atomics, nothing grid wide: the result is a function of the inputs alone.
// Latency bound: at most 2 KB of logits and 20 * k bytes of candidates in, a few hundred bytes out per clip.
#include "common.h"
#include "prof.h"
#include "spanclip.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void span_expected_iou_kernel(const float* __restrict__ zs_, const float* __restrict__ ze_,
                                                                         const int32_t* __restrict__ vlen_, int T, int k,
                                                                         int64_t* start_index, int64_t* end_index, float* score,
                                                                         float* __restrict__ expected_iou, float* __restrict__ span_entropy,
                                                                         int reorder) {
  __shared__ float ps[256], pe[256], ls[256], le[256];
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  __shared__ double red[SPAN_WAVES][SPAN_MAXK + 2];
  __shared__ double tot[SPAN_MAXK + 2];
  __shared__ SpanSlots slots;
  __shared__ float val[SPAN_MAXK];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t < k) val[t] = -1.0f;
  const SpanClip clip = open_span_clip(zs_, ze_, vlen_, T, ps, pe, smf, smd,
                                       [&](int v) { load_slots(slots, b, k, v, start_index, end_index, score); });
  const int v = clip.v, *ca = slots.ca, *cb = slots.cb;
  bool live = false;
  if (clip.open) {
    if (t < v) { ls[t] = log2f(ps[t]); le[t] = log2f(pe[t]); }
    __syncthreads();
    const int n = tri_row_off(v, v);
    const int c0 = t * n / SPAN_THREADS, c1 = (t + 1) * n / SPAN_THREADS;
    int i0 = 0, j0 = 0;
    if (c0 < c1) tri_entry(c0, v, i0, j0);
    // ---- Z and the entropy sum
    double z = 0.0, hs = 0.0;
    {
      int i = i0, j = j0;
      for (int c = c0; c < c1; ++c) {
        const float wt = ps[i] * pe[j];
        if (wt != 0.f) {      // (then both logarithms are finite)
          z += (double)wt;
          hs += (double)wt * (double)(ls[i] + le[j]);
        }
        if (++j >= v) { ++i; j = i; }
      }
    }
    z = wave_sum64_f64(z); hs = wave_sum64_f64(hs);
    if (lane == 0) { red[w][k] = z; red[w][k + 1] = hs; }
    // ---- the IoU-weighted sum of every valid candidate
    for (int q = 0; q < k; ++q) {
      const int a = ca[q], e = cb[q];
      if (a < 0) continue;      // (uniform)
      const int len = e - a + 1;
      double acc = 0.0;
      int i = i0, j = j0;
      for (int c = c0; c < c1; ++c) {
        const int inter = max(0, min(e, j) + 1 - max(a, i));
        const int uni = len + (j - i + 1) - inter;
        const float term = (ps[i] * pe[j]) * __fdiv_rn((float)inter, (float)uni);
        acc += (double)term;
        if (++j >= v) { ++i; j = i; }
      }
      acc = wave_sum64_f64(acc);
      if (lane == 0) red[w][q] = acc;
    }
    __syncthreads();
    if (t < k + 2 && (t >= k || ca[t] >= 0)) {
      double s = 0.0;
      for (int q = 0; q < SPAN_WAVES; ++q) s += red[q][t];
      tot[t] = s;
    }
    __syncthreads();
    const double Z = tot[k];
    live = span_mass_live(Z);      // (uniform)
    if (live) {
      if (t < k && ca[t] >= 0) val[t] = (float)(tot[t] / Z);
      if (t == 0 && span_entropy) {
        const double h = log2(Z) - tot[k + 1] / Z;
        span_entropy[b] = h > 0.0 ? (float)h : 0.f;
      }
    }
  }
  if (!live && t == 0 && span_entropy) span_entropy[b] = -1.0f;
  __syncthreads();
  if (t < k) {
    int pos = t;
    if (reorder && live) {
      pos = slot_rank(k, t, [&](int q) { return val[q]; });
      store_slot(slots, t, b, k, pos, start_index, end_index, score);
    }
    expected_iou[(size_t)b * k + pos] = val[t];
  }
}

}  // namespace

extern "C" int hual_span_expected_iou(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T, int k,
                                      int64_t* start_index, int64_t* end_index, float* score, float* expected_iou, float* span_entropy,
                                      int reorder, void* stream) {
  HUAL_REQUIRE(start_logits && end_logits && video_seq_len && start_index && end_index && expected_iou,
               "hual_span_expected_iou: null pointer");
  HUAL_REQUIRE(B >= 1, "hual_span_expected_iou: B >= 1");
  HUAL_REQUIRE(T >= 1 && T <= 256, "hual_span_expected_iou: 1 <= T <= 256");
  HUAL_REQUIRE(k >= 1 && k <= SPAN_MAXK, "hual_span_expected_iou: 1 <= k <= 16");
  const double bytes = 8.0 * B * T + 8.0 * B + (reorder ? 44.0 : 20.0) * B * k;
  HUAL_LAUNCH(0.0, bytes, span_expected_iou_kernel, dim3(B), dim3(SPAN_THREADS), 0, (hipStream_t)stream, start_logits, end_logits,
              video_seq_len, T, k, start_index, end_index, score, expected_iou, span_entropy, reorder);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
