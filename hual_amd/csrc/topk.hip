// The k best spans of each clip with greedy temporal NMS (hual_span_topk, include/hual_seqpan.h): what R@k evaluation and the
// "best few moments" of a video need, on the device.  Beside the forward, not in it: heads.hip keeps its span argmax as it is.
//
// One 1024-thread workgroup per clip.  Thread t < 256 computes frame t's probabilities exactly as the span stage of heads_kernel does
// (spanprob.h, shared with spanconf.hip), so the numbers are bit for bit those of hual_span_argmax.  The triangle of up to 32,896
// candidates (i <= j < vlen, j - i < max_len) is cut into 1024 contiguous stretches of the row-major order, one
// per thread.  A thread keeps the best candidate of its stretch that no selected span suppresses; each of the k rounds is one
// (score, key) arg-reduction (wave64 butterfly, then the 16 waves through LDS), and after it only the threads whose best the new span
// suppresses rescan their stretch - the suppressed set only grows, so a best that survives stays best.
// Latency bound: at most 2 KB of logits in and 20 * k bytes out per clip, no matrix work; one barrier per round (ABI 9).
#include "common.h"
#include "prof.h"
#include "spanclip.h"

using namespace hual;

namespace {

constexpr int TK_THREADS = SPAN_THREADS;      // 16 waves: four per SIMD hide each other's LDS latency in the candidate scans
constexpr int TK_WAVES = SPAN_WAVES;
constexpr int TK_NONE = 0x7fffffff;      // key of "no candidate" (score -1: below every real score, which is >= 0)

// candidate order: higher score first, then the smaller key i * 256 + j (smaller i, then smaller j).  A NaN score is never better.
__device__ __forceinline__ bool tk_better(float s1, int k1, float s2, int k2) { return s1 > s2 || (s1 == s2 && k1 < k2); }

// greedy NMS test on the half-open intervals [i, j + 1): suppressed iff inter >= nms_iou * union, in fp32
__device__ __forceinline__ bool tk_suppresses(int key_a, int i, int j, float nms_iou) {
  const int ai = key_a >> 8, aj = key_a & 255;
  const int inter = max(0, min(aj, j) + 1 - max(ai, i));
  const int uni = (aj - ai + 1) + (j - i + 1) - inter;
  return (float)inter >= nms_iou * (float)uni;
}

// first flat index of row i of the candidate triangle: rows r < a = v - L hold L candidates, rows r >= a hold v - r
__device__ __forceinline__ int tk_row_off(int i, int v, int L) {
  const int a = max(0, v - L);
  int off = min(i, a) * L;
  if (i > a) {
    const int n = i - a;
    off += n * v - (n * (a + i - 1)) / 2;
  }
  return off;
}

// best candidate of the flat stretch [c0, c1) not suppressed by any of the nsel selected spans (sel: keys in LDS) nor by `extra` (a
// key, or TK_NONE)
__device__ __forceinline__ void tk_scan(int c0, int c1, int v, int L, const float* ps, const float* pe, const int* sel, int nsel, int extra,
                                        float nms_iou, float& bs, int& bk) {
  bs = -1.f; bk = TK_NONE;
  if (c0 >= c1) return;
  int i = tri_locate(c0, v, [=](int r) { return tk_row_off(r, v, L); });      // the row holding c0
  int j = i + (c0 - tk_row_off(i, v, L));
  int jend = min(v - 1, i + L - 1);
  float p = ps[i];
  for (int c = c0; c < c1; ++c) {
    const float s = p * pe[j];
    const int key = (i << 8) | j;
    if (tk_better(s, key, bs, bk)) {
      bool sup = extra != TK_NONE && tk_suppresses(extra, i, j, nms_iou);
      for (int q = 0; q < nsel && !sup; ++q) sup = tk_suppresses(sel[q], i, j, nms_iou);
      if (!sup) { bs = s; bk = key; }
    }
    if (++j > jend) { ++i; j = i; jend = min(v - 1, i + L - 1); p = ps[min(i, v - 1)]; }
  }
}

__global__ __launch_bounds__(TK_THREADS) void span_topk_kernel(const float* __restrict__ zs_, const float* __restrict__ ze_,
                                                                const int32_t* __restrict__ vlen_, int T, int k, int max_len,
                                                                float nms_iou, int64_t* __restrict__ start_index,
                                                                int64_t* __restrict__ end_index, float* __restrict__ score) {
  __shared__ float ps[256], pe[256];
  __shared__ float smf[2 * TK_WAVES];
  __shared__ double smd[2 * TK_WAVES];
  __shared__ float wbs[2][TK_WAVES];
  __shared__ int wbk[2][TK_WAVES];
  __shared__ int sel[SPAN_MAXK];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const SpanClip clip = open_span_clip(zs_, ze_, vlen_, T, ps, pe, smf, smd, [](int) {});
  const int v = clip.v;
  int nout = 0;
  if (clip.open) {
    // ---- candidates: this thread's stretch of the row-major triangle
    const int L = max_len > 0 ? min(max_len, v) : v;
    const int n = tk_row_off(v, v, L);
    const int c0 = t * n / TK_THREADS, c1 = (t + 1) * n / TK_THREADS;
    float bs; int bk;
    tk_scan(c0, c1, v, L, ps, pe, sel, 0, TK_NONE, nms_iou, bs, bk);
    for (int r = 0; r < k; ++r) {
      float rs = bs; int rk = bk;
      wave_best(rs, rk, tk_better);
      if (lane == 0) { wbs[r & 1][w] = rs; wbk[r & 1][w] = rk; }      // (double buffered: one barrier per round)
      __syncthreads();
      best_of_waves(wbs[r & 1], wbk[r & 1], TK_WAVES, rs, rk, tk_better);
      if (rk == TK_NONE) break;      // (uniform) fewer than k candidates survive
      if (t == 0) {
        sel[r] = rk;
        start_index[(size_t)b * k + r] = rk >> 8;
        end_index[(size_t)b * k + r] = rk & 255;
        score[(size_t)b * k + r] = rs;
      }
      nout = r + 1;
      // sel[0 .. r-1] were written before this round's barrier; the new span is in registers
      if (r + 1 < k && bk != TK_NONE && tk_suppresses(rk, bk >> 8, bk & 255, nms_iou))
        tk_scan(c0, c1, v, L, ps, pe, sel, r, rk, nms_iou, bs, bk);
    }
  }
  if (t >= nout && t < k) {      // padding: fewer candidates than k, an empty clip or a NaN logit
    start_index[(size_t)b * k + t] = -1;
    end_index[(size_t)b * k + t] = -1;
    score[(size_t)b * k + t] = -1.0f;
  }
}

}  // namespace

extern "C" int hual_span_topk(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T, int k,
                              int max_len, float nms_iou, int64_t* start_index, int64_t* end_index, float* score, void* stream) {
  HUAL_REQUIRE(start_logits && end_logits && video_seq_len && start_index && end_index && score, "hual_span_topk: null pointer");
  HUAL_REQUIRE(B >= 1, "hual_span_topk: B >= 1");
  HUAL_REQUIRE(T >= 1 && T <= 256, "hual_span_topk: 1 <= T <= 256");
  HUAL_REQUIRE(k >= 1 && k <= SPAN_MAXK, "hual_span_topk: 1 <= k <= 16");
  HUAL_REQUIRE(nms_iou > 0.f && nms_iou <= 1.f, "hual_span_topk: 0 < nms_iou <= 1");
  HUAL_REQUIRE(max_len >= 0, "hual_span_topk: max_len >= 0 (0: no limit)");
  const double bytes = 8.0 * B * T + 4.0 * B + 20.0 * B * k;
  HUAL_LAUNCH(0.0, bytes, span_topk_kernel, dim3(B), dim3(TK_THREADS), 0, (hipStream_t)stream, start_logits, end_logits, video_seq_len,
              T, k, max_len, nms_iou, start_index, end_index, score);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
