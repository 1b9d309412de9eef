// Hit probability of spans under the clip's own span distribution (hual_span_hit_prob, include/hual_seqpan.h): the chance
// P(IoU(span, truth) >= m) that a proposal of hual_span_topk counts as a hit at each of up to 4 exact rational IoU thresholds, the order
// of the proposals by one of them, and per threshold the span of the whole triangle that maximises it - the Bayes decision for R@1 at that
// threshold.  Beside topk.hip and spanconf.hip, not in the forward.
//
// One 1024-thread workgroup per clip, and with the Bayes spans one per (clip, threshold): blockIdx.y = m searches threshold m, and the
// workgroups with blockIdx.y = 0 also score the proposals.  No workgroup reads what another writes.  The probabilities are those of
// topk.hip (spanprob.h).  No pair of spans is enumerated: for a candidate (a, b) and a start i of the truth the ends j that hit form one
// interval [j_lo, j_hi] (the derivation is in front of sh_mass, spanmass.h), so a candidate's hit mass is sum_i p_s[i] * (E[j_hi + 1] - E[j_lo]) over
// the float64 prefix sums E of p_e in LDS - prefix DIFFERENCES, on purpose: their error is a few 2^-53 on values <= 1, far below the
// float32 result (hual_al_mbr_label avoids them; this kernel need not).  The two integer divisions of the interval ends depend on one
// length each and come from two tables of 257 entries per threshold, built once per workgroup; the starts i that hit at all are a range
// known in closed form, so the inner loops carry no test.  A proposal's mass is summed by one wave (lanes stride the starts, one butterfly);
// the Bayes search gives thread t the candidates t, t + 1024, .. ordered by length, then by end - the lanes of a wave hold neighbouring
// spans of one length, whose loops have the same trip counts (but for the clip's edge) and read the tables at one address and p_s / E at
// consecutive ones (row-major order, where a wave's trip counts differ, measured 10 % slower) - each summed by its thread in a fixed
// order, and ends on the family's (value, key) reduction (block.h).  No atomics, nothing grid wide: the result is a function of the inputs alone.
// Cost: 4.0 / 2.8 / 1.7 M multiply-adds per clip of 256 frames at 3/10, 1/2, 7/10, four LDS reads (24 bytes) each: the time is that of
// the longest clip's lowest threshold on its one CU, bound by the dependent LDS reads.
#include "common.h"
#include "prof.h"
#include "spanclip.h"
#include "spanmass.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void span_hit_prob_kernel(const float* __restrict__ zs_, const float* __restrict__ ze_,
                                                                     const int32_t* __restrict__ vlen_, int T, ShThresholds thr, int M, int k,
                                                                     int64_t* start_index, int64_t* end_index, float* score,
                                                                     float* __restrict__ hit_prob, int reorder_by,
                                                                     int64_t* __restrict__ best_start, int64_t* __restrict__ best_end,
                                                                     float* __restrict__ best_prob) {
  __shared__ float ps[256], pe[256];
  __shared__ double E[257];                                  // E[x] = sum of p_e[j], j < x
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  __shared__ int ce[SH_MAXM][257], fl[SH_MAXM][257];
  __shared__ SpanSlots slots;
  __shared__ float val[SPAN_MAXK][SH_MAXM];
  __shared__ double wbv[SPAN_WAVES];
  __shared__ int wbk[SPAN_WAVES];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const bool proposals = k > 0 && blockIdx.y == 0;           // (uniform)
  const SpanClip clip = open_span_clip(zs_, ze_, vlen_, T, ps, pe, smf, smd, [&](int v) {
    if (proposals) {
      load_slots(slots, b, k, v, start_index, end_index, score);
      if (t < k) for (int m = 0; m < M; ++m) val[t][m] = -1.0f;
    }
    sh_build_tables(thr.num, thr.den, M, ce, fl);
  });
  const int v = clip.v, *ca = slots.ca, *cb = slots.cb;
  bool live = false;
  double Z = 0.0;
  if (clip.open) {
    if (t <= v) {      // the prefix sums, each one serial sum in ascending order (all threads read the same p_e: a broadcast)
      double s = 0.0;
      for (int j = 0; j < t; ++j) s += (double)pe[j];
      E[t] = s;
    }
    __syncthreads();
    Z = t < v ? (double)ps[t] * (E[v] - E[t]) : 0.0;
    Z = block_reduce<BlockSumD, SPAN_WAVES>(Z, smd);
    live = span_mass_live(Z);      // (uniform)
  }
  // ---- the proposals: one wave per (slot, threshold) pair
  if (proposals) {
    if (live) {
      for (int p = w; p < k * M; p += SPAN_WAVES) {
        const int q = p / M, m = p - q * M;
        if (ca[q] < 0) continue;      // (uniform over the wave)
        double acc = sh_mass(ca[q], cb[q], v, ps, E, ce[m], fl[m], lane, 64);
        acc = wave_sum64_f64(acc);
        if (lane == 0) val[q][m] = (float)fmin(1.0, fmax(0.0, acc / Z));
      }
    }
    __syncthreads();
    if (t < k) {
      int pos = t;
      if (reorder_by >= 0 && live) {
        pos = slot_rank(k, t, [&](int q) { return val[q][reorder_by]; });
        store_slot(slots, t, b, k, pos, start_index, end_index, score);
      }
      for (int m = 0; m < M; ++m) hit_prob[((size_t)b * k + pos) * M + m] = val[t][m];
    }
  }
  // ---- the Bayes span of threshold blockIdx.y
  if (best_start) {
    const int m = blockIdx.y;
    double bv = -1.0; int bk = SH_NONE;
    if (live) {
      const int n = tri_row_off(v, v);
      for (int c = t; c < n; c += SPAN_THREADS) {      // by length, then by end: diagonal r holds the v - r spans of r + 1 frames
        int r, e;
        tri_entry(c, v, r, e);
        const int a = e - r, key = (a << 8) | e;
        const double mass = sh_mass(a, e, v, ps, E, ce[m], fl[m], 0, 1);
        if (FirstIndexMax()(mass, key, bv, bk)) { bv = mass; bk = key; }      // (the key a * 256 + b: first in row-major order)
      }
    }
    wave_best(bv, bk);
    if (lane == 0) { wbv[w] = bv; wbk[w] = bk; }
    __syncthreads();
    if (t == 0) {
      best_of_waves(wbv, wbk, SPAN_WAVES, bv, bk);
      const size_t o = (size_t)b * M + m;
      const bool found = bk != SH_NONE;      // (a live row has Z > 0, so some mass is positive)
      best_start[o] = found ? bk >> 8 : -1;
      best_end[o] = found ? bk & 255 : -1;
      best_prob[o] = found ? (float)fmin(1.0, fmax(0.0, bv / Z)) : -1.0f;
    }
  }
}

}  // namespace

extern "C" int hual_span_hit_prob(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T,
                                  const int32_t* thresholds, int M, int k, int64_t* start_index, int64_t* end_index, float* score,
                                  float* hit_prob, int reorder_by, int64_t* best_start, int64_t* best_end, float* best_prob, void* stream) {
  HUAL_REQUIRE(start_logits && end_logits && video_seq_len && thresholds, "hual_span_hit_prob: null pointer");
  HUAL_REQUIRE(B >= 1, "hual_span_hit_prob: B >= 1");
  HUAL_REQUIRE(T >= 1 && T <= 256, "hual_span_hit_prob: 1 <= T <= 256");
  HUAL_REQUIRE(k >= 0 && k <= SPAN_MAXK, "hual_span_hit_prob: 0 <= k <= 16");
  HUAL_REQUIRE(M >= 1 && M <= SH_MAXM, "hual_span_hit_prob: 1 <= M <= 4");
  ShThresholds thr = {};
  for (int m = 0; m < M; ++m) {
    thr.num[m] = thresholds[2 * m]; thr.den[m] = thresholds[2 * m + 1];
    HUAL_REQUIRE(thr.num[m] >= 1 && thr.num[m] <= thr.den[m] && thr.den[m] <= SH_MAXDEN,
                 "hual_span_hit_prob: thresholds are (num, den) with 1 <= num <= den <= 1024");
  }
  HUAL_REQUIRE(k == 0 || (start_index && end_index && hit_prob), "hual_span_hit_prob: null pointer (start_index, end_index, hit_prob with k >= 1)");
  const int nbest = (best_start ? 1 : 0) + (best_end ? 1 : 0) + (best_prob ? 1 : 0);
  HUAL_REQUIRE(nbest == 0 || nbest == 3, "hual_span_hit_prob: best_start, best_end, best_prob are given together or not at all");
  HUAL_REQUIRE(reorder_by >= -1 && reorder_by < M, "hual_span_hit_prob: -1 <= reorder_by < M");
  HUAL_REQUIRE(reorder_by < 0 || k >= 1, "hual_span_hit_prob: reorder_by needs k >= 1");
  HUAL_REQUIRE(k >= 1 || nbest == 3, "hual_span_hit_prob: nothing to do (k == 0 and no best_* outputs)");
  const double bytes = 8.0 * B * T + 4.0 * B + (reorder_by >= 0 ? 40.0 : 16.0) * B * k + 4.0 * B * k * M + (nbest ? 20.0 * B * M : 0.0);
  HUAL_LAUNCH(0.0, bytes, span_hit_prob_kernel, dim3(B, nbest ? M : 1), dim3(SPAN_THREADS), 0, (hipStream_t)stream, start_logits,
              end_logits, video_seq_len, T, thr, M, k, start_index, end_index, score, hit_prob, reorder_by, best_start, best_end, best_prob);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
