// Coverage of span sets under the clip's own span distribution (hual_span_hit_cover, include/hual_seqpan.h): the chance that at least one
// span of a set hits the truth at IoU >= m - what R@k counts - for the cumulative sets of k proposals, and per threshold the greedy set of
// K spans of the whole triangle that covers the most: each step takes the span whose hits add the most mass no earlier pick hits.  The
// coverage is monotone and submodular, so the greedy set is within 1 - (1 - 1/K)^K of the best set of K spans; its step 0 is the Bayes
// span for R@1 of spanhit.hip.  Beside topk.hip, spanconf.hip and spanhit.hip, not in the forward.
//
// One 1024-thread workgroup per (clip, threshold): blockIdx.y = m.  No workgroup reads what another writes.  Probabilities, prefix sums
// E, division tables and the interval of hitting ends per start are those of spanhit.hip (spanmass.h): for a span c and a start i of the
// truth the ends that hit c are ONE interval, so the truths already covered at start i are a union of at most 16 intervals of ends.
// LDS keeps that union per start as a list of disjoint, non-adjacent intervals (two bytes each, entry q of start i at [q][i]: the lanes
// of a wave read neighbouring starts, one bank each); after a pick thread i merges the pick's interval of start i into its list.  The
// gain of a candidate is sum_i p_s[i] * ((E[j_hi + 1] - E[j_lo]) - sum over the list of the overlap's E-difference), a start's term
// clamped at >= 0 against the rounding of the differences; with empty lists, step 0, it is sh_mass, and step 0 calls sh_mass itself, so
// its span and probability are hual_span_hit_prob's bit for bit.  Candidates go to the threads as in the Bayes search - by length, then
// by end - and every step ends on the family's (value, key) reduction.  The proposals use the same lists: thread i holds start i's
// uncovered mass of the slot, a block sum in a fixed order gives the slot's gain, then the merge.  Float64 throughout, no atomics,
// nothing grid wide: the result is a function of the inputs alone.
// Gains only fall from step to step (the coverage is submodular), so a candidate's gain of an earlier step bounds its gain now: dynamic
// LDS keeps one float per candidate, its last computed gain rounded UP (sc_bound).  A step first has every thread compute the gain of
// its candidate of largest bound; the largest of those gains, L, is reached by some candidate, so a candidate whose bound lies below L
// is neither the maximum nor tied with it and is skipped, and the pick is the one a full evaluation takes.
// Cost: a candidate evaluated at step s costs its share of the Bayes search of spanhit.hip times (1 + the list length of the starts it
// walks), <= 1 + s; how many are evaluated depends on the distribution.
#include "common.h"
#include "prof.h"
#include "spanclip.h"
#include "spanmass.h"

using namespace hual;

namespace {

// the covered ends per start: n[i] disjoint intervals iv[q][i] = lo | hi << 8, q < n[i], no two of them adjacent, in no particular order
struct CoverLists {
  unsigned short iv[SPAN_MAXK][256];
  unsigned char n[256];
};

// the mass of the ends [jlo, jhi] of start i that no interval of its list holds, over p_s[i]
__device__ __forceinline__ double sc_open_ends(const CoverLists& L, const double* E, int i, int jlo, int jhi) {
  double r = E[jhi + 1] - E[jlo];
  const int n = L.n[i];
  for (int q = 0; q < n; ++q) {
    const int x = L.iv[q][i], lo = max(jlo, x & 255), hi = min(jhi, x >> 8);
    if (lo <= hi) r -= E[hi + 1] - E[lo];
  }
  return fmax(r, 0.0);
}

// sh_mass over the ends not yet covered: this thread's share of the gain of (a, b), the starts in sh_mass's order
__device__ __forceinline__ double sc_gain(const CoverLists& L, int a, int b, int v, const float* ps, const double* E, const int* ce,
                                          const int* fl, int first, int step) {
  const int n = b + 1 - a, F = fl[n], C = ce[n];
  const int imin = max(0, b + 1 - F), imax = b + 1 - C;
  double acc = 0.0;
  for (int i = a - first; i >= imin; i -= step)
    acc += (double)ps[i] * sc_open_ends(L, E, i, a - 1 + ce[b + 1 - i], min(v - 1, i - 1 + F));
  for (int i = a + step - first; i <= imax; i += step)
    acc += (double)ps[i] * sc_open_ends(L, E, i, i - 1 + C, min(v - 1, a - 1 + fl[b + 1 - i]));
  return acc;
}

// an upper bound of every later gain of a candidate whose gain is g now, as a float: g plus 1e-12 - the computed gains fall only up to
// their rounding, a few 2^-53 per covered interval on values that sum to <= 1 - rounded up
__device__ __forceinline__ float sc_bound(double g) {
  const double x = g + 1e-12;
  const float u = (float)x;
  return (double)u < x ? __uint_as_float(__float_as_uint(u) + 1u) : u;      // (x > 0: the next float above u)
}

// thread i < v: the interval of start i that (a, b) hits, if any, joins the list - with every interval it overlaps or touches, as one.
// At most one interval more than before: 16 merges fit SPAN_MAXK entries.
__device__ __forceinline__ void sc_merge(CoverLists& L, int a, int b, int v, int i, const int* ce, const int* fl) {
  int lo, hi;
  if (!sh_interval(a, b, v, i, ce, fl, lo, hi)) return;
  int kept = L.n[i];
  // an entry kept before the interval grew may touch the grown one: fold until none does (<= 16 entries, rarely a third pass)
  for (bool again = true; again;) {
    again = false;
    int m = 0;
    for (int q = 0; q < kept; ++q) {
      const int x = L.iv[q][i], xl = x & 255, xh = x >> 8;
      if (xl <= hi + 1 && lo <= xh + 1) { lo = min(lo, xl); hi = max(hi, xh); again = true; }
      else L.iv[m++][i] = (unsigned short)x;
    }
    kept = m;
  }
  if (kept < SPAN_MAXK) {      // (always: see above; the bound keeps a broken invariant inside the array)
    L.iv[kept][i] = (unsigned short)(lo | (hi << 8));
    L.n[i] = (unsigned char)(kept + 1);
  }
}

__global__ __launch_bounds__(SPAN_THREADS) void span_hit_cover_kernel(const float* __restrict__ zs_, const float* __restrict__ ze_,
                                                                      const int32_t* __restrict__ vlen_, int T, ShThresholds thr, int M, int k,
                                                                      const int64_t* __restrict__ start_index,
                                                                      const int64_t* __restrict__ end_index, float* __restrict__ set_prob,
                                                                      int K, float min_gain, int64_t* __restrict__ cover_start,
                                                                      int64_t* __restrict__ cover_end, float* __restrict__ cover_prob) {
  __shared__ float ps[256], pe[256];
  __shared__ double E[257];                                  // E[x] = sum of p_e[j], j < x
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  __shared__ int ce[1][257], fl[1][257];                     // of threshold blockIdx.y
  __shared__ SpanSlots slots;
  __shared__ CoverLists L;
  __shared__ double wbv[SPAN_WAVES];
  __shared__ int wbk[SPAN_WAVES];
  __shared__ double pickv;
  __shared__ int pickk;
  extern __shared__ float ub[];                              // K >= 2: per candidate (flat, by length then end) the bound of its gain
  const int b = blockIdx.x, m = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const SpanClip clip = open_span_clip(zs_, ze_, vlen_, T, ps, pe, smf, smd, [&](int v) {
    if (k > 0) load_slots(slots, b, k, v, start_index, end_index, nullptr);
    sh_build_tables(thr.num + m, thr.den + m, 1, ce, fl);
    if (t < 256) L.n[t] = 0;
  });
  const int v = clip.v, *ca = slots.ca, *cb = slots.cb;
  bool live = false;
  double Z = 0.0;
  if (clip.open) {
    if (t <= v) {      // the prefix sums and Z of spanhit.hip, in its order
      double s = 0.0;
      for (int j = 0; j < t; ++j) s += (double)pe[j];
      E[t] = s;
    }
    __syncthreads();
    Z = t < v ? (double)ps[t] * (E[v] - E[t]) : 0.0;
    Z = block_reduce<BlockSumD, SPAN_WAVES>(Z, smd);
    live = span_mass_live(Z);      // (uniform)
  }
  if (!live) {
    for (int q = t; q < k; q += SPAN_THREADS) set_prob[((size_t)b * k + q) * M + m] = -1.0f;
    for (int s = t; s < K; s += SPAN_THREADS) {
      const size_t o = ((size_t)b * M + m) * K + s;
      cover_start[o] = -1; cover_end[o] = -1; cover_prob[o] = -1.0f;
    }
    return;
  }
  // ---- the proposals: slot after slot, the coverage of the valid slots so far
  if (k > 0) {
    double covered = 0.0;
    for (int q = 0; q < k; ++q) {
      if (ca[q] >= 0) {      // (uniform)
        int jlo, jhi;
        double g = 0.0;
        if (t < v && sh_interval(ca[q], cb[q], v, t, ce[0], fl[0], jlo, jhi)) g = (double)ps[t] * sc_open_ends(L, E, t, jlo, jhi);
        covered += block_reduce<BlockSumD, SPAN_WAVES>(g, smd);
        if (t < v) sc_merge(L, ca[q], cb[q], v, t, ce[0], fl[0]);      // (thread t alone reads and writes start t's list)
      }
      if (t == 0) set_prob[((size_t)b * k + q) * M + m] = (float)fmin(1.0, fmax(0.0, covered / Z));
    }
    __syncthreads();
    if (t < 256) L.n[t] = 0;      // the greedy set starts with nothing covered
    __syncthreads();
  }
  // ---- the greedy set of threshold m
  double covered = 0.0;
  bool stopped = false;
  float last = 0.0f;
  const int n = tri_row_off(v, v);
  int topc = -1;      // this thread's candidate of largest bound
  for (int s = 0; s < K; ++s) {
    const size_t o = ((size_t)b * M + m) * K + s;
    if (stopped) {      // (uniform)
      if (t == 0) { cover_start[o] = -1; cover_end[o] = -1; cover_prob[o] = last; }
      continue;
    }
    double reached = -1.0;      // (uniform) a gain some candidate reaches at this step
    if (s > 0) {
      if (topc >= 0) {
        int r, e;
        tri_entry(topc, v, r, e);
        reached = sc_gain(L, e - r, e, v, ps, E, ce[0], fl[0], 0, 1);
      }
      reached = block_reduce<BlockMaxD, SPAN_WAVES>(reached, smd);
    }
    double bv = -1.0; int bk = SH_NONE;
    float topu = -1.0f;
    topc = -1;
    for (int c = t; c < n; c += SPAN_THREADS) {      // by length, then by end: the candidate order of spanhit.hip
      float u = s > 0 ? ub[c] : 0.0f;
      if (s == 0 || (double)u >= reached) {
        int r, e;
        tri_entry(c, v, r, e);
        const int a = e - r, key = (a << 8) | e;
        const double mass = s == 0 ? sh_mass(a, e, v, ps, E, ce[0], fl[0], 0, 1) : sc_gain(L, a, e, v, ps, E, ce[0], fl[0], 0, 1);
        if (FirstIndexMax()(mass, key, bv, bk)) { bv = mass; bk = key; }
        if (K > 1) { u = sc_bound(mass); ub[c] = u; }      // (thread t alone reads and writes its candidates' bounds)
      }
      if (u > topu) { topu = u; topc = c; }
    }
    wave_best(bv, bk);
    if (lane == 0) { wbv[w] = bv; wbk[w] = bk; }
    __syncthreads();
    if (t == 0) {
      best_of_waves(wbv, wbk, SPAN_WAVES, bv, bk);
      pickv = bv; pickk = bk;
    }
    __syncthreads();
    bv = pickv; bk = pickk;      // (uniform from here on)
    if (bk == SH_NONE || bv / Z <= (double)min_gain) {
      stopped = true;
      if (t == 0) { cover_start[o] = -1; cover_end[o] = -1; cover_prob[o] = last; }
      continue;
    }
    covered += bv;
    last = (float)fmin(1.0, fmax(0.0, covered / Z));
    const int a = bk >> 8, e = bk & 255;
    if (t == 0) { cover_start[o] = a; cover_end[o] = e; cover_prob[o] = last; }
    if (s + 1 < K) {
      if (t < v) sc_merge(L, a, e, v, t, ce[0], fl[0]);
      __syncthreads();      // the lists are read by every thread in the next step
    }
  }
}

}  // namespace

extern "C" int hual_span_hit_cover(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T,
                                   const int32_t* thresholds, int M, int k, const int64_t* start_index, const int64_t* end_index,
                                   float* set_prob, int K, float min_gain, int64_t* cover_start, int64_t* cover_end, float* cover_prob,
                                   void* stream) {
  HUAL_REQUIRE(start_logits && end_logits && video_seq_len && thresholds, "hual_span_hit_cover: null pointer");
  HUAL_REQUIRE(B >= 1, "hual_span_hit_cover: B >= 1");
  HUAL_REQUIRE(T >= 1 && T <= 256, "hual_span_hit_cover: 1 <= T <= 256");
  HUAL_REQUIRE(k >= 0 && k <= SPAN_MAXK, "hual_span_hit_cover: 0 <= k <= 16");
  HUAL_REQUIRE(K >= 0 && K <= SPAN_MAXK, "hual_span_hit_cover: 0 <= K <= 16");
  HUAL_REQUIRE(M >= 1 && M <= SH_MAXM, "hual_span_hit_cover: 1 <= M <= 4");
  ShThresholds thr = {};
  for (int m = 0; m < M; ++m) {
    thr.num[m] = thresholds[2 * m]; thr.den[m] = thresholds[2 * m + 1];
    HUAL_REQUIRE(thr.num[m] >= 1 && thr.num[m] <= thr.den[m] && thr.den[m] <= SH_MAXDEN,
                 "hual_span_hit_cover: thresholds are (num, den) with 1 <= num <= den <= 1024");
  }
  HUAL_REQUIRE(k >= 1 || K >= 1, "hual_span_hit_cover: nothing to do (k == 0 and K == 0)");
  HUAL_REQUIRE(min_gain >= 0.0f && min_gain < 1.0f, "hual_span_hit_cover: 0 <= min_gain < 1");      // (a NaN fails both)
  HUAL_REQUIRE(k == 0 || (start_index && end_index && set_prob), "hual_span_hit_cover: null pointer (start_index, end_index, set_prob with k >= 1)");
  const int ncover = (cover_start ? 1 : 0) + (cover_end ? 1 : 0) + (cover_prob ? 1 : 0);
  HUAL_REQUIRE(ncover == 0 || ncover == 3, "hual_span_hit_cover: cover_start, cover_end, cover_prob are given together or not at all");
  HUAL_REQUIRE(K == 0 || ncover == 3, "hual_span_hit_cover: null pointer (cover_start, cover_end, cover_prob with K >= 1)");
  const int lds = K > 1 ? (4 * (T * (T + 1) / 2) + 15) & ~15 : 0;
  HUAL_DYN_LDS(span_hit_cover_kernel, 4 * (256 * 257 / 2));
  const double bytes = 8.0 * B * T + 4.0 * B + 16.0 * B * k + 4.0 * B * k * M + 20.0 * B * M * K;
  HUAL_LAUNCH(0.0, bytes, span_hit_cover_kernel, dim3(B, M), dim3(SPAN_THREADS), lds, (hipStream_t)stream, start_logits, end_logits,
              video_seq_len, T, thr, M, k, start_index, end_index, set_prob, K, min_gain, cover_start, cover_end, cover_prob);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
