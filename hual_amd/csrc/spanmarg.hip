// hual_al_span_marginals (include/hual_seqpan.h): the start and end marginals of the span posterior given the answered active points -
// the soft labels the localizing loss can be trained on (assemble.hip blends them into y1 / y2).  Beside al.hip's hual_al_query, whose
// set A (alpost.h), probabilities (spanprob.h) and Z / Z_A (spanmbr.h's posterior_masses) it shares; not in the train step.
//
// One 1024-thread workgroup per sample; the first quarter holds the start marginal (thread c: frame c), the second the end marginal.
// No walk over the triangle: the ends a start i can take within A form ONE interval - [hi, negR) for a start in (negL, lo] around a
// positive hull, [i, the end of i's gap] without a positive - and Z_A y_start[i] is p_s[i] times the sum of p_e over it; the starts of
// an end j alike.  Each sum is a serial walk of one thread over at most 256 LDS values in ascending order, float64, terms of one sign.
#include "al.h"
#include "prof.h"
#include "spanmbr.h"

using namespace hual;

namespace {

enum AlMargRow { AG_LIVE, AG_POISONED, AG_CONTRADICTORY };

__global__ __launch_bounds__(SPAN_THREADS) void al_span_marginals_kernel(AlMargArgs a) {
  __shared__ float ps[256], pe[256];
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  const int n = blockIdx.x, t = threadIdx.x;
  const int T = a.tlen[n];
  const size_t row = (size_t)n * a.ld;
  const bool fits = T >= 1 && T <= 256 && T <= a.ld;      // a longer row is poisoned, as in al_query_kernel
  const int v = fits ? span_clip_len(a.vlen[n], T) : 0;
  int status = (v == 0 || span_row_poisoned(a.s0, a.e0, row, v)) ? AG_POISONED : AG_LIVE;      // (uniform)
  const int kind = t >> 8, c = t & 255;     // kind 0: y_start[c], kind 1: y_end[c]
  float y = 0.f;
  if (status == AG_LIVE) {
    span_probabilities(a.s0, a.e0, row, T, v, ps, pe, smf, smd);
    const int ap0 = a.ap_off[n], napn = a.ap_off[n + 1] - ap0;
    const int32_t* aidx = a.ap_idx + ap0;
    const int8_t* apos = a.ap_pos + ap0;
    const ApHull hull = ap_hull(aidx, apos, napn, v);
    double zf, za;
    posterior_masses(aidx, apos, napn, v, hull, ps, pe, smd, zf, za);
    if (!(zf > 0.0 && zf < INFINITY)) status = AG_POISONED;
    else if (!(za > 0.0)) status = AG_CONTRADICTORY;
    if (status == AG_LIVE && kind < 2 && c < v) {
      // the partners of frame c within A: the ends [l, r] of the start c (kind 0), the starts [l, r] of the end c (kind 1)
      int l = 0, r = -1;
      if (hull.npos > 0) {
        if (kind == 0) { if (c > hull.negL && c <= hull.lo) { l = hull.hi; r = min(hull.negR, v) - 1; } }
        else if (c >= hull.hi && c < hull.negR) { l = hull.negL + 1; r = hull.lo; }
      } else {
        const ApSegment sg = ap_segment(aidx, apos, napn, v, c);
        if (!sg.closed) { l = kind == 0 ? c : sg.sa; r = kind == 0 ? sg.sb : c; }
      }
      const float* other = kind == 0 ? pe : ps;
      double sum = 0.0;
      for (int i = l; i <= r; ++i) sum += (double)other[i];
      y = (float)(((double)(kind == 0 ? ps : pe)[c] * sum) / za);
    }
  }
  // columns [0, T): a live row has T <= 256 and thread (kind, c) holds its value - 0 at c >= v; any other row is zeroed up to min(T, ld)
  if (status == AG_LIVE) {
    if (kind < 2 && c < T) (kind == 0 ? a.y_start : a.y_end)[row + c] = y;
  } else {
    const int Tw = min(max(T, 0), a.ld);
    for (int k = t; k < Tw; k += SPAN_THREADS) { a.y_start[row + k] = 0.f; a.y_end[row + k] = 0.f; }
  }
  if (t == 0) a.status[n] = status == AG_LIVE ? 1 : 0;
}

}  // namespace

namespace hual {

int launch_al_span_marginals(const AlMargArgs& a, hipStream_t s) {
  HUAL_REQUIRE(a.s0 && a.e0 && a.vlen && a.tlen && a.ap_off && a.ap_idx && a.ap_pos, "al_span_marginals: null input");
  HUAL_REQUIRE(a.y_start && a.y_end && a.status, "al_span_marginals: null output");
  HUAL_REQUIRE(a.N > 0 && a.ld >= 2 && a.ld <= HUAL_AL_MAX_T, "al_span_marginals: need N > 0 and 2 <= ld <= 1024");
  // per frame: two logits in, two marginals out
  HUAL_LAUNCH(0.0, 16.0 * a.N * a.ld + 4.0 * a.N, al_span_marginals_kernel, dim3(a.N), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_span_marginals(const hual_al_set* set, const float* s0, const float* e0, float* y_start, float* y_end,
                                      int32_t* status, void* stream) {
  HUAL_REQUIRE(set, "hual_al_span_marginals: null set");
  AlMargArgs a{};
  a.ld = set->ld; a.N = set->N; a.vlen = set->vlen; a.tlen = set->tlen;
  a.ap_off = set->ap_off; a.ap_idx = set->ap_idx; a.ap_pos = set->ap_pos;
  a.s0 = s0; a.e0 = e0; a.y_start = y_start; a.y_end = y_end; a.status = status;
  return launch_al_span_marginals(a, (hipStream_t)stream);
}
