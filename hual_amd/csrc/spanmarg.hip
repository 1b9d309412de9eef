// hual_al_span_marginals (include/hual_seqpan.h): the start and end marginals of the span posterior given the answered active points -
// the soft labels the localizing loss can be trained on (assemble.hip blends them into y1 / y2).  The row - its
// status, probabilities (spanprob.h), set A and Z / Z_A - is opened by spanpost.h, as in every launch of the family; not in the train step.
//
// One 1024-thread workgroup per sample; the first quarter holds the start marginal (thread c: frame c), the second the end marginal.
// No walk over the triangle: the ends a start i can take within A form ONE interval - [hi, negR) for a start in (negL, lo] around a
// positive hull, [i, the end of i's gap] without a positive - and Z_A y_start[i] is p_s[i] times the sum of p_e over it; the starts of
// an end j alike.  Each sum is a serial walk of one thread over at most 256 LDS values in ascending order, float64, terms of one sign.
#include "prof.h"
#include "spanpost.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_span_marginals_kernel(AlMargArgs a) {
  __shared__ SpanRowLds lds;
  const int n = blockIdx.x, t = threadIdx.x;
  SpanRow r;
  open_posterior_row(a.in, n, lds, r);
  const int kind = t >> 8, c = t & 255;     // kind 0: y_start[c], kind 1: y_end[c]
  float y = 0.f;
  if (r.status == SPAN_LIVE && kind < 2 && c < r.v) {
    // the partners of frame c within A: the ends [lo, hi] of the start c (kind 0), the starts [lo, hi] of the end c (kind 1)
    const ApHull& hull = r.hull;
    int lo = 0, hi = -1;
    if (hull.npos > 0) {
      if (kind == 0) { if (c > hull.negL && c <= hull.lo) { lo = hull.hi; hi = min(hull.negR, r.v) - 1; } }
      else if (c >= hull.hi && c < hull.negR) { lo = hull.negL + 1; hi = hull.lo; }
    } else {
      const ApSegment sg = ap_segment(r.aidx, r.apos, r.napn, r.v, c);
      if (!sg.closed) { lo = kind == 0 ? c : sg.sa; hi = kind == 0 ? sg.sb : c; }
    }
    const float* other = kind == 0 ? lds.pe : lds.ps;
    double sum = 0.0;
    for (int i = lo; i <= hi; ++i) sum += (double)other[i];
    y = (float)(((double)(kind == 0 ? lds.ps : lds.pe)[c] * sum) / r.za);
  }
  // columns [0, T): a live row has T <= 256 and thread (kind, c) holds its value - 0 at c >= v; any other row is zeroed up to min(T, ld)
  if (r.status == SPAN_LIVE) {
    if (kind < 2 && c < r.T) (kind == 0 ? a.y_start : a.y_end)[r.row + c] = y;
  } else {
    for_each_column(r, a.in.set.ld, [&](int k) { a.y_start[r.row + k] = 0.f; a.y_end[r.row + k] = 0.f; });
  }
  if (t == 0) a.status[n] = r.status == SPAN_LIVE ? 1 : 0;
}

}  // namespace

namespace hual {

int launch_al_span_marginals(const AlMargArgs& a, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_span_marginals", [&] {
    HUAL_REQUIRE(a.y_start && a.y_end && a.status, "al_span_marginals: null output");
    return 0;
  });
  if (rc) return rc;
  // per frame: two logits in, two marginals out
  const hual_al_set& set = a.in.set;
  HUAL_LAUNCH(0.0, 16.0 * set.N * set.ld + 4.0 * set.N, al_span_marginals_kernel, dim3(set.N), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_span_marginals(const hual_al_set* set, const float* s0, const float* e0, float* y_start, float* y_end,
                                      int32_t* status, void* stream) {
  HUAL_REQUIRE(set, "hual_al_span_marginals: null set");
  AlMargArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0; a.y_start = y_start; a.y_end = y_end; a.status = status;
  return launch_al_span_marginals(a, (hipStream_t)stream);
}
