// One reading of the span posterior for the question to ask: the body hual_al_query (spanquery.hip) and every step of hual_al_session
// (spansession.hip) share, so that a session's step is the query's arithmetic instruction for instruction.  Given an opened row
// (spanpost.h: v, the hull, p_s / p_e in LDS) and the log2f rows of its probabilities: the segmented float64 sums, Z / Z_A / the entropy
// sum, the row's final status, q(t) and its gain per frame, and the first frame of maximal gain.  The derivation is at the top of
// spanquery.hip.
#pragma once
#include "spanpost.h"

namespace hual {

// the LDS of one step beside SpanRowLds
struct QueryStepLds {
  float ls[256], le[256];                   // log2f of p_s / p_e, written by the caller for t < v before the step
  double cum[5][256];                       // segmented: Ps | Ps of p log2 p | Pe | Pe of p log2 p;  [4]: the unsegmented Ps
  float bestv[SPAN_WAVES];
  int besti[SPAN_WAVES];
};

// what a step leaves: q / g in the thread of frame t (0 elsewhere and on a row that is not live), za / zf / hs / status uniform
struct QueryStep {
  float q, g;                               // q(t) and h2_bits(q(t)) of this thread's frame
  double zf, za, hs;                        // Z | Z_A | the entropy sum
  int status;                               // SpanRowStatus after posterior_status
};

// p log2f(p) in float64, 0 at p == 0 (where the logarithm is -inf)
__device__ __forceinline__ double p_log2(float p, float l) { return p > 0.f ? (double)p * (double)l : 0.0; }

// Called by the whole workgroup on a row that stage 1 left LIVE.  Starts on a barrier that publishes ls / le (and whatever else the caller
// wrote: an active-point list in LDS) and protects cum / bestv / besti against a previous step's readers; ends with bestv / besti written
// and a barrier behind them on a LIVE row: one thread then calls query_step_best.
__device__ __forceinline__ void query_step(const int32_t* aidx, const int8_t* apos, int napn, int v, const ApHull& hull, const float* ps,
                                           const float* pe, QueryStepLds& ql, double* smd, QueryStep& o) {
  const int t = threadIdx.x;
  const float *ls = ql.ls, *le = ql.le;
  double(*cum)[256] = ql.cum;
  const int npos = hull.npos, lo = hull.lo, hi = hull.hi, negL = hull.negL, negR = hull.negR;
  const bool inside = hull.inside;          // a negative inside the positive hull
  // frame c's segment [a, b]: between the nearest negatives around it; closed: c is itself a negative
  const int kind = t >> 8, c = t & 255;
  const ApSegment sg = ap_segment(aidx, apos, napn, v, c);
  const int sa = sg.sa, sb = sg.sb;
  const bool closed = sg.closed;
  o.q = 0.f; o.g = 0.f;
  __syncthreads();                          // ls / le are read across threads from here on
  if (c < v) {
    if (kind == 0) {
      double below = 0.0, seg = 0.0;
      for (int i = 0; i < sa; ++i) below += (double)ps[i];
      for (int i = sa; i <= c; ++i) seg += (double)ps[i];
      cum[4][c] = below + seg;              // (no negative below c: below == 0 and the sum is seg bit for bit)
      cum[0][c] = closed ? 0.0 : seg;
    } else if (kind == 1) {
      double seg = 0.0;
      for (int i = sa; i <= c; ++i) seg += p_log2(ps[i], ls[i]);
      cum[1][c] = closed ? 0.0 : seg;
    } else if (kind == 2) {
      double seg = 0.0;
      for (int i = c; i <= sb; ++i) seg += (double)pe[i];
      cum[2][c] = closed ? 0.0 : seg;
    } else {
      double seg = 0.0;
      for (int i = c; i <= sb; ++i) seg += p_log2(pe[i], le[i]);
      cum[3][c] = closed ? 0.0 : seg;
    }
  }
  __syncthreads();
  // Z over the whole triangle, and over the gaps' triangles Z_A and the entropy sum (a negative frame holds zeros): posterior_masses'
  // sums in its order, kept here because cum[] is read again below
  double zf = 0.0, za = 0.0, hs = 0.0;
  if (t < v) {
    const double e = (double)pe[t];
    zf = e * cum[4][t];
    za = e * cum[0][t];
    hs = e * cum[1][t] + p_log2(pe[t], le[t]) * cum[0][t];
  }
  block_reduce<BlockSumD, SPAN_WAVES>(zf, za, hs, smd);
  if (npos > 0) {                           // starts in (negL, lo] x ends in [hi, negR)
    const double S = cum[0][lo], E = cum[2][hi];
    za = inside ? 0.0 : S * E;
    hs = inside ? 0.0 : cum[1][lo] * E + S * cum[3][hi];
  }
  o.zf = zf; o.za = za; o.hs = hs;
  o.status = posterior_status(zf, za);
  if (o.status == SPAN_LIVE) {
    if (t < v) {
      double num;
      if (npos > 0) num = (t > negL && t < negR) ? cum[0][min(t, lo)] * cum[2][max(t, hi)] : 0.0;      // (on the hull: S * E, q == 1)
      else num = cum[0][t] * cum[2][t];
      o.q = (float)fmin(fmax(num / za, 0.0), 1.0);
      o.g = hual::h2_bits(o.q);
    }
    float best = t < v ? o.g : -1.0f;
    int bi = t < v ? t : 0x7fffffff;
    wave_best(best, bi);
    if ((t & 63) == 0) { ql.bestv[t >> 6] = best; ql.besti[t >> 6] = bi; }
    __syncthreads();
  }
}

// (one thread, after query_step on a LIVE row) the first frame of maximal gain, that gain, and the posterior's entropy in bits as the
// launches store it: clamped at >= 0, rounded to float32
__device__ __forceinline__ void query_step_best(const QueryStepLds& ql, const QueryStep& o, int& bi, float& best, float& entropy) {
  best_of_waves(ql.bestv, ql.besti, SPAN_WAVES, best, bi);
  const double h = log2(o.za) - o.hs / o.za;
  entropy = h > 0.0 ? (float)h : 0.f;
}

}  // namespace hual
