// hual_al_query (include/hual_seqpan.h): the frame whose answer says most about the span.  The annotator's answer at frame t is a
// function of the true span, so its mutual information with the span is the entropy h2(q(t)) of the answer, q(t) the posterior
// probability that t lies inside the span: the span distribution P(i,j) ~ p_s[i] p_e[j] (spanprob.h: the numbers of hual_span_argmax)
// restricted to the set A of spans the answered active points allow.  One 1024-thread workgroup per sample, as the other span kernels;
// the row - its status, probabilities and set A - is opened by spanpost.h, as in every launch of the family; not in the train step.
//
// No walk over the triangle: i <= t <= j implies i <= j, and A is a product of a start range and an end range (with a positive point:
// (negL, lo] x [hi, negR)) or a union of triangles, one per gap between negatives (without one).  Both are read from SEGMENTED sums -
// a negative frame closes a segment -: Ps(t) = sum of p_s over the segment's frames <= t, Pe(t) = sum of p_e over its frames >= t, and
// the same two of p log2f p.  Then q(t) Z_A = Ps(min(t, lo)) Pe(max(t, hi)) resp. Ps(t) Pe(t), Z_A = Ps(lo) Pe(hi) resp. the sum over j of
// p_e[j] Ps(j), and the entropy sum factors alike.  Every sum adds terms of one sign in float64 (no difference of prefix sums: a gap
// that holds 1e-10 of the mass keeps its digits).  The four segmented sums and the unsegmented one behind Z are each a serial walk of one
// thread per frame, the four kinds on the four quarters of the workgroup: at most 256 LDS reads and additions per thread, fixed order,
// the segment's ends known before the walk (from the active-point list), so the reads are not chained to a flag read on every step.
#include "prof.h"
#include "spanpost.h"

using namespace hual;

namespace {

// p log2f(p) in float64, 0 at p == 0 (where the logarithm is -inf)
__device__ __forceinline__ double p_log2(float p, float l) { return p > 0.f ? (double)p * (double)l : 0.0; }

}  // namespace

__global__ __launch_bounds__(SPAN_THREADS) void al_query_kernel(AlQueryArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ float ls[256], le[256];
  __shared__ double cum[5][256];            // segmented: Ps | Ps of p log2 p | Pe | Pe of p log2 p;  [4]: the unsegmented Ps
  __shared__ float bestv[SPAN_WAVES];
  __shared__ int besti[SPAN_WAVES];
  const int n = blockIdx.x, t = threadIdx.x;
  SpanRow r;
  open_span_row(a.in, n, lds, r);
  const float *ps = lds.ps, *pe = lds.pe;
  const int v = r.v;
  float q = 0.f, g = 0.f;
  if (r.status == SPAN_LIVE) {
    if (t < v) { ls[t] = log2f(ps[t]); le[t] = log2f(pe[t]); }
    const int npos = r.hull.npos, lo = r.hull.lo, hi = r.hull.hi, negL = r.hull.negL, negR = r.hull.negR;
    const bool inside = r.hull.inside;      // a negative inside the positive hull
    // frame c's segment [a, b]: between the nearest negatives around it; closed: c is itself a negative
    const int kind = t >> 8, c = t & 255;
    const ApSegment sg = ap_segment(r.aidx, r.apos, r.napn, v, c);
    const int sa = sg.sa, sb = sg.sb;
    const bool closed = sg.closed;
    __syncthreads();                        // ls / le are read across threads from here on
    if (c < v) {
      if (kind == 0) {
        double below = 0.0, seg = 0.0;
        for (int i = 0; i < sa; ++i) below += (double)ps[i];
        for (int i = sa; i <= c; ++i) seg += (double)ps[i];
        cum[4][c] = below + seg;            // (no negative below c: below == 0 and the sum is seg bit for bit)
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
    block_reduce<BlockSumD, SPAN_WAVES>(zf, za, hs, lds.smd);
    if (npos > 0) {                         // starts in (negL, lo] x ends in [hi, negR)
      const double S = cum[0][lo], E = cum[2][hi];
      za = inside ? 0.0 : S * E;
      hs = inside ? 0.0 : cum[1][lo] * E + S * cum[3][hi];
    }
    r.status = posterior_status(zf, za);
    if (r.status == SPAN_LIVE) {
      if (t < v) {
        double num;
        if (npos > 0) num = (t > negL && t < negR) ? cum[0][min(t, lo)] * cum[2][max(t, hi)] : 0.0;      // (on the hull: S * E, q == 1)
        else num = cum[0][t] * cum[2][t];
        q = (float)fmin(fmax(num / za, 0.0), 1.0);
        g = h2_bits(q);
      }
      float best = t < v ? g : -1.0f;
      int bi = t < v ? t : 0x7fffffff;
      wave_best(best, bi);
      if ((t & 63) == 0) { bestv[t >> 6] = best; besti[t >> 6] = bi; }
      __syncthreads();
      if (t == 0) {
        best_of_waves(bestv, besti, SPAN_WAVES, best, bi);
        const double h = log2(za) - hs / za;
        a.query_point[n] = bi;
        a.query_gain[n] = best;
        a.post_entropy[n] = h > 0.0 ? (float)h : 0.f;
        a.agree[n] = (float)(za / zf);
      }
    }
  }
  if (r.status != SPAN_LIVE && t == 0) {
    a.query_point[n] = -1;
    a.query_gain[n] = -1.0f;
    a.post_entropy[n] = -1.0f;
    a.agree[n] = r.status == SPAN_CONTRADICTORY ? 0.f : -1.0f;
  }
  // columns [0, T): q and its gain below v on a live row (thread t holds frame t), 0 elsewhere
  for_each_column(r, a.in.set.ld, [&](int c) {
    const bool on = r.status == SPAN_LIVE && c < v;
    if (a.incl) a.incl[r.row + c] = on ? q : 0.f;
    if (a.gain) a.gain[r.row + c] = on ? g : 0.f;
  });
}

namespace hual {

int launch_al_query(const AlQueryArgs& a, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_query", [&] {
    HUAL_REQUIRE(a.query_point && a.query_gain && a.post_entropy && a.agree, "al_query: null output");
    return 0;
  });
  if (rc) return rc;
  const hual_al_set& set = a.in.set;
  // per frame: two logits in, q and its gain out
  HUAL_LAUNCH(0.0, (8.0 + (a.incl ? 4.0 : 0.0) + (a.gain ? 4.0 : 0.0)) * set.N * set.ld + 28.0 * set.N, al_query_kernel, dim3(set.N),
              dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_query(const hual_al_set* set, const float* s0, const float* e0, float* incl, float* gain, int32_t* query_point,
                             float* query_gain, float* post_entropy, float* agree, void* stream) {
  HUAL_REQUIRE(set, "hual_al_query: null set");
  AlQueryArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0; a.incl = incl; a.gain = gain;
  a.query_point = query_point; a.query_gain = query_gain; a.post_entropy = post_entropy; a.agree = agree;
  return launch_al_query(a, (hipStream_t)stream);
}
