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
#include "spanstep.h"

using namespace hual;

// (the body - segmented sums, Z / Z_A / the entropy sum, q, the arg-reduction - is spanstep.h's query_step, shared with hual_al_session)
__global__ __launch_bounds__(SPAN_THREADS) void al_query_kernel(AlQueryArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ QueryStepLds ql;
  const int n = blockIdx.x, t = threadIdx.x;
  SpanRow r;
  open_span_row(a.in, n, lds, r);
  const int v = r.v;
  QueryStep st;
  st.q = 0.f; st.g = 0.f;
  if (r.status == SPAN_LIVE) {
    if (t < v) { ql.ls[t] = log2f(lds.ps[t]); ql.le[t] = log2f(lds.pe[t]); }
    query_step(r.aidx, r.apos, r.napn, v, r.hull, lds.ps, lds.pe, ql, lds.smd, st);
    r.status = st.status;
    if (r.status == SPAN_LIVE && t == 0) {
      int bi;
      float best, h;
      query_step_best(ql, st, bi, best, h);
      a.query_point[n] = bi;
      a.query_gain[n] = best;
      a.post_entropy[n] = h;
      a.agree[n] = (float)(st.za / st.zf);
    }
  }
  if (r.status != SPAN_LIVE && t == 0) {
    a.query_point[n] = -1;
    a.query_gain[n] = -1.0f;
    a.post_entropy[n] = -1.0f;
    a.agree[n] = r.status == SPAN_CONTRADICTORY ? 0.f : -1.0f;
  }
  // columns [0, T): q and its gain below v on a live row (thread t holds frame t), 0 elsewhere
  const float q = st.q, g = st.g;
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
