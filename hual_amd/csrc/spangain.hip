// hual_al_label_gain (include/hual_seqpan.h): per frame t, the temporal IoU the pseudo-label of hual_al_mbr_label is expected to gain
// from the annotator's answer at t - one-step lookahead under the span posterior given the answered active points, in the evaluation's
// own metric.  The row - its status, probabilities (spanprob.h), set A and Z / Z_A - is opened by spanpost.h, as in every launch
// of the family; the maximisation (spanmbr.h) is spanlabel.hip's; not in the train step.
//
// One 1024-thread workgroup per selected sample.  V0, the value of today's label, is the maximum of label_region over the regions of A,
// as in al_mbr_label_kernel.  Then a uniform loop over the candidate frames: the answer "inside" leaves one region around the hull
// grown by t; the answer "outside" beside a positive hull moves the nearest negative on t's side, and without a positive splits the gap
// that holds t in two - the other gaps keep the maxima the V0 pass found (the best and the second best with the best one's gap: a
// maximum is exact).  Every branch maximises R / Z_A with the PARENT's Z_A, so the gain is M+ + M- - V0 without a further division.  A
// branch without mass has no positive R (a span of positive weight overlaps itself), which is how a determined answer is recognised.
// The arithmetic is label_region's: float64 sums of one sign in a fixed order, maxima, no atomics, nothing grid wide.
#include "prof.h"
#include "spanmbr.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_label_gain_kernel(AlGainArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[256], xg[256];       // label_region's p_s[l] H_e[l] | p_s[l] G_e[l]
  __shared__ float gs[256];                 // the gain of the evaluated frames, 0 elsewhere
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  if (t < 256) gs[t] = 0.f;
  if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;      // (the opening's barriers publish both)
  SpanRow r;
  open_posterior_row(a.in, n, lds, r);
  if (r.status == SPAN_LIVE) {
    const float *ps = lds.ps, *pe = lds.pe;
    double* smd = lds.smd;
    const ApHull& hull = r.hull;
    const int v = r.v, napn = r.napn;
    const int32_t* aidx = r.aidx;
    const int8_t* apos = r.apos;
    const double za = r.za;
    double v0 = -1.0, askg = -1.0;          // (uniform: every thread holds the reductions' results)
    int askt = -1;
    int bi;                                 // (the label itself is hual_al_mbr_label's to report)
    // V0 over the regions of A; without a positive also the second-best gap's maximum and the best one's first frame
    double second = -1.0;
    int topgap = -1;
    if (hull.npos > 0) {
      label_region(hull.negL + 1, hull.lo, hull.hi, min(hull.negR, v) - 1, ps, pe, inv, xh, xg, za, v0, bi);
      v0 = block_reduce<BlockMaxD, SPAN_WAVES>(v0, smd);
    } else {
      for_each_gap(r, [&](int first, int last) {
        double gv = -1.0;
        label_region(first, last, first, last, ps, pe, inv, xh, xg, za, gv, bi);
        gv = block_reduce<BlockMaxD, SPAN_WAVES>(gv, smd);
        if (gv > v0) { second = v0; v0 = gv; topgap = first; }
        else if (gv > second) second = gv;
      });
    }
    const int count = a.cand ? a.M : v;
    for (int k = 0; k < count; ++k) {       // the candidate frames (uniform)
      const int f = a.cand ? a.cand[(size_t)n * a.M + k] : k;
      if (f < 0 || f >= v) continue;
      const ApHull hp = ap_hull(aidx, apos, napn, v, f, 1);      // A after "inside": (negL', lo'] x [hi', negR')
      const ApHull hn = ap_hull(aidx, apos, napn, v, f, 0);      // A after "outside", beside a positive hull
      double g = 0.0;
      if (!hp.inside && !(hull.npos > 0 && hn.inside)) {         // neither answer is ruled out by the points alone
        double mp = -1.0, mn = -1.0, rest = -1.0;
        label_region(hp.negL + 1, hp.lo, hp.hi, min(hp.negR, v) - 1, ps, pe, inv, xh, xg, za, mp, bi);
        if (hull.npos > 0) {
          label_region(hn.negL + 1, hn.lo, hn.hi, min(hn.negR, v) - 1, ps, pe, inv, xh, xg, za, mn, bi);
        } else {
          // f's gap splits in two (either half may be empty); the other gaps keep their maxima
          const ApSegment sl = ap_segment(aidx, apos, napn, v, f - 1, f, 0), sr = ap_segment(aidx, apos, napn, v, f + 1, f, 0);
          if (f >= 1 && !sl.closed) label_region(sl.sa, f - 1, sl.sa, f - 1, ps, pe, inv, xh, xg, za, mn, bi);
          if (f + 1 < v && !sr.closed) label_region(f + 1, sr.sb, f + 1, sr.sb, ps, pe, inv, xh, xg, za, mn, bi);
          rest = hp.negL + 1 == topgap ? second : v0;
        }
        block_reduce<BlockMaxD, SPAN_WAVES>(mp, mn, smd);
        mn = fmax(mn, rest);
        if (mp > 0.0 && mn > 0.0) g = fmin(fmax(mp + mn - v0, 0.0), 1.0);      // else: the posterior determines the answer
      }
      if (t == 0) gs[f] = (float)g;
      if (g > askg) { askg = g; askt = f; }
    }
    if (t == 0) {
      a.ask_point[n] = askt;
      a.ask_gain[n] = askt < 0 ? 0.f : (float)askg;
      a.value[n] = (float)fmin(fmax(v0, 0.0), 1.0);
    }
  } else if (t == 0) {
    a.ask_point[n] = -1;
    a.ask_gain[n] = -1.0f;
    a.value[n] = -1.0f;
  }
  if (a.gain) {
    // columns [0, T): the gain of the evaluated frames of a live row, 0 elsewhere
    __syncthreads();
    for_each_column(r, a.in.set.ld, [&](int c) { a.gain[r.row + c] = (r.status == SPAN_LIVE && c < r.v) ? gs[c] : 0.f; });
  }
}

}  // namespace

namespace hual {

int launch_al_label_gain(const AlGainArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_label_gain", [&] {
    HUAL_REQUIRE(a.ask_point && a.ask_gain && a.value, "al_label_gain: null output");
    HUAL_REQUIRE(nsel >= 1, "al_label_gain: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  HUAL_REQUIRE(!a.cand || (a.M >= 1 && a.M <= 256), "al_label_gain: cand needs 1 <= M <= 256");
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits (and the candidate list) in, the three values (and the row of gains) out
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + 12.0 + (a.gain ? 4.0 * a.in.set.ld : 0.0) + (a.cand ? 4.0 * a.M : 0.0) + (a.sel ? 4.0 : 0.0)) * grid,
              al_label_gain_kernel, dim3(grid), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_label_gain(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel,
                                  const int32_t* cand, int M, float* gain, int32_t* ask_point, float* ask_gain, float* value,
                                  void* stream) {
  HUAL_REQUIRE(set, "hual_al_label_gain: null set");
  AlGainArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.sel = sel; a.cand = cand; a.M = M; a.gain = gain; a.ask_point = ask_point; a.ask_gain = ask_gain; a.value = value;
  return launch_al_label_gain(a, nsel, (hipStream_t)stream);
}
