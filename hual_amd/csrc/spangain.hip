// hual_al_label_gain (include/hual_seqpan.h): per frame t, the temporal IoU the pseudo-label of hual_al_mbr_label is expected to gain
// from the annotator's answer at t - one-step lookahead under the span posterior given the answered active points, in the evaluation's
// own metric.  Beside spanlabel.hip, whose set A (alpost.h), probabilities (spanprob.h), Z / Z_A and maximisation (spanmbr.h) it shares;
// not in the train step.
//
// One 1024-thread workgroup per selected sample.  V0, the value of today's label, is the maximum of label_region over the regions of A,
// as in al_mbr_label_kernel.  Then a uniform loop over the candidate frames: the answer "inside" leaves one region around the hull
// grown by t; the answer "outside" beside a positive hull moves the nearest negative on t's side, and without a positive splits the gap
// that holds t in two - the other gaps keep the maxima the V0 pass found (the best and the second best with the best one's gap: a
// maximum is exact).  Every branch maximises R / Z_A with the PARENT's Z_A, so the gain is M+ + M- - V0 without a further division.  A
// branch without mass has no positive R (a span of positive weight overlaps itself), which is how a determined answer is recognised.
// The arithmetic is label_region's: float64 sums of one sign in a fixed order, maxima, no atomics, nothing grid wide.
#include "al.h"
#include "prof.h"
#include "spanmbr.h"

using namespace hual;

namespace {

enum AlGainRow { AG_LIVE, AG_POISONED, AG_CONTRADICTORY };

__global__ __launch_bounds__(SPAN_THREADS) void al_label_gain_kernel(AlGainArgs a) {
  __shared__ float ps[256], pe[256];
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[256], xg[256];       // label_region's p_s[l] H_e[l] | p_s[l] G_e[l]
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  __shared__ float gs[256];                 // the gain of the evaluated frames, 0 elsewhere
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.N) return;            // (uniform) an id outside the set writes nothing
  const int T = a.tlen[n];
  const size_t row = (size_t)n * a.ld;
  const bool fits = T >= 1 && T <= 256 && T <= a.ld;      // a longer row is poisoned, as in al_query_kernel
  const int v = fits ? span_clip_len(a.vlen[n], T) : 0;
  if (t < 256) gs[t] = 0.f;
  int status = (v == 0 || span_row_poisoned(a.s0, a.e0, row, v)) ? AG_POISONED : AG_LIVE;      // (uniform)
  double v0 = -1.0, askg = -1.0;            // (uniform from here on: every thread holds the reductions' results)
  int askt = -1;
  if (status == AG_LIVE) {
    span_probabilities(a.s0, a.e0, row, T, v, ps, pe, smf, smd);
    if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;
    const int ap0 = a.ap_off[n], napn = a.ap_off[n + 1] - ap0;
    const int32_t* aidx = a.ap_idx + ap0;
    const int8_t* apos = a.ap_pos + ap0;
    const ApHull hull = ap_hull(aidx, apos, napn, v);
    double zf, za;
    posterior_masses(aidx, apos, napn, v, hull, ps, pe, smd, zf, za);      // (its barriers publish inv)
    if (!(zf > 0.0 && zf < INFINITY)) status = AG_POISONED;
    else if (!(za > 0.0)) status = AG_CONTRADICTORY;
    if (status == AG_LIVE) {
      int bi;                               // (the label itself is hual_al_mbr_label's to report)
      // V0 over the regions of A; without a positive also the second-best gap's maximum and the best one's first frame
      double second = -1.0;
      int topgap = -1;
      if (hull.npos > 0) {
        label_region(hull.negL + 1, hull.lo, hull.hi, min(hull.negR, v) - 1, ps, pe, inv, xh, xg, za, v0, bi);
        v0 = block_reduce<BlockMaxD, SPAN_WAVES>(v0, smd);
      } else {
        for (int cur = 0; cur < v;) {       // the gaps between the negatives, ascending (uniform)
          int nxt = v;
          for (int k = 0; k < napn; ++k) {
            const int f = aidx[k];
            if (!apos[k] && f >= cur && f < nxt) nxt = f;
          }
          if (nxt > cur) {
            double gv = -1.0;
            label_region(cur, nxt - 1, cur, nxt - 1, ps, pe, inv, xh, xg, za, gv, bi);
            gv = block_reduce<BlockMaxD, SPAN_WAVES>(gv, smd);
            if (gv > v0) { second = v0; v0 = gv; topgap = cur; }
            else if (gv > second) second = gv;
          }
          cur = nxt + 1;
        }
      }
      const int count = a.cand ? a.M : v;
      for (int k = 0; k < count; ++k) {     // the candidate frames (uniform)
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
    }
  }
  if (status != AG_LIVE && t == 0) {
    a.ask_point[n] = -1;
    a.ask_gain[n] = -1.0f;
    a.value[n] = -1.0f;
  }
  if (a.gain) {
    // columns [0, T): the gain of the evaluated frames of a live row, 0 elsewhere
    __syncthreads();
    const int Tw = min(max(T, 0), a.ld);
    for (int c = t; c < Tw; c += SPAN_THREADS) a.gain[row + c] = (status == AG_LIVE && c < v) ? gs[c] : 0.f;
  }
}

}  // namespace

namespace hual {

int launch_al_label_gain(const AlGainArgs& a, int nsel, hipStream_t s) {
  HUAL_REQUIRE(a.s0 && a.e0 && a.vlen && a.tlen && a.ap_off && a.ap_idx && a.ap_pos, "al_label_gain: null input");
  HUAL_REQUIRE(a.ask_point && a.ask_gain && a.value, "al_label_gain: null output");
  HUAL_REQUIRE(nsel >= 1, "al_label_gain: nsel >= 1");
  HUAL_REQUIRE(a.N > 0 && a.ld >= 2 && a.ld <= HUAL_AL_MAX_T, "al_label_gain: need N > 0 and 2 <= ld <= 1024");
  HUAL_REQUIRE(!a.cand || (a.M >= 1 && a.M <= 256), "al_label_gain: cand needs 1 <= M <= 256");
  const int grid = a.sel ? nsel : a.N;      // without a list every sample is selected
  // per sample: two rows of logits (and the candidate list) in, the three values (and the row of gains) out
  HUAL_LAUNCH(0.0, (8.0 * a.ld + 12.0 + (a.gain ? 4.0 * a.ld : 0.0) + (a.cand ? 4.0 * a.M : 0.0) + (a.sel ? 4.0 : 0.0)) * grid,
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
  a.ld = set->ld; a.N = set->N; a.vlen = set->vlen; a.tlen = set->tlen;
  a.ap_off = set->ap_off; a.ap_idx = set->ap_idx; a.ap_pos = set->ap_pos;
  a.s0 = s0; a.e0 = e0; a.sel = sel; a.cand = cand; a.M = M; a.gain = gain; a.ask_point = ask_point; a.ask_gain = ask_gain; a.value = value;
  return launch_al_label_gain(a, nsel, (hipStream_t)stream);
}
