// hual_al_mbr_label (include/hual_seqpan.h): the pseudo-label by minimum Bayes risk - the span of the consistent set A of maximal
// expected temporal IoU under the span posterior given the answered active points, its value, and the value of the sample's old span.
// Beside al.hip's hual_al_query, whose set A (alpost.h), probabilities (spanprob.h) and Z / Z_A it shares; not in the train step.
//
// One 1024-thread workgroup per selected sample, four lanes per frame.  No pair of spans is enumerated: A is a union of regions, and the
// maximum over the candidates of a region is spanmbr.h's label_region (the factorisation and its sums are described there).  At most
// v^3 / 2 additions per clip for the full triangle at 8.8 KB of LDS.
#include "al.h"
#include "prof.h"
#include "spanmbr.h"

using namespace hual;

namespace {

enum AlLabelRow { AM_LIVE, AM_POISONED, AM_CONTRADICTORY };

__global__ __launch_bounds__(SPAN_THREADS) void al_mbr_label_kernel(AlLabelArgs a) {
  __shared__ float ps[256], pe[256];
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[256], xg[256];       // p_s[l] H_e[l] | p_s[l] G_e[l] of the current e
  __shared__ float smf[2 * SPAN_WAVES];
  __shared__ double smd[2 * SPAN_WAVES];
  __shared__ double bestv[SPAN_WAVES];
  __shared__ int besti[SPAN_WAVES];
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.N) return;            // (uniform) an id outside the set writes nothing
  const int T = a.tlen[n];
  const size_t row = (size_t)n * a.ld;
  const bool fits = T >= 1 && T <= 256 && T <= a.ld;      // a longer row is poisoned, as in al_query_kernel
  const int v = fits ? span_clip_len(a.vlen[n], T) : 0;
  int status = (v == 0 || span_row_poisoned(a.s0, a.e0, row, v)) ? AM_POISONED : AM_LIVE;      // (uniform)
  if (status == AM_LIVE) {
    span_probabilities(a.s0, a.e0, row, T, v, ps, pe, smf, smd);
    if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;
    const int ap0 = a.ap_off[n], napn = a.ap_off[n + 1] - ap0;
    const int32_t* aidx = a.ap_idx + ap0;
    const int8_t* apos = a.ap_pos + ap0;
    const ApHull hull = ap_hull(aidx, apos, napn, v);
    double zf, za;
    posterior_masses(aidx, apos, napn, v, hull, ps, pe, smd, zf, za);      // (its barriers publish inv)
    const int sbh = min(hull.negR, v) - 1;  // the last end a positive hull allows
    if (!(zf > 0.0 && zf < INFINITY)) status = AM_POISONED;
    else if (!(za > 0.0)) status = AM_CONTRADICTORY;
    if (status == AM_LIVE) {
      double best = -1.0;
      int bi = 0x7fffffff;
      if (hull.npos > 0) {
        label_region(hull.negL + 1, hull.lo, hull.hi, sbh, ps, pe, inv, xh, xg, za, best, bi);
      } else {
        for (int cur = 0; cur < v;) {       // the gaps between the negatives, ascending (uniform)
          int nxt = v;
          for (int k = 0; k < napn; ++k) {
            const int f = aidx[k];
            if (!apos[k] && f >= cur && f < nxt) nxt = f;
          }
          if (nxt > cur) label_region(cur, nxt - 1, cur, nxt - 1, ps, pe, inv, xh, xg, za, best, bi);
          cur = nxt + 1;
        }
      }
      wave_best(best, bi);
      if ((t & 63) == 0) { bestv[t >> 6] = best; besti[t >> 6] = bi; }
      __syncthreads();
      if (t == 0) {
        best_of_waves(bestv, besti, SPAN_WAVES, best, bi);
        a.new_idx[2 * n] = bi >> 8;
        a.new_idx[2 * n + 1] = bi & 255;
        a.conf[n] = (float)fmin(fmax(best, 0.0), 1.0);
      }
      if (a.old_idx) {
        // R of the old span by one walk over A: the quad of start g takes the ends its region allows
        const int oa = a.old_idx[2 * n], oe = a.old_idx[2 * n + 1];
        const bool valid = oa >= 0 && oa <= oe && oe < v;      // (uniform)
        const int g = t / AM_QUAD, q = t % AM_QUAD;
        double acc = 0.0;
        if (valid && g < v) {
          int jl = 0, jh = -1;
          if (hull.npos > 0) {
            if (g > hull.negL && g <= hull.lo) { jl = hull.hi; jh = sbh; }
          } else {
            const ApSegment sg = ap_segment(aidx, apos, napn, v, g);
            if (!sg.closed) { jl = g; jh = sg.sb; }
          }
          const int len = oe - oa + 1;
          for (int j = jl + q; j <= jh; j += AM_QUAD) {
            const int inter = min(oe, j) + 1 - max(oa, g);
            if (inter <= 0) continue;
            const int uni = len + (j - g + 1) - inter;
            acc += ((double)ps[g] * (double)pe[j]) * ((double)inter / (double)uni);
          }
        }
        acc = block_reduce<BlockSumD, SPAN_WAVES>(acc, smd);
        if (t == 0) a.old_conf[n] = valid ? (float)fmin(fmax(acc / za, 0.0), 1.0) : -1.0f;
      }
    }
  }
  if (status != AM_LIVE && t == 0) {
    a.new_idx[2 * n] = -1;
    a.new_idx[2 * n + 1] = -1;
    a.conf[n] = -1.0f;
    if (a.old_conf) a.old_conf[n] = -1.0f;
  }
}

}  // namespace

namespace hual {

int launch_al_mbr_label(const AlLabelArgs& a, int nsel, hipStream_t s) {
  HUAL_REQUIRE(a.s0 && a.e0 && a.vlen && a.tlen && a.ap_off && a.ap_idx && a.ap_pos, "al_mbr_label: null input");
  HUAL_REQUIRE(a.new_idx && a.conf, "al_mbr_label: null output");
  HUAL_REQUIRE(!a.old_idx == !a.old_conf, "al_mbr_label: old_idx and old_conf are both set or both null");
  HUAL_REQUIRE(nsel >= 1, "al_mbr_label: nsel >= 1");
  HUAL_REQUIRE(a.N > 0 && a.ld >= 2 && a.ld <= HUAL_AL_MAX_T, "al_mbr_label: need N > 0 and 2 <= ld <= 1024");
  const int grid = a.sel ? nsel : a.N;      // without a list every sample is selected
  // per sample: two rows of logits in, the label and its value out (and the old span in, its value out)
  HUAL_LAUNCH(0.0, (8.0 * a.ld + 12.0 + (a.old_idx ? 12.0 : 0.0) + (a.sel ? 4.0 : 0.0)) * grid, al_mbr_label_kernel, dim3(grid),
              dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_mbr_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel,
                                 const int32_t* old_idx, int32_t* new_idx, float* conf, float* old_conf, void* stream) {
  HUAL_REQUIRE(set, "hual_al_mbr_label: null set");
  AlLabelArgs a{};
  a.ld = set->ld; a.N = set->N; a.vlen = set->vlen; a.tlen = set->tlen;
  a.ap_off = set->ap_off; a.ap_idx = set->ap_idx; a.ap_pos = set->ap_pos;
  a.s0 = s0; a.e0 = e0; a.sel = sel; a.old_idx = old_idx; a.new_idx = new_idx; a.conf = conf; a.old_conf = old_conf;
  return launch_al_mbr_label(a, nsel, (hipStream_t)stream);
}
