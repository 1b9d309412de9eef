// hual_al_mbr_label (include/hual_seqpan.h): the pseudo-label by minimum Bayes risk - the span of the consistent set A of maximal
// expected temporal IoU under the span posterior given the answered active points, its value, and the value of the sample's old span.
// The row - its status, probabilities (spanprob.h), set A and Z / Z_A - is opened by spanpost.h, as in every launch of the family; not in
// the train step.
//
// One 1024-thread workgroup per selected sample, four lanes per frame.  No pair of spans is enumerated: A is a union of regions, and the
// maximum over the candidates of a region is spanmbr.h's label_region (the factorisation and its sums are described there).  At most
// v^3 / 2 additions per clip for the full triangle at 9.0 KB of LDS.
#include "prof.h"
#include "spanmbr.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_mbr_label_kernel(AlLabelArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[256], xg[256];       // p_s[l] H_e[l] | p_s[l] G_e[l] of the current e
  __shared__ double bestv[SPAN_WAVES];
  __shared__ int besti[SPAN_WAVES];
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;      // (the opening's barriers publish it)
  SpanRow r;
  open_posterior_row(a.in, n, lds, r);
  if (r.status == SPAN_LIVE) {
    const float *ps = lds.ps, *pe = lds.pe;
    const ApHull& hull = r.hull;
    const int v = r.v;
    const double za = r.za;
    const int sbh = min(hull.negR, v) - 1;  // the last end a positive hull allows
    double best = -1.0;
    int bi = 0x7fffffff;
    if (hull.npos > 0)
      label_region(hull.negL + 1, hull.lo, hull.hi, sbh, ps, pe, inv, xh, xg, za, best, bi);
    else
      for_each_gap(r, [&](int first, int last) { label_region(first, last, first, last, ps, pe, inv, xh, xg, za, best, bi); });
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
          const ApSegment sg = ap_segment(r.aidx, r.apos, r.napn, v, g);
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
      acc = block_reduce<BlockSumD, SPAN_WAVES>(acc, lds.smd);
      if (t == 0) a.old_conf[n] = valid ? (float)fmin(fmax(acc / za, 0.0), 1.0) : -1.0f;
    }
  } else if (t == 0) {
    a.new_idx[2 * n] = -1;
    a.new_idx[2 * n + 1] = -1;
    a.conf[n] = -1.0f;
    if (a.old_conf) a.old_conf[n] = -1.0f;
  }
}

}  // namespace

namespace hual {

int launch_al_mbr_label(const AlLabelArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_mbr_label", [&] {
    HUAL_REQUIRE(a.new_idx && a.conf, "al_mbr_label: null output");
    HUAL_REQUIRE(!a.old_idx == !a.old_conf, "al_mbr_label: old_idx and old_conf are both set or both null");
    HUAL_REQUIRE(nsel >= 1, "al_mbr_label: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits in, the label and its value out (and the old span in, its value out)
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + 12.0 + (a.old_idx ? 12.0 : 0.0) + (a.sel ? 4.0 : 0.0)) * grid, al_mbr_label_kernel, dim3(grid),
              dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_mbr_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel,
                                 const int32_t* old_idx, int32_t* new_idx, float* conf, float* old_conf, void* stream) {
  HUAL_REQUIRE(set, "hual_al_mbr_label: null set");
  AlLabelArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.sel = sel; a.old_idx = old_idx; a.new_idx = new_idx; a.conf = conf; a.old_conf = old_conf;
  return launch_al_mbr_label(a, nsel, (hipStream_t)stream);
}
