// hual_al_mbr_label (include/hual_seqpan.h): the pseudo-label by minimum Bayes risk - the span of the consistent set A of maximal
// expected temporal IoU under the span posterior given the answered active points, its value, and the value of the sample's old span.
// Beside al.hip's hual_al_query, whose set A (alpost.h), probabilities (spanprob.h) and Z / Z_A it shares; not in the train step.
//
// One 1024-thread workgroup per selected sample, four lanes per frame.  No pair of spans is enumerated.  A is a union of regions
// {sa <= i <= ihi, jlo <= j <= sb, i <= j} (a gap between negatives: ihi = sb, jlo = sa; a positive hull: (negL, lo] x [hi, negR)), and a
// candidate (a, e) overlaps only the spans of its own region.  With, for a fixed end e,
//   G_e[m] = sum_{j = max(m, jlo) .. e} p_e[j] (j - m + 1)        H_e[l] = sum_{j = e + 1 .. sb} p_e[j] / (j - l + 1)
// the IoU-weighted mass Z_A R(a, e) is the sum of the four cases of (i < a or i >= a) x (j <= e or j > e):
//   G_e[a] sum_{i < a} p_s[i] / (e - i + 1)  +  (e - a + 1) sum_{i < a} p_s[i] H_e[i]
//   +  sum_{i = a .. min(ihi, e)} p_s[i] G_e[i] / (e - a + 1)  +  H_e[a] sum_{i = a .. min(ihi, e)} p_s[i] (e - i + 1)
// The workgroup walks e down from sb; the quad of frame l keeps H_e[l] in a register (one term added per step), sums G_e[l] over j,
// publishes p_s[l] H_e[l] and p_s[l] G_e[l] in LDS, and after a barrier sums its own two prefixes and two suffixes over i.  Every sum
// adds terms of one sign in float64 in a fixed order (a lane takes every fourth term, the quad is folded by two shuffles): no difference
// of prefix sums, no atomics, nothing grid wide.  At most v^3 / 2 additions per clip for the full triangle at 8.8 KB of LDS.
#include "al.h"
#include "alpost.h"
#include "prof.h"
#include "spanprob.h"

using namespace hual;

namespace {

enum AlLabelRow { AM_LIVE, AM_POISONED, AM_CONTRADICTORY };

constexpr int AM_QUAD = 4;      // lanes per frame

// the sum over the four lanes of a frame, in every one of them
__device__ __forceinline__ double quad_sum(double x) {
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  return x;
}

// the candidates (a, e) of one region, a = the quad's frame g: best / bi <- the first maximal R = (IoU-weighted mass) / za in row-major
// order, bi = a * 256 + e.  Called by the whole workgroup with uniform arguments; starts and ends on a barrier-free state of xh / xg
// (its last statement of an iteration is a barrier).
__device__ __forceinline__ void label_region(int sa, int ihi, int jlo, int sb, const float* ps, const float* pe, const double* inv,
                                             double* xh, double* xg, double za, double& best, int& bi) {
  const int g = threadIdx.x / AM_QUAD, q = threadIdx.x % AM_QUAD;
  double H = 0.0;                           // H_e[g]
  for (int e = sb; e >= jlo; --e) {
    const int m = min(ihi, e);
    const bool on = g >= sa && g <= m;
    double G = 0.0;                         // G_e[g]
    if (on)
      for (int j = max(g, jlo) + q; j <= e; j += AM_QUAD) G += (double)pe[j] * (double)(j - g + 1);
    G = quad_sum(G);
    if (on && q == 0) { xh[g] = (double)ps[g] * H; xg[g] = (double)ps[g] * G; }
    __syncthreads();
    double p1 = 0.0, p2 = 0.0, s3 = 0.0, s4 = 0.0;
    if (on) {
      for (int i = sa + q; i < g; i += AM_QUAD) { p1 += (double)ps[i] * inv[e - i + 1]; p2 += xh[i]; }
      for (int i = g + q; i <= m; i += AM_QUAD) { s3 += xg[i]; s4 += (double)ps[i] * (double)(e - i + 1); }
    }
    p1 = quad_sum(p1); p2 = quad_sum(p2); s3 = quad_sum(s3); s4 = quad_sum(s4);
    if (on) {
      const double len = (double)(e - g + 1);
      const double r = (G * p1 + len * p2 + s3 / len + H * s4) / za;
      if (r >= best) { best = r; bi = g * 256 + e; }      // e descends: among equal values the smallest e stays
    }
    __syncthreads();                        // xh / xg are rewritten by the next step
    if (g <= e) H += (double)pe[e] * inv[e - g + 1];
  }
}

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
    // Z over the whole triangle and Z_A over the gaps' triangles, frame t's share: p_e[t] times the sum of p_s over the frames <= t (of
    // its segment), the sums of al_query_kernel in its order
    double zf = 0.0, za = 0.0;
    if (t < v) {
      const ApSegment sg = ap_segment(aidx, apos, napn, v, t);
      double below = 0.0, seg = 0.0;
      for (int i = 0; i < sg.sa; ++i) below += (double)ps[i];
      for (int i = sg.sa; i <= t; ++i) seg += (double)ps[i];
      zf = (double)pe[t] * (below + seg);
      za = sg.closed ? 0.0 : (double)pe[t] * seg;
    }
    block_reduce<BlockSumD, SPAN_WAVES>(zf, za, smd);      // (its barriers publish inv)
    const int sbh = min(hull.negR, v) - 1;  // the last end a positive hull allows
    if (hull.npos > 0) {                    // starts in (negL, lo] x ends in [hi, negR)
      double S = 0.0, E = 0.0;
      for (int i = hull.negL + 1; i <= hull.lo; ++i) S += (double)ps[i];
      for (int j = hull.hi; j <= sbh; ++j) E += (double)pe[j];
      za = hull.inside ? 0.0 : S * E;
    }
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
