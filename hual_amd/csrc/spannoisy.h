// The span posterior under an annotator who errs with probability eps, for the two launches of spannoisy.hip (hual_al_noisy_tilt,
// hual_al_label_gain_noisy; the contract is in include/hual_seqpan.h).  With r = (1 - eps) / eps and G(t) = (positive answers at frames
// <= t) - (negative answers at frames <= t), the likelihood of the answers under the span (i, j) is a constant times r^(G(j) - G(i-1)),
// so the posterior is the product form of the logits tilted by -G(i-1) ln r and +G(j) ln r on the WHOLE triangle: no consistent set, no
// contradictory row.  Here: the opening of such a row (spanpost.h's, with no active point read) and the IoU-weighted mass of a
// candidate span against one region of the triangle - spanmbr.h's factorisation with the region's bounds clamped and candidates
// outside the region admitted (label_region itself stays as it is: the bits of the kernels that call it do not move).
#pragma once
#include "spanmbr.h"

namespace hual {

// hual_al_noisy_tilt
struct AlTiltArgs {
  AlSpanIn in;                                // the set with its answers, the untilted logits
  float lam;                                  // (float)ln r
  double lnr, ln_eps, ln_1meps;               // ln r, ln eps, ln(1 - eps) in float64 (the host's)
  float *s_t, *e_t;                           // [N, ld] the tilted logits, columns [0, tlen[n])
  float* log_evidence;                        // [N] ln P(the answers | the model, eps)
};

// hual_al_label_gain_noisy
struct AlNoisyGainArgs {
  AlSpanIn in;                                // the set (N, ld, vlen, tlen: the active points are not read), the TILTED logits
  double eps;
  const int32_t* sel;                         // [nsel] sample ids to evaluate (NULL: all)
  const int32_t* cand;                        // [N, M] the frames to evaluate, entries outside [0, v) skipped (NULL: every frame)
  int M;
  float* gain;                                // [N, ld] columns [0, tlen[n]) (NULL: not written)
  int32_t* ask_point;                         // [N] first evaluated frame of maximal gain (rows of unselected samples are left untouched)
  float *ask_gain, *value;                    // [N] that gain | V0, the conf of hual_al_mbr_label on the same rows without answers
};

int launch_al_noisy_tilt(const AlTiltArgs& a, hipStream_t s);
int launch_al_label_gain_noisy(const AlNoisyGainArgs& a, int nsel, hipStream_t s);

// x + (float)g * lam: one float32 product and one float32 addition, each rounded on its own, as h2_bits (al.h) states such arithmetic.
// (__fmul_rn / __fadd_rn are plain operators that carry the contraction flag of the header that defines them: the compiler fused the
// pair into one v_pk_fma_f32 for both heads, which no pragma here reaches.)  g == 0 copies x, so that -0 stays -0
__device__ __forceinline__ float tilt_logit(float x, int g, float lam) {
#pragma clang fp contract(off)
  if (g == 0) return x;
  const float p = (float)g * lam;
  return x + p;
}

}  // namespace hual

// stage 1 of spanpost.h's opening for a row whose answers are already in its logits: the same T, v, status and probabilities, an
// empty list of active points in place of the set's (ap_hull / ap_segment never dereference an empty list).  Called by the whole
// workgroup; its barriers publish what was written before it.
__device__ __forceinline__ void open_free_row(const hual::AlSpanIn& in, int n, SpanRowLds& lds, SpanRow& r) {
  r.T = in.set.tlen[n];
  r.row = (size_t)n * in.set.ld;
  const bool fits = r.T >= 1 && r.T <= 256 && r.T <= in.set.ld;
  r.v = fits ? span_clip_len(in.set.vlen[n], r.T) : 0;
  r.status = (r.v == 0 || span_row_poisoned(in.s0, in.e0, r.row, r.v)) ? SPAN_POISONED : SPAN_LIVE;
  if (r.status == SPAN_LIVE) {
    span_probabilities(in.s0, in.e0, r.row, r.T, r.v, lds.ps, lds.pe, lds.smf, lds.smd);
    r.napn = 0;
    r.aidx = nullptr;
    r.apos = nullptr;
    r.hull = ap_hull(r.aidx, r.apos, 0, r.v);
  }
}

// stage 2: Z over the whole triangle by posterior_masses (Z_A == Z: nothing is ruled out) and the row's final status
__device__ __forceinline__ void open_free_posterior_row(const hual::AlSpanIn& in, int n, SpanRowLds& lds, SpanRow& r) {
  open_free_row(in, n, lds, r);
  if (r.status == SPAN_LIVE) {
    posterior_masses(r.aidx, r.apos, 0, r.v, r.hull, lds.ps, lds.pe, lds.smd, r.zf, r.za);
    r.status = posterior_status(r.zf, r.za);
  }
}

// one region of the triangle: the spans (i, j) with sa <= i <= ihi, jlo <= j <= sb, i <= j (empty where a bound pair is crossed)
struct NoisyRegion {
  int sa, ihi, jlo, sb;
};

// The IoU-weighted mass F(a, e) = sum over the region's spans of p_s[i] p_e[j] IoU((a, e), (i, j)) of ANY candidate 0 <= a <= e, in the
// walk of label_region: e descends, the quad of frame g holds
//   G_e[g] = sum_{j = max(g, jlo) .. min(e, sb)} p_e[j] (j - g + 1)        H_e[g] = sum_{j = max(e + 1, jlo) .. sb} p_e[j] / (j - g + 1)
// and F is the four cases of (i < a or i >= a) x (j <= e or j > e), every start clamped to [sa, ihi]:
//   G_e[a] sum_{i = sa .. min(a - 1, ihi)} p_s[i] / (e - i + 1)  +  (e - a + 1) sum_{i = sa .. min(a - 1, ihi)} p_s[i] H_e[i]
//   +  sum_{i = max(a, sa) .. min(ihi, e)} p_s[i] G_e[i] / (e - a + 1)  +  H_e[a] sum_{i = max(a, sa) .. min(ihi, e)} p_s[i] (e - i + 1)
// Three steps per e, so that several regions share the walk's two barriers: region_publish, a barrier, region_mass, a barrier,
// region_advance.  Every sum adds terms of one sign in float64 in a fixed order, as label_region's.

// G_e[g] of the quad's frame g <= e -> G (in every lane of the quad); p_s[g] H_e[g] and p_s[g] G_e[g] -> xh / xg where g is a start of
// the region
__device__ __forceinline__ void region_publish(const NoisyRegion& R, int e, int g, int q, double H, const float* ps, const float* pe,
                                               double* xh, double* xg, double& G) {
  G = 0.0;
  if (g <= e)
    for (int j = max(g, R.jlo) + q; j <= min(e, R.sb); j += AM_QUAD) G += (double)pe[j] * (double)(j - g + 1);
  G = quad_sum(G);
  if (g <= e && g >= R.sa && g <= R.ihi && q == 0) { xh[g] = (double)ps[g] * H; xg[g] = (double)ps[g] * G; }
}

// F(g, e) of the quad's frame g <= e (in every lane of the quad); 0 for g > e
__device__ __forceinline__ double region_mass(const NoisyRegion& R, int e, int g, int q, double H, double G, const float* ps,
                                              const double* inv, const double* xh, const double* xg) {
  double p1 = 0.0, p2 = 0.0, s3 = 0.0, s4 = 0.0;
  if (g <= e) {
    const int m = min(R.ihi, e);
    for (int i = R.sa + q; i <= min(g - 1, R.ihi); i += AM_QUAD) { p1 += (double)ps[i] * inv[e - i + 1]; p2 += xh[i]; }
    for (int i = max(g, R.sa) + q; i <= m; i += AM_QUAD) { s3 += xg[i]; s4 += (double)ps[i] * (double)(e - i + 1); }
  }
  p1 = quad_sum(p1); p2 = quad_sum(p2); s3 = quad_sum(s3); s4 = quad_sum(s4);
  const double len = (double)(e - g + 1);
  return g <= e ? G * p1 + len * p2 + s3 / len + H * s4 : 0.0;
}

// H_e[g] -> H_{e-1}[g]: the end e joins the ends above the candidate's
__device__ __forceinline__ void region_advance(const NoisyRegion& R, int e, int g, const float* pe, const double* inv, double& H) {
  if (g <= e && e >= R.jlo && e <= R.sb) H += (double)pe[e] * inv[e - g + 1];
}
