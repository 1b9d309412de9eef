// hual_al_noisy_tilt and hual_al_label_gain_noisy (include/hual_seqpan.h): the span posterior under an annotator who errs with
// probability eps.  The identity and the helpers are in spannoisy.h; not in the train step.
//
// hual_al_noisy_tilt - one 1024-thread workgroup per sample - folds the answers into the logits (every launch of the family then reads
// the noisy posterior from the tilted rows and a set without answers) and reports the evidence of the answers under the untilted model,
//   ln [ eps^npos (1 - eps)^nneg sum_j p_e[j] r^G(j) sum_{i <= j} p_s[i] r^-G(i-1) / Z ].
// The powers of r are carried as integer exponents: frame j's inner sum against the largest exponent among its own starts, its term
// against the largest exponent K of the whole triangle, which leaves the logarithm as K ln r - so 64 answers at eps = 1e-6 neither
// overflow nor underflow the spans that carry the sum.
//
// hual_al_label_gain_noisy - one 1024-thread workgroup per selected sample - is the one-step lookahead of hual_al_label_gain rebuilt for
// an answer that re-weights the triangle instead of cutting it.  V0 is label_region over the whole triangle, as hual_al_mbr_label
// computes it on a set without answers.  Then a uniform loop over the candidate frames t: one walk of the ends e, in which the quad of
// start a holds the IoU-weighted mass of the candidate (a, e) against the rectangle of the spans that hold t and against the two
// triangles of those that do not (region_mass), and keeps the maxima of (1 - eps) F_in + eps F_out and eps F_in + (1 - eps) F_out.
// About v^3 additions per frame, v^4 per clip with every frame; float64 sums of one sign in a fixed order, maxima, no
// atomics, nothing grid wide.
#include "prof.h"
#include "spannoisy.h"

#include <cmath>

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_noisy_tilt_kernel(AlTiltArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ int gs[257];                   // gs[t + 1] = G(t), gs[0] = G(-1) = 0
  const int n = blockIdx.x, t = threadIdx.x;
  SpanRow r;
  open_span_row(a.in, n, lds, r);
  double ev = NAN;
  if (r.status == SPAN_LIVE) {
    const float *ps = lds.ps, *pe = lds.pe;
    const int v = r.v;
    int G = 0, npos = 0, nneg = 0;          // (npos / nneg uniform: every thread walks the whole list)
    for (int k = 0; k < r.napn; ++k) {
      const int f = r.aidx[k];
      if (f < 0 || f >= v) continue;
      const int sgn = r.apos[k] ? 1 : -1;
      if (sgn > 0) ++npos; else ++nneg;
      if (f <= t) G += sgn;
    }
    if (t < v) gs[t + 1] = G;
    if (t == 0) gs[0] = 0;
    __syncthreads();
    // frame t's share of the two sums: the likelihood-weighted one against its own largest exponent, and Z
    double inner = 0.0, plain = 0.0, kt = -INFINITY;
    if (t < v) {
      int amax = -0x7fffffff;
      for (int i = 0; i <= t; ++i) amax = max(amax, -gs[i]);
      for (int i = 0; i <= t; ++i) {
        inner += (double)ps[i] * exp((double)(-gs[i] - amax) * a.lnr);
        plain += (double)ps[i];
      }
      kt = (double)(gs[t + 1] + amax);
    }
    const double kmax = block_reduce<BlockMaxD, SPAN_WAVES>(kt, lds.smd);
    double sum = 0.0, zf = 0.0;
    if (t < v) {
      sum = (double)pe[t] * inner * exp((kt - kmax) * a.lnr);
      zf = (double)pe[t] * plain;
    }
    block_reduce<BlockSumD, SPAN_WAVES>(sum, zf, lds.smd);
    if (zf > 0.0 && zf < INFINITY)
      ev = (double)npos * a.ln_eps + (double)nneg * a.ln_1meps + kmax * a.lnr + log(sum) - log(zf);
    else
      r.status = SPAN_POISONED;             // every weight underflowed, or an infinite logit made them NaN
  }
  if (t == 0) a.log_evidence[n] = (float)ev;
  // columns [0, T): the tilted logits below v of a live row, raw copies elsewhere
  for_each_column(r, a.in.set.ld, [&](int c) {
    float s = a.in.s0[r.row + c], e = a.in.e0[r.row + c];
    if (r.status == SPAN_LIVE && c < r.v && a.lam != 0.f) {
      s = tilt_logit(s, -gs[c], a.lam);
      e = tilt_logit(e, gs[c + 1], a.lam);
    }
    a.s_t[r.row + c] = s;
    a.e_t[r.row + c] = e;
  });
}

__global__ __launch_bounds__(SPAN_THREADS) void al_label_gain_noisy_kernel(AlNoisyGainArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[256], xg[256];       // p_s[l] H_e[l] | p_s[l] G_e[l] of the rectangle (and label_region's, for V0)
  __shared__ double yh[256], yg[256];       // the same of the two triangles: their starts lie on either side of t
  __shared__ float gs[256];                 // the gain of the evaluated frames, 0 elsewhere
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  if (t < 256) gs[t] = 0.f;
  if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;      // (the opening's barriers publish both)
  SpanRow r;
  open_free_posterior_row(a.in, n, lds, r);
  if (r.status == SPAN_LIVE) {
    const float *ps = lds.ps, *pe = lds.pe;
    double* smd = lds.smd;
    const int v = r.v;
    const double za = r.za, eps = a.eps, cps = 1.0 - a.eps;
    const int g = t / AM_QUAD, q = t % AM_QUAD;
    double v0 = -1.0, askg = -1.0;          // (uniform: every thread holds the reductions' results)
    int askt = -1;
    int bi;                                 // (the label itself is hual_al_mbr_label's to report)
    label_region(0, v - 1, 0, v - 1, ps, pe, inv, xh, xg, za, v0, bi);
    v0 = block_reduce<BlockMaxD, SPAN_WAVES>(v0, smd);
    const int count = a.cand ? a.M : v;
    for (int k = 0; k < count; ++k) {       // the candidate frames (uniform)
      const int f = a.cand ? a.cand[(size_t)n * a.M + k] : k;
      if (f < 0 || f >= v) continue;
      const NoisyRegion in{0, f, f, v - 1}, lo{0, f - 1, 0, f - 1}, hi{f + 1, v - 1, f + 1, v - 1};
      double Hi = 0.0, Hl = 0.0, Hh = 0.0;  // H_e[g] of the three regions
      double my = -1.0, mn = -1.0;
      for (int e = v - 1; e >= 0; --e) {
        double Gi, Gl, Gh;
        region_publish(in, e, g, q, Hi, ps, pe, xh, xg, Gi);
        region_publish(lo, e, g, q, Hl, ps, pe, yh, yg, Gl);
        region_publish(hi, e, g, q, Hh, ps, pe, yh, yg, Gh);
        __syncthreads();
        const double fin = region_mass(in, e, g, q, Hi, Gi, ps, inv, xh, xg);
        const double fout = region_mass(lo, e, g, q, Hl, Gl, ps, inv, yh, yg) + region_mass(hi, e, g, q, Hh, Gh, ps, inv, yh, yg);
        if (g <= e) {
          my = fmax(my, cps * fin + eps * fout);
          mn = fmax(mn, eps * fin + cps * fout);
        }
        __syncthreads();                    // xh / xg, yh / yg are rewritten by the next step
        region_advance(in, e, g, pe, inv, Hi);
        region_advance(lo, e, g, pe, inv, Hl);
        region_advance(hi, e, g, pe, inv, Hh);
      }
      block_reduce<BlockMaxD, SPAN_WAVES>(my, mn, smd);
      const double gn = fmin(fmax((my + mn) / za - v0, 0.0), 1.0);      // >= 0 in exact arithmetic: the candidates are not restricted
      if (t == 0) gs[f] = (float)gn;
      if (gn > askg) { askg = gn; askt = f; }
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

// eps in (0, 0.5]; a NaN fails the comparison
bool eps_ok(float eps) { return eps > 0.f && eps <= 0.5f; }

}  // namespace

namespace hual {

int launch_al_noisy_tilt(const AlTiltArgs& a, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_noisy_tilt", [&] {
    HUAL_REQUIRE(a.s_t && a.e_t && a.log_evidence, "al_noisy_tilt: null output");
    return 0;
  });
  if (rc) return rc;
  // per sample: two rows of logits in, two out, the evidence
  HUAL_LAUNCH(0.0, (16.0 * a.in.set.ld + 4.0) * a.in.set.N, al_noisy_tilt_kernel, dim3(a.in.set.N), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_al_label_gain_noisy(const AlNoisyGainArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_label_gain_noisy", [&] {
    HUAL_REQUIRE(a.ask_point && a.ask_gain && a.value, "al_label_gain_noisy: null output");
    HUAL_REQUIRE(nsel >= 1, "al_label_gain_noisy: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  HUAL_REQUIRE(!a.cand || (a.M >= 1 && a.M <= 256), "al_label_gain_noisy: cand needs 1 <= M <= 256");
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits (and the candidate list) in, the three values (and the row of gains) out
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + 12.0 + (a.gain ? 4.0 * a.in.set.ld : 0.0) + (a.cand ? 4.0 * a.M : 0.0) + (a.sel ? 4.0 : 0.0)) * grid,
              al_label_gain_noisy_kernel, dim3(grid), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_noisy_tilt(const hual_al_set* set, const float* s0, const float* e0, float eps, float* s_t, float* e_t,
                                  float* log_evidence, void* stream) {
  HUAL_REQUIRE(set, "hual_al_noisy_tilt: null set");
  HUAL_REQUIRE(eps_ok(eps), "hual_al_noisy_tilt: eps in (0, 0.5]");
  AlTiltArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  const double de = (double)eps;
  a.lnr = std::log((1.0 - de) / de); a.ln_eps = std::log(de); a.ln_1meps = std::log1p(-de);
  a.lam = (float)a.lnr;
  a.s_t = s_t; a.e_t = e_t; a.log_evidence = log_evidence;
  return launch_al_noisy_tilt(a, (hipStream_t)stream);
}

extern "C" int hual_al_label_gain_noisy(const hual_al_set* set, const float* s_t, const float* e_t, float eps, const int32_t* sel,
                                        int nsel, const int32_t* cand, int M, float* gain, int32_t* ask_point, float* ask_gain,
                                        float* value, void* stream) {
  HUAL_REQUIRE(set, "hual_al_label_gain_noisy: null set");
  HUAL_REQUIRE(eps_ok(eps), "hual_al_label_gain_noisy: eps in (0, 0.5]");
  AlNoisyGainArgs a{};
  a.in.set = *set; a.in.s0 = s_t; a.in.e0 = e_t;
  a.eps = (double)eps;
  a.sel = sel; a.cand = cand; a.M = M; a.gain = gain; a.ask_point = ask_point; a.ask_gain = ask_gain; a.value = value;
  return launch_al_label_gain_noisy(a, nsel, (hipStream_t)stream);
}
