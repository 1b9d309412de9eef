// hual_al_ensemble_query and hual_al_ensemble_label (include/hual_seqpan.h): the span posterior as a Bayesian model average over K
// stochastic passes.  The predictive distribution is the mixture P(i,j) = (1/K) sum_k P_k(i,j), every P_k the product form the family
// opens; conditioning on the answers keeps it a mixture, P(i,j | answers) = sum_k w_k P_k(i,j | answers), w_k proportional to pass k's
// evidence of the answers Z_A,k / Z_k (times a caller's prior weight).  Not in the train step.
//
// One 1024-thread workgroup per sample.  open_ensemble_row opens every pass with spanpost.h's own opening on plane k - the consistent
// set A depends on the answers and v only and is shared -, keeps the K pairs of factor rows in LDS (K * 2 * 256 floats, 32 KB at K = 16)
// and leaves the weights: the one definition both launches read.
//
// What is linear in the posterior is the w-weighted sum of what the family computes per pass, by the family's own code per pass: q(t)
// from spanstep.h's query_step, the marginals by spanmarg.hip's interval sums, the expected tIoU of a candidate by spannoisy.h's
// region_publish / region_mass / region_advance (spanmbr.h's factorisation in steps, so that the passes are summed per candidate before
// the argmax).  With K = 1 the weight is exactly 1.0 and every such output is the single-pass launch's bit for bit.
// What is not linear: the entropy of the mixture has no product form and is a walk over the pairs of A - the quad of start i strides
// over its ends, m(i,j) = sum_k (w_k / Z_A,k) p_s,k[i] p_e,k[j] from LDS, float64, one fixed-order block sum, no atomics.  At most
// K v^2 / 2 multiply-adds per clip beside one log2 per pair.
#include "prof.h"
#include "spannoisy.h"
#include "spanstep.h"

#include <cmath>

using namespace hual;

namespace {

constexpr int ENS_MAX_K = 16;

struct AlEnsIn {
  hual_al_set set;
  const float *pass_s, *pass_e;               // [K, N, ld] start / end logits of the passes, plane stride N * ld
  int K;
  const float* logw;                          // [K, N] log prior weight per pass and row (NULL: 0)
};

struct AlEnsQueryArgs {
  AlEnsIn in;
  float* weight;                              // [N, K]
  float* log_evidence;                        // [N]
  float *incl, *gain;                         // [N, ld] columns [0, tlen[n]) (NULL: not written)
  int32_t* query_point;                       // [N]
  float* query_gain;                          // [N]
  float *y_start, *y_end;                     // [N, ld] columns [0, tlen[n]) (NULL, both: not computed)
  float *post_entropy, *expected_entropy, *span_bald;      // [N]
  int32_t* status;                            // [N] 1 = live
};

struct AlEnsLabelArgs {
  AlEnsIn in;
  const int32_t* sel;                         // [nsel] sample ids to label (NULL: all)
  const int32_t* old_idx;                     // [N, 2] (NULL with old_conf: not scored)
  int32_t* new_idx;                           // [N, 2] (rows of unselected samples are left untouched, as conf and old_conf)
  float *conf, *old_conf;                     // [N]
};

// the LDS of an opened ensemble row beside SpanRowLds
struct EnsLds {
  float ps[ENS_MAX_K][256], pe[ENS_MAX_K][256];      // the passes' factor rows (spanprob.h)
  double zf[ENS_MAX_K], za[ENS_MAX_K];        // Z_k | Z_A,k, 0 where it is not positive
  double w[ENS_MAX_K], c[ENS_MAX_K];          // the weight w_k | w_k / Z_A,k, both 0 on a pass without weight
  double logev;
  int status;                                 // SpanRowStatus of the row
};

// Sample n's row under every pass.  r: T, v, row always; the active points and the hull on a row that is not POISONED (they depend on
// the set only: the last pass's opening left them); r.status: POISONED if any pass is by hual_al_query's rule, CONTRADICTORY if no pass
// has weight, else LIVE with el.ps / el.pe, el.za, el.w, el.c and el.logev readable.
//   u_k = ln(Z_A,k / Z_k) + logw[k][n];  a pass whose Z_A,k is not positive, or whose u_k is not finite, has no weight;
//   w_k = exp(u_k - max u) / sum;  logev = max u + ln(sum) - ln K  (-inf on a CONTRADICTORY row)
// in float64, the passes in ascending k.  Called by the whole workgroup; ends on a barrier.
__device__ __forceinline__ void open_ensemble_row(const AlEnsIn& a, int n, SpanRowLds& lds, EnsLds& el, SpanRow& r) {
  const int t = threadIdx.x;
  const size_t plane = (size_t)a.set.N * a.set.ld;
  bool poisoned = false;
  for (int k = 0; k < a.K && !poisoned; ++k) {
    AlSpanIn in;
    in.set = a.set; in.s0 = a.pass_s + k * plane; in.e0 = a.pass_e + k * plane;
    open_posterior_row(in, n, lds, r);
    poisoned = r.status == SPAN_POISONED;
    if (!poisoned) {
      // (thread t copies what it wrote itself; the next opening's first barrier stands between the readers of lds.ps / lds.pe and it)
      if (t < 256) { el.ps[k][t] = lds.ps[t]; el.pe[k][t] = lds.pe[t]; }
      if (t == 0) { el.zf[k] = r.zf; el.za[k] = r.status == SPAN_LIVE ? r.za : 0.0; }
    }
  }
  if (poisoned) {
    r.status = SPAN_POISONED;
    __syncthreads();
    return;
  }
  __syncthreads();
  if (t == 0) {
    const int K = a.K;
    double umax = -INFINITY;
    for (int k = 0; k < K; ++k) {             // (el.w holds u_k until the weights are formed)
      double u = -INFINITY;
      if (el.za[k] > 0.0) u = log(el.za[k] / el.zf[k]) + (a.logw ? (double)a.logw[(size_t)k * a.set.N + n] : 0.0);
      if (!(u > -INFINITY && u < INFINITY)) u = -INFINITY;
      el.w[k] = u;
      umax = fmax(umax, u);
    }
    if (umax == -INFINITY) {
      for (int k = 0; k < K; ++k) { el.w[k] = 0.0; el.c[k] = 0.0; }
      el.logev = -INFINITY;
      el.status = SPAN_CONTRADICTORY;
    } else {
      double sum = 0.0;
      for (int k = 0; k < K; ++k) sum += exp(el.w[k] - umax);
      for (int k = 0; k < K; ++k) {
        const double w = exp(el.w[k] - umax) / sum;
        el.w[k] = w;
        el.c[k] = w > 0.0 ? w / el.za[k] : 0.0;
      }
      el.logev = umax + log(sum) - log((double)K);
      el.status = SPAN_LIVE;
    }
  }
  __syncthreads();
  r.status = el.status;
}

// the mixture's density at the span (i, j) of A: sum_k (w_k / Z_A,k) p_s,k[i] p_e,k[j], the passes in ascending k
__device__ __forceinline__ double mixture_at(const EnsLds& el, int K, int i, int j) {
  double m = 0.0;
  for (int k = 0; k < K; ++k) m += (el.c[k] * (double)el.ps[k][i]) * (double)el.pe[k][j];
  return m;
}

__global__ __launch_bounds__(SPAN_THREADS) void al_ensemble_query_kernel(AlEnsQueryArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ EnsLds el;
  __shared__ QueryStepLds ql;
  const int n = blockIdx.x, t = threadIdx.x, K = a.in.K;
  SpanRow r;
  open_ensemble_row(a.in, n, lds, el, r);
  const int v = r.v;
  const int kind = t >> 8, c = t & 255;       // the marginals: kind 0 holds y_start[c], kind 1 y_end[c] (spanmarg.hip)
  float q = 0.f, g = 0.f, y = 0.f;
  if (r.status == SPAN_LIVE) {
    const ApHull& hull = r.hull;
    const int sbh = min(hull.negR, v) - 1;    // the last end a positive hull allows
    // the partners of frame c within A, as hual_al_span_marginals takes them: they depend on the answers only
    int plo = 0, phi = -1;
    if (a.y_start && kind < 2 && c < v) {
      if (hull.npos > 0) {
        if (kind == 0) { if (c > hull.negL && c <= hull.lo) { plo = hull.hi; phi = sbh; } }
        else if (c >= hull.hi && c < hull.negR) { plo = hull.negL + 1; phi = hull.lo; }
      } else {
        const ApSegment sg = ap_segment(r.aidx, r.apos, r.napn, v, c);
        if (!sg.closed) { plo = kind == 0 ? c : sg.sa; phi = kind == 0 ? sg.sb : c; }
      }
    }
    double qacc = 0.0, yacc = 0.0, ee = 0.0;
    for (int k = 0; k < K; ++k) {
      const double w = el.w[k];
      if (!(w > 0.0)) continue;               // (uniform)
      const float *ps = el.ps[k], *pe = el.pe[k];
      if (t < v) { ql.ls[t] = log2f(ps[t]); ql.le[t] = log2f(pe[t]); }
      QueryStep st;
      query_step(r.aidx, r.apos, r.napn, v, hull, ps, pe, ql, lds.smd, st);
      if (st.status != SPAN_LIVE) continue;   // (uniform; the step's sums are the opening's: a pass with weight is live)
      if (t < v) {                            // q_k(t) as the step forms it, before its rounding to float32
        double num;
        if (hull.npos > 0) num = (t > hull.negL && t < hull.negR) ? ql.cum[0][min(t, hull.lo)] * ql.cum[2][max(t, hull.hi)] : 0.0;
        else num = ql.cum[0][t] * ql.cum[2][t];
        qacc += w * fmin(fmax(num / st.za, 0.0), 1.0);
      }
      const double h = log2(st.za) - st.hs / st.za;
      ee += w * (h > 0.0 ? h : 0.0);
      if (phi >= plo) {
        const float* other = kind == 0 ? pe : ps;
        double sum = 0.0;
        for (int i = plo; i <= phi; ++i) sum += (double)other[i];
        yacc += w * (((double)(kind == 0 ? ps : pe)[c] * sum) / el.za[k]);
      }
    }
    y = (float)yacc;
    if (t < v) {
      q = (float)fmin(fmax(qacc, 0.0), 1.0);
      g = h2_bits(q);
    }
    float best = t < v ? g : -1.0f;
    int bi = t < v ? t : 0x7fffffff;
    wave_best(best, bi);
    if ((t & 63) == 0) { ql.bestv[t >> 6] = best; ql.besti[t >> 6] = bi; }
    // the mixture's entropy: the quad of start i strides over the ends A allows it
    double hs = 0.0;
#ifndef HUAL_ENS_NO_WALK                      // (a measuring build: what the walk costs, scripts/bench_al_ensemble.py)
    const int i = t / AM_QUAD, q4 = t % AM_QUAD;
    auto walk = [&](int sa, int ihi, int jlo, int sb) {
      if (i < sa || i > ihi) return;
      for (int j = max(i, jlo) + q4; j <= sb; j += AM_QUAD) {
        const double m = mixture_at(el, K, i, j);
        if (m > 0.0) hs += m * log2(m);
      }
    };
    if (hull.npos > 0) walk(hull.negL + 1, hull.lo, hull.hi, sbh);
    else for_each_gap(r, [&](int first, int last) { walk(first, last, first, last); });
#endif
    hs = block_reduce<BlockSumD, SPAN_WAVES>(hs, lds.smd);      // (its barriers publish bestv / besti)
    if (t == 0) {
      best_of_waves(ql.bestv, ql.besti, SPAN_WAVES, best, bi);
      const double hm = -hs > 0.0 ? -hs : 0.0;
      const double bald = hm - ee;
      a.query_point[n] = bi;
      a.query_gain[n] = best;
      a.post_entropy[n] = (float)hm;
      a.expected_entropy[n] = (float)ee;
      a.span_bald[n] = bald > 0.0 ? (float)bald : 0.f;
      a.log_evidence[n] = (float)el.logev;
    }
    if (t < K) a.weight[(size_t)n * K + t] = (float)el.w[t];
  } else {
    if (t == 0) {
      a.query_point[n] = -1;
      a.query_gain[n] = -1.0f;
      a.post_entropy[n] = -1.0f;
      a.expected_entropy[n] = -1.0f;
      a.span_bald[n] = -1.0f;
      a.log_evidence[n] = r.status == SPAN_CONTRADICTORY ? -INFINITY : NAN;
    }
    if (t < K) a.weight[(size_t)n * K + t] = 0.f;
  }
  if (t == 0) a.status[n] = r.status == SPAN_LIVE ? 1 : 0;
  // columns [0, T): a live row has T <= 256 and thread t holds frame t - 0 at t >= v; any other row is zeroed up to min(T, ld)
  const bool live = r.status == SPAN_LIVE;
  for_each_column(r, a.in.set.ld, [&](int col) {
    if (a.incl) a.incl[r.row + col] = live ? q : 0.f;
    if (a.gain) a.gain[r.row + col] = live ? g : 0.f;
    if (a.y_start && !live) { a.y_start[r.row + col] = 0.f; a.y_end[r.row + col] = 0.f; }
  });
  if (a.y_start && live && kind < 2 && c < r.T) (kind == 0 ? a.y_start : a.y_end)[r.row + c] = y;
}

__global__ __launch_bounds__(SPAN_THREADS) void al_ensemble_label_kernel(AlEnsLabelArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ EnsLds el;
  __shared__ double inv[257];               // inv[d] = 1 / d, 1 <= d <= 256
  __shared__ double xh[2][256], xg[2][256]; // p_s[l] H_e[l] | p_s[l] G_e[l] of the current (e, pass), two buffers in turn
  __shared__ double bestv[SPAN_WAVES];
  __shared__ int besti[SPAN_WAVES];
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x, K = a.in.K;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  if (t >= 1 && t <= 256) inv[t] = 1.0 / (double)t;      // (the opening's barriers publish it)
  SpanRow r;
  open_ensemble_row(a.in, n, lds, el, r);
  if (r.status == SPAN_LIVE) {
    const ApHull& hull = r.hull;
    const int v = r.v;
    const int sbh = min(hull.negR, v) - 1;  // the last end a positive hull allows
    const int g = t / AM_QUAD, q = t % AM_QUAD;
    double best = -1.0;
    int bi = 0x7fffffff;
    int step = 0;                           // (uniform) which of the two xh / xg buffers the next publication takes
    // the candidates (g, e) of one region: R = sum_k (w_k / Z_A,k) F_k(g, e), the passes in ascending k; one barrier per (e, pass) - a
    // buffer is rewritten two steps after it was read
    auto region = [&](int sa, int ihi, int jlo, int sb) {
      const NoisyRegion R{sa, ihi, jlo, sb};
      double H[ENS_MAX_K];                  // H_e[g] of every pass
#pragma unroll
      for (int k = 0; k < ENS_MAX_K; ++k) H[k] = 0.0;
      for (int e = sb; e >= jlo; --e) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < ENS_MAX_K; ++k) {
          if (k >= K) break;
          const double ck = el.c[k];
          if (!(ck > 0.0)) continue;        // (uniform)
          const float *ps = el.ps[k], *pe = el.pe[k];
          double* bh = xh[step & 1];
          double* bg = xg[step & 1];
          ++step;
          double G;
          region_publish(R, e, g, q, H[k], ps, pe, bh, bg, G);
          __syncthreads();
          acc += ck * region_mass(R, e, g, q, H[k], G, ps, inv, bh, bg);
          region_advance(R, e, g, pe, inv, H[k]);
        }
        if (g >= sa && g <= min(ihi, e) && acc >= best) { best = acc; bi = g * 256 + e; }      // e descends: the smallest e stays
      }
    };
    if (hull.npos > 0) region(hull.negL + 1, hull.lo, hull.hi, sbh);
    else for_each_gap(r, [&](int first, int last) { region(first, last, first, last); });
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
      // R of the old span by one walk over A under the mixture: the quad of start g takes the ends its region allows
      const int oa = a.old_idx[2 * n], oe = a.old_idx[2 * n + 1];
      const bool valid = oa >= 0 && oa <= oe && oe < v;      // (uniform)
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
          acc += mixture_at(el, K, g, j) * ((double)inter / (double)uni);
        }
      }
      acc = block_reduce<BlockSumD, SPAN_WAVES>(acc, lds.smd);
      if (t == 0) a.old_conf[n] = valid ? (float)fmin(fmax(acc, 0.0), 1.0) : -1.0f;
    }
  } else if (t == 0) {
    a.new_idx[2 * n] = -1;
    a.new_idx[2 * n + 1] = -1;
    a.conf[n] = -1.0f;
    if (a.old_conf) a.old_conf[n] = -1.0f;
  }
}

// the requirements both launches share, under the entry point's prefix `who`; `own`: the launch's own, checked between the null inputs
// and the ranges as check_span_in orders them
template <class Own>
int check_ens_in(const AlEnsIn& in, const char* who, Own own) {
  AlSpanIn si;
  si.set = in.set; si.s0 = in.pass_s; si.e0 = in.pass_e;
  return check_span_in(si, who, [&] {
    if (const int rc = own()) return rc;
    HUAL_REQUIRE(in.K >= 1 && in.K <= ENS_MAX_K, std::string(who) + ": 1 <= K <= 16");
    return 0;
  });
}

int launch_al_ensemble_query(const AlEnsQueryArgs& a, hipStream_t s) {
  const int rc = check_ens_in(a.in, "al_ensemble_query", [&] {
    HUAL_REQUIRE(a.weight && a.log_evidence && a.query_point && a.query_gain && a.post_entropy && a.expected_entropy && a.span_bald &&
                     a.status,
                 "al_ensemble_query: null output");
    HUAL_REQUIRE(!a.y_start == !a.y_end, "al_ensemble_query: y_start and y_end are both set or both null");
    return 0;
  });
  if (rc) return rc;
  const hual_al_set& set = a.in.set;
  // per frame: two logits per pass in, q, its gain and the two marginals out
  HUAL_LAUNCH(0.0, (8.0 * a.in.K + (a.incl ? 4.0 : 0.0) + (a.gain ? 4.0 : 0.0) + (a.y_start ? 8.0 : 0.0)) * set.N * set.ld +
                       (32.0 + 4.0 * a.in.K) * set.N,
              al_ensemble_query_kernel, dim3(set.N), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_al_ensemble_label(const AlEnsLabelArgs& a, int nsel, hipStream_t s) {
  const int rc = check_ens_in(a.in, "al_ensemble_label", [&] {
    HUAL_REQUIRE(a.new_idx && a.conf, "al_ensemble_label: null output");
    HUAL_REQUIRE(!a.old_idx == !a.old_conf, "al_ensemble_label: old_idx and old_conf are both set or both null");
    HUAL_REQUIRE(nsel >= 1, "al_ensemble_label: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits per pass in, the label and its value out (and the old span in, its value out)
  HUAL_LAUNCH(0.0, (8.0 * a.in.K * a.in.set.ld + 12.0 + (a.old_idx ? 12.0 : 0.0) + (a.sel ? 4.0 : 0.0)) * grid, al_ensemble_label_kernel,
              dim3(grid), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int hual_al_ensemble_query(const hual_al_set* set, const float* pass_s, const float* pass_e, int K, const float* logw,
                                      float* weight, float* log_evidence, float* incl, float* gain, int32_t* query_point,
                                      float* query_gain, float* y_start, float* y_end, float* post_entropy, float* expected_entropy,
                                      float* span_bald, int32_t* status, void* stream) {
  HUAL_REQUIRE(set, "hual_al_ensemble_query: null set");
  AlEnsQueryArgs a{};
  a.in.set = *set; a.in.pass_s = pass_s; a.in.pass_e = pass_e; a.in.K = K; a.in.logw = logw;
  a.weight = weight; a.log_evidence = log_evidence; a.incl = incl; a.gain = gain; a.query_point = query_point; a.query_gain = query_gain;
  a.y_start = y_start; a.y_end = y_end; a.post_entropy = post_entropy; a.expected_entropy = expected_entropy; a.span_bald = span_bald;
  a.status = status;
  return launch_al_ensemble_query(a, (hipStream_t)stream);
}

extern "C" int hual_al_ensemble_label(const hual_al_set* set, const float* pass_s, const float* pass_e, int K, const float* logw,
                                      const int32_t* sel, int nsel, const int32_t* old_idx, int32_t* new_idx, float* conf,
                                      float* old_conf, void* stream) {
  HUAL_REQUIRE(set, "hual_al_ensemble_label: null set");
  AlEnsLabelArgs a{};
  a.in.set = *set; a.in.pass_s = pass_s; a.in.pass_e = pass_e; a.in.K = K; a.in.logw = logw;
  a.sel = sel; a.old_idx = old_idx; a.new_idx = new_idx; a.conf = conf; a.old_conf = old_conf;
  return launch_al_ensemble_label(a, nsel, (hipStream_t)stream);
}
