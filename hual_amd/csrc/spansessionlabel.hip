// hual_al_session_label (include/hual_seqpan.h): an annotation session per clip that knows what the annotation is for.  Every pass of
// hual_al_session (spansession.h: the posterior on the list so far, the frame of most information gain) is followed by the pseudo-label
// that list gives - hual_al_mbr_label's span of maximal expected tIoU - and by the label's reliability - hual_al_hit_label's chance
// that it counts as a hit at up to 4 exact rational IoU thresholds - and the session may stop as soon as that chance reaches stop_hit:
// "ask until the label is safe at IoU 0.7 with probability 0.9".  One 1024-thread workgroup per selected sample, the list, the
// transcript and the label trail in LDS.  Not in the train step.
//
// Nothing here is arithmetic of its own.  Per pass:
//  - the posterior and the question: session_pass (spansession.h), the body hual_al_session runs;
//  - the label: spanmbr.h's label_region over the regions of the consistent set of the list so far - one region around a positive
//    hull, one per gap without a positive, the whole triangle under noise (the answers are in the tilted rows) - reduced with
//    wave_best / best_of_waves as al_mbr_label_kernel does;
//  - its hit mass: spanmass.h's sh_mass_within, one wave per threshold, over the float64 prefix sums E of p_e (rebuilt per pass only
//    under noise, where p_e changes) and the interval of ends elo / ehi that the list allows each start, as al_hit_label_kernel does;
//  - the divisor of both: query_step's Z_A, which is posterior_masses' Z_A bit for bit (the same terms, the same wave and workgroup
//    folds: block.h's reductions of two and of three values fold each value alike).
// So every stored value equals what the launches it replaces store: hual_al_noisy_tilt (under noise), hual_al_query,
// hual_al_mbr_label and hual_al_hit_label per pass, with a read-back and an append on the host between them.
//
// The stop rule reads the float32 that is stored, so a host loop reproduces every decision from the outputs.  Barrier discipline is
// hual_al_session's: thread 0 alone decides, and no thread-dependent exit lies between two barriers.  No atomics, nothing grid wide.
#include "prof.h"
#include "spanmass.h"
#include "spanmbr.h"
#include "spansession.h"

#include <cmath>

using namespace hual;

namespace {

struct SessionLabelLds {
  double inv[257];                          // inv[d] = 1 / d, 1 <= d <= 256
  double xh[256], xg[256];                  // label_region's p_s[l] H_e[l] | p_s[l] G_e[l] of the current e
  double E[257];                            // E[x] = sum of p_e[j], j < x
  int ce[SH_MAXM][257], fl[SH_MAXM][257];   // spanmass.h's division tables
  int elo[256], ehi[256];                   // the ends start i may take in A; elo > ehi: none
  double bv[SPAN_WAVES];                    // the waves' best label
  int bk[SPAN_WAVES];
  int32_t lab[SESSION_MAX_Q + 1][2];        // the label trail, unused slots -1
  float conf[SESSION_MAX_Q + 1];
  float hit[SESSION_MAX_Q + 1][SH_MAXM];
};

// 8 waves per SIMD: 64 VGPRs, so that two workgroups share a CU as al_mbr_label_kernel's do - label_region is a chain of short steps
// between barriers, which a second resident workgroup fills.  The session's pass then spills (440 bytes of scratch per lane), and the
// launch is still 3 to 27 % faster than at the 128 VGPRs a 1024-thread workgroup may have; the bits do not depend on it.
__global__ __launch_bounds__(SPAN_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void al_session_label_kernel(AlSessionLabelArgs b) {
  __shared__ SpanRowLds lds;
  __shared__ QueryStepLds ql;
  __shared__ SessionLds ss;
  __shared__ SessionLabelLds ll;
  const AlSessionArgs& a = b.s;
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  const int qmax = a.qmax, M = b.M;
  const int cap = session_cap(a, n);
  const int napn0 = a.in.set.ap_off[n + 1] - a.in.set.ap_off[n];
  if (t >= 1 && t <= 256) ll.inv[t] = 1.0 / (double)t;
  if (t <= qmax) { ll.lab[t][0] = -1; ll.lab[t][1] = -1; ll.conf[t] = -1.0f; }
  if (t < (qmax + 1) * SH_MAXM) ll.hit[t / SH_MAXM][t % SH_MAXM] = -1.0f;
  sh_build_tables(b.num, b.den, M, ll.ce, ll.fl);
  SpanRow r;
  float zs, ze;                             // this thread's untilted logits
  int reason = session_begin(a, n, cap, lds, ql, ss, r, zs, ze), k = 0;      // (uniform) why the session ended | the questions asked so far
  const int v = r.v;
  bool sums = false;                        // (uniform) E holds the prefix sums of the current p_e
  __syncthreads();                          // the list, the fills, the tables (and, under the hard rule, ls / le) are in LDS
  while (reason < 0) {                      // (uniform: `reason` is read from LDS behind a barrier at the end of every pass)
    const int napn = napn0 + k;
    QueryStep st;
    int nread;
    const int status = session_pass(a, r, napn, zs, ze, lds, ql, ss, nread, st);
    if (status == SPAN_LIVE) {              // (uniform)
      const float *ps = lds.ps, *pe = lds.pe;
      if (t < v) ss.qv[t] = st.q;
      // ---- the label of this pass: al_mbr_label_kernel's walk over the regions of the list so far
      const ApHull hull = ap_hull(ss.idx, ss.pos, nread, v);
      const int sbh = min(hull.negR, v) - 1;               // the last end a positive hull allows
      const double za = st.za;
      SpanRow lr;                           // the list as for_each_gap reads it
      lr.v = v; lr.napn = nread; lr.aidx = ss.idx; lr.apos = ss.pos;
      double best = -1.0;
      int bi = 0x7fffffff;
      if (hull.npos > 0)
        label_region(hull.negL + 1, hull.lo, hull.hi, sbh, ps, pe, ll.inv, ll.xh, ll.xg, za, best, bi);
      else
        for_each_gap(lr, [&](int first, int last) { label_region(first, last, first, last, ps, pe, ll.inv, ll.xh, ll.xg, za, best, bi); });
      wave_best(best, bi);
      if (lane == 0) { ll.bv[w] = best; ll.bk[w] = bi; }
      // ---- what its reliability reads: al_hit_label_kernel's prefix sums and intervals of ends
      if (!sums || a.noisy) {
        if (t <= v) {    // each one serial sum in ascending order (spanhit.hip's)
          double s = 0.0;
          for (int j = 0; j < t; ++j) s += (double)pe[j];
          ll.E[t] = s;
        }
        sums = true;
      }
      if (t < v) {
        int jl = 256, jh = -1;
        if (hull.npos > 0) {
          if (t > hull.negL && t <= hull.lo) { jl = hull.hi; jh = sbh; }
        } else {
          const ApSegment sg = ap_segment(ss.idx, ss.pos, nread, v, t);
          if (!sg.closed) { jl = t; jh = sg.sb; }
        }
        ll.elo[t] = jl; ll.ehi[t] = jh;
      }
      __syncthreads();
      best_of_waves(ll.bv, ll.bk, SPAN_WAVES, best, bi);   // (every thread: the label is the candidate of the hit mass)
      const int la = bi >> 8, lb = bi & 255;
      if (w < M) {                          // one wave per threshold
        float val = -1.0f;
        if (la >= 0 && la <= lb && lb < v) {
          double acc = sh_mass_within(la, lb, v, ps, ll.E, ll.ce[w], ll.fl[w], ll.elo, ll.ehi, lane, 64);
          acc = wave_sum64_f64(acc);
          val = (float)fmin(1.0, fmax(0.0, acc / za));
        }
        if (lane == 0) ll.hit[k][w] = val;
      }
      if (t == 0) { ll.lab[k][0] = la; ll.lab[k][1] = lb; ll.conf[k] = (float)fmin(fmax(best, 0.0), 1.0); }
    }
    __syncthreads();
    if (t == 0) {
      int why = -1, bi = -1;
      float best = -1.0f, ent = -1.0f;
      if (status == SPAN_POISONED) {
        why = HUAL_AL_STOP_POISONED;
      } else if (status == SPAN_CONTRADICTORY) {
        why = HUAL_AL_STOP_CONTRADICTORY;
      } else {
        query_step_best(ql, st, bi, best, ent);
        if (b.stop_hit >= 0.f && ll.hit[k][b.stop_m] >= b.stop_hit) why = HUAL_AL_STOP_RELIABLE;      // the float32 that is stored
        else why = session_stop_bits(a, ent, best, bi, k, cap, v);
      }
      ss.entropy[k] = ent;                  // (k <= cap <= qmax: the pass after the last question fills the last slot)
      if (why < 0) session_ask(a, n, k, napn, bi, best, ss);
      ss.reason = why;
    }
    __syncthreads();
    reason = ss.reason;
    if (reason < 0) ++k;
  }
  __syncthreads();
  session_store(a, n, k, reason, ss);
  const size_t o = (size_t)n * (qmax + 1);
  if (t < 2 * (qmax + 1)) b.label[2 * o + t] = ll.lab[t >> 1][t & 1];
  if (t <= qmax) b.label_conf[o + t] = ll.conf[t];
  if (t < M * (qmax + 1)) b.label_hit[M * o + t] = ll.hit[t / M][t % M];
}

}  // namespace

namespace hual {

int launch_al_session_label(const AlSessionLabelArgs& b, int nsel, hipStream_t s) {
  const AlSessionArgs& a = b.s;
  const int rc = check_span_in(a.in, "al_session_label", [&] {
    if (const int bad = check_session_args(a, nsel, "al_session_label")) return bad;
    HUAL_REQUIRE(b.label && b.label_conf && b.label_hit, "al_session_label: null output (label, label_conf, label_hit)");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits in, the transcript and the label trail out (12 + 4 M bytes per pass)
  const double bytes = (8.0 * a.in.set.ld + 17.0 * a.qmax + 12.0 + (12.0 + 4.0 * b.M) * (a.qmax + 1)) * grid;
  HUAL_LAUNCH(0.0, bytes, al_session_label_kernel, dim3(grid), dim3(SPAN_THREADS), 0, s, b);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_session_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* gt, const int32_t* sel,
                                     int nsel, int qmax, const int32_t* budget, float stop_entropy, float min_gain, float eps,
                                     const uint32_t* flip, const int32_t* thresholds, int M, int stop_m, float stop_hit, int32_t* asked,
                                     int8_t* answer, float* q_asked, float* gain, float* entropy, int32_t* n_asked, int32_t* stop_reason,
                                     int32_t* label, float* label_conf, float* label_hit, void* stream) {
  HUAL_REQUIRE(set && thresholds, "hual_al_session_label: null pointer (set, thresholds)");
  HUAL_REQUIRE(eps == 0.f || (eps > 0.f && eps <= 0.5f), "hual_al_session_label: eps is 0 (the hard rule) or in (0, 0.5]");
  HUAL_REQUIRE(M >= 1 && M <= SH_MAXM, "hual_al_session_label: 1 <= M <= 4");
  HUAL_REQUIRE(stop_m >= 0 && stop_m < M, "hual_al_session_label: stop_m in [0, M)");
  HUAL_REQUIRE(stop_hit < 0.f || (stop_hit > 0.f && stop_hit <= 1.f), "hual_al_session_label: stop_hit is negative (off) or in (0, 1]");
  AlSessionLabelArgs b{};
  for (int m = 0; m < M; ++m) {
    b.num[m] = thresholds[2 * m]; b.den[m] = thresholds[2 * m + 1];
    HUAL_REQUIRE(b.num[m] >= 1 && b.num[m] <= b.den[m] && b.den[m] <= SH_MAXDEN,
                 "hual_al_session_label: thresholds are (num, den) with 1 <= num <= den <= 1024");
  }
  fill_session_args(b.s, set, s0, e0, gt, sel, qmax, budget, stop_entropy, min_gain, eps, flip, asked, answer, q_asked, gain, entropy,
                    n_asked, stop_reason);
  b.M = M; b.stop_m = stop_m; b.stop_hit = stop_hit;
  b.label = label; b.label_conf = label_conf; b.label_hit = label_hit;
  return launch_al_session_label(b, nsel, (hipStream_t)stream);
}
