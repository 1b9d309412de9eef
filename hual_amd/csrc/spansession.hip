// hual_al_session (include/hual_seqpan.h): an annotation session per clip - up to qmax questions, each chosen after the previous
// answer, answered from the ground-truth span - in one launch.  The span posterior conditions on the answers, not on a new forward pass,
// so after the annotator has answered frame t the best next frame is defined by the same logits: one 1024-thread workgroup per
// selected sample, as the rest of the family, loops "open the posterior on the list so far, choose the frame, stop or ask" with the
// list of active points and the transcript in LDS.  Not in the train step.
//
// Every step is hual_al_query's arithmetic (spanstep.h's query_step, the body al_query_kernel runs) on the row opening of the family
// (spanpost.h, spanprob.h), so a session's transcript equals the launches it replaces bit for bit:
//  - hard rule (eps == 0): span_probabilities and the log2f rows once, before the loop; per step the hull, the segments and the
//    segmented float64 sums on the grown list.
//  - noisy annotator (eps > 0): per step G is rebuilt from the whole list, tilt_logit (spannoisy.h) is applied to the UNTILTED logits
//    held in registers (never a tilt of a tilt), the softmax is retaken from the tilted rows in LDS and the row is read with no
//    active point - hual_al_noisy_tilt followed by hual_al_query on the set without answers.
//
// The loop holds barriers, so it is left by every thread in the same iteration: thread 0 alone decides, writes the decision to LDS,
// and all threads read that word behind a barrier.  No break or return under a thread-dependent condition lies between two barriers.
#include "prof.h"
#include "spannoisy.h"
#include "spanstep.h"

#include <cmath>

using namespace hual;

namespace {

constexpr int SESSION_MAX_Q = 16;           // question slots per sample
constexpr int SESSION_MAX_POINTS = 64;      // the list in LDS: the set's points plus the session's

struct SessionLds {
  int32_t idx[SESSION_MAX_POINTS];          // the list so far, in annotation order
  int8_t pos[SESSION_MAX_POINTS];
  float ts[256], te[256];                   // the tilted logits of a noisy step
  float qv[256];                            // q(t) of the step, for the thread that records the asked frame's
  int32_t asked[SESSION_MAX_Q];             // the transcript, unused slots -1
  int8_t answer[SESSION_MAX_Q];
  float q[SESSION_MAX_Q], gain[SESSION_MAX_Q], entropy[SESSION_MAX_Q + 1];
  int reason;                               // the step's decision: -1 = asked, go on; else the HUAL_AL_STOP_* that ended the session
};

__global__ __launch_bounds__(SPAN_THREADS) void al_session_kernel(AlSessionArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ QueryStepLds ql;
  __shared__ SessionLds ss;
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  const int qmax = a.qmax;
  const int cap = a.budget ? min(max(a.budget[n], 0), qmax) : qmax;
  const int ap0 = a.in.set.ap_off[n], napn0 = a.in.set.ap_off[n + 1] - ap0;
  if (t < qmax) { ss.asked[t] = -1; ss.answer[t] = -1; ss.q[t] = -1.0f; ss.gain[t] = -1.0f; }
  if (t <= qmax) ss.entropy[t] = -1.0f;
  int reason = -1, k = 0;                   // (uniform) why the session ended | the questions asked so far
  SpanRow r;
  r.v = 0;
  if (napn0 < 0 || napn0 + cap > SESSION_MAX_POINTS) {
    reason = HUAL_AL_STOP_OVERFLOW;         // the list would not fit: nothing is asked
  } else {
    open_span_row(a.in, n, lds, r);
    if (r.status != SPAN_LIVE) reason = HUAL_AL_STOP_POISONED;
  }
  const int v = r.v;
  float zs = 0.f, ze = 0.f;                 // this thread's untilted logits
  if (reason < 0) {
    if (t < napn0) { ss.idx[t] = r.aidx[t]; ss.pos[t] = r.apos[t]; }
    if (a.noisy) {
      if (t < v) { zs = a.in.s0[r.row + t]; ze = a.in.e0[r.row + t]; }
      // hual_al_noisy_tilt's own gate: a Z of the untilted row that is not a positive finite number leaves raw copies, which poison
      double zf, za;
      posterior_masses(nullptr, nullptr, 0, v, ap_hull(nullptr, nullptr, 0, v), lds.ps, lds.pe, lds.smd, zf, za);
      if (posterior_status(zf, zf) != SPAN_LIVE) reason = HUAL_AL_STOP_POISONED;
    } else if (t < v) {
      ql.ls[t] = log2f(lds.ps[t]);
      ql.le[t] = log2f(lds.pe[t]);
    }
  }
  __syncthreads();                          // the list, the transcript's fill (and, under the hard rule, ls / le) are in LDS
  while (reason < 0) {                      // (uniform: `reason` is read from LDS behind a barrier at the end of every pass)
    const int napn = napn0 + k;
    QueryStep st;
    int status = SPAN_LIVE;
    if (a.noisy) {
      int gm = 0, g = 0;                    // G(t - 1) | G(t) over the whole list
      for (int j = 0; j < napn; ++j) {
        const int f = ss.idx[j];
        if (f < 0 || f >= v) continue;
        const int sgn = ss.pos[j] ? 1 : -1;
        if (f <= t) g += sgn;
        if (f < t) gm += sgn;
      }
      if (t < v) {
        ss.ts[t] = a.lam != 0.f ? tilt_logit(zs, -gm, a.lam) : zs;
        ss.te[t] = a.lam != 0.f ? tilt_logit(ze, g, a.lam) : ze;
      }
      // (every thread reads back its own two words; the check's barrier publishes the rows)
      if (span_row_poisoned(ss.ts, ss.te, 0, v)) {
        status = SPAN_POISONED;
      } else {
        span_probabilities(ss.ts, ss.te, 0, r.T, v, lds.ps, lds.pe, lds.smf, lds.smd);
        if (t < v) { ql.ls[t] = log2f(lds.ps[t]); ql.le[t] = log2f(lds.pe[t]); }
      }
    }
    if (status == SPAN_LIVE) {
      const int nread = a.noisy ? 0 : napn; // the answers are in the tilted rows: the row is read with no active point
      const ApHull hull = ap_hull(ss.idx, ss.pos, nread, v);
      query_step(ss.idx, ss.pos, nread, v, hull, lds.ps, lds.pe, ql, lds.smd, st);
      status = st.status;
    }
    if (status == SPAN_LIVE && t < v) ss.qv[t] = st.q;
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
        if (a.stop_entropy >= 0.f && ent <= a.stop_entropy) why = HUAL_AL_STOP_ENTROPY;
        else if (!(best > a.min_gain)) why = HUAL_AL_STOP_GAIN;
        else if (k >= cap) why = HUAL_AL_STOP_BUDGET;
        else if (bi < 0 || bi >= v) why = HUAL_AL_STOP_GAIN;      // (never on a live row: the list and qv are indexed by it)
      }
      ss.entropy[k] = ent;                  // (k <= cap <= qmax: the pass after the last question fills the last slot)
      if (why < 0) {                        // ask: k < cap, bi in [0, v), napn < napn0 + cap <= SESSION_MAX_POINTS
        const bool truth = a.gt[2 * (size_t)n] <= bi && bi <= a.gt[2 * (size_t)n + 1];
        const bool ans = truth != (bool)(((a.flip ? a.flip[n] : 0u) >> k) & 1u);
        ss.asked[k] = bi; ss.answer[k] = ans ? 1 : 0; ss.q[k] = ss.qv[bi]; ss.gain[k] = best;
        ss.idx[napn] = bi; ss.pos[napn] = ans ? 1 : 0;
      }
      ss.reason = why;
    }
    __syncthreads();
    reason = ss.reason;
    if (reason < 0) ++k;
  }
  __syncthreads();
  const size_t o = (size_t)n * qmax;
  if (t < qmax) { a.asked[o + t] = ss.asked[t]; a.answer[o + t] = ss.answer[t]; a.q_asked[o + t] = ss.q[t]; a.gain[o + t] = ss.gain[t]; }
  if (t <= qmax) a.entropy[(size_t)n * (qmax + 1) + t] = ss.entropy[t];
  if (t == 0) { a.n_asked[n] = k; a.stop_reason[n] = reason; }
}

}  // namespace

namespace hual {

int launch_al_session(const AlSessionArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_session", [&] {
    HUAL_REQUIRE(a.gt, "al_session: null gt");
    HUAL_REQUIRE(a.asked && a.answer && a.q_asked && a.gain && a.entropy && a.n_asked && a.stop_reason, "al_session: null output");
    HUAL_REQUIRE(!a.sel || nsel >= 1, "al_session: nsel >= 1");
    HUAL_REQUIRE(a.qmax >= 1 && a.qmax <= SESSION_MAX_Q, "al_session: qmax in [1, 16]");
    HUAL_REQUIRE(a.min_gain >= 0.f, "al_session: min_gain >= 0");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits in, the transcript out (13 bytes per slot, 4 (qmax + 1) of entropies, the two counters)
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + 17.0 * a.qmax + 12.0) * grid, al_session_kernel, dim3(grid), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_session(const hual_al_set* set, const float* s0, const float* e0, const int32_t* gt, const int32_t* sel, int nsel,
                               int qmax, const int32_t* budget, float stop_entropy, float min_gain, float eps, const uint32_t* flip,
                               int32_t* asked, int8_t* answer, float* q_asked, float* gain, float* entropy, int32_t* n_asked,
                               int32_t* stop_reason, void* stream) {
  HUAL_REQUIRE(set, "hual_al_session: null set");
  HUAL_REQUIRE(eps == 0.f || (eps > 0.f && eps <= 0.5f), "hual_al_session: eps is 0 (the hard rule) or in (0, 0.5]");
  AlSessionArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.gt = gt; a.sel = sel; a.qmax = qmax; a.budget = budget; a.stop_entropy = stop_entropy; a.min_gain = min_gain;
  a.noisy = eps > 0.f;
  if (a.noisy) {
    const double de = (double)eps;
    a.lam = (float)std::log((1.0 - de) / de);      // hual_al_noisy_tilt's
  }
  a.flip = flip;
  a.asked = asked; a.answer = answer; a.q_asked = q_asked; a.gain = gain; a.entropy = entropy; a.n_asked = n_asked; a.stop_reason = stop_reason;
  return launch_al_session(a, nsel, (hipStream_t)stream);
}
