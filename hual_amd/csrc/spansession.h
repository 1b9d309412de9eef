// The parts of an annotation session that hual_al_session (spansession.hip) and hual_al_session_label (spansessionlabel.hip) share: the
// session's LDS block, the opening before the loop, the posterior of one pass (under noise the tilt of the UNTILTED logits by the whole
// list and the softmax of the tilted rows; then spanstep.h's query_step), the stop rules in bits, the append of an answer and the store
// of the transcript.  One definition each, so that the session with a label trail asks, answers and stops on the same arithmetic as the
// session without one, instruction for instruction.
//
// Every function is called by the whole workgroup with uniform arguments unless it says "one thread".  The loop around them holds
// barriers: thread 0 alone decides, writes the decision to SessionLds::reason, and all threads read that word behind a barrier.
#pragma once
#include "spannoisy.h"
#include "spanstep.h"

#include <cmath>
#include <string>

namespace hual {

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

// (uniform) sample n's cap on the questions of this session
__device__ __forceinline__ int session_cap(const AlSessionArgs& a, int n) {
  return a.budget ? min(max(a.budget[n], 0), a.qmax) : a.qmax;
}

// Before the loop: the transcript's fill, the row's opening, the set's points into the list and - under the hard rule - the log2f rows.
// -> -1, or the reason that ends the session before its first pass; r.v is set either way (0 on a row that was not opened); zs / ze:
// this thread's untilted logits under noise.  The caller's barrier behind it publishes what it wrote.
__device__ __forceinline__ int session_begin(const AlSessionArgs& a, int n, int cap, SpanRowLds& lds, QueryStepLds& ql, SessionLds& ss,
                                             SpanRow& r, float& zs, float& ze) {
  const int t = threadIdx.x, qmax = a.qmax;
  const int ap0 = a.in.set.ap_off[n], napn0 = a.in.set.ap_off[n + 1] - ap0;
  if (t < qmax) { ss.asked[t] = -1; ss.answer[t] = -1; ss.q[t] = -1.0f; ss.gain[t] = -1.0f; }
  if (t <= qmax) ss.entropy[t] = -1.0f;
  int reason = -1;
  r.v = 0;
  if (napn0 < 0 || napn0 + cap > SESSION_MAX_POINTS) {
    reason = HUAL_AL_STOP_OVERFLOW;         // the list would not fit: nothing is asked
  } else {
    open_span_row(a.in, n, lds, r);
    if (r.status != SPAN_LIVE) reason = HUAL_AL_STOP_POISONED;
  }
  const int v = r.v;
  zs = 0.f; ze = 0.f;
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
  return reason;
}

// The posterior of one pass on the list of napn points -> its status; on a LIVE row `st` is query_step's, bestv / besti are written
// with a barrier behind them, and lds.ps / lds.pe are the probabilities the pass read (under noise: of the tilted rows, to be read
// with NO active point - nread is 0 there, napn under the hard rule).
__device__ __forceinline__ int session_pass(const AlSessionArgs& a, const SpanRow& r, int napn, float zs, float ze, SpanRowLds& lds,
                                            QueryStepLds& ql, SessionLds& ss, int& nread, QueryStep& st) {
  const int t = threadIdx.x, v = r.v;
  int status = SPAN_LIVE;
  if (a.noisy) {
    int gm = 0, g = 0;                      // G(t - 1) | G(t) over the whole list
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
  nread = a.noisy ? 0 : napn;               // the answers are in the tilted rows: the row is read with no active point
  if (status == SPAN_LIVE) {
    const ApHull hull = ap_hull(ss.idx, ss.pos, nread, v);
    query_step(ss.idx, ss.pos, nread, v, hull, lds.ps, lds.pe, ql, lds.smd, st);
    status = st.status;
  }
  return status;
}

// (one thread, a LIVE pass) the stop rules in bits, in the contract's order -> the reason, or -1: ask
__device__ __forceinline__ int session_stop_bits(const AlSessionArgs& a, float ent, float best, int bi, int k, int cap, int v) {
  if (a.stop_entropy >= 0.f && ent <= a.stop_entropy) return HUAL_AL_STOP_ENTROPY;
  if (!(best > a.min_gain)) return HUAL_AL_STOP_GAIN;
  if (k >= cap) return HUAL_AL_STOP_BUDGET;
  if (bi < 0 || bi >= v) return HUAL_AL_STOP_GAIN;      // (never on a live row: the list and qv are indexed by it)
  return -1;
}

// (one thread) question k at frame bi: answered from gt XOR the flip bit, recorded and appended to the list of napn points.
// k < cap, bi in [0, v), napn < napn0 + cap <= SESSION_MAX_POINTS
__device__ __forceinline__ void session_ask(const AlSessionArgs& a, int n, int k, int napn, int bi, float best, SessionLds& ss) {
  const bool truth = a.gt[2 * (size_t)n] <= bi && bi <= a.gt[2 * (size_t)n + 1];
  const bool ans = truth != (bool)(((a.flip ? a.flip[n] : 0u) >> k) & 1u);
  ss.asked[k] = bi; ss.answer[k] = ans ? 1 : 0; ss.q[k] = ss.qv[bi]; ss.gain[k] = best;
  ss.idx[napn] = bi; ss.pos[napn] = ans ? 1 : 0;
}

// the seven outputs of a session, behind the barrier that follows the loop
__device__ __forceinline__ void session_store(const AlSessionArgs& a, int n, int k, int reason, const SessionLds& ss) {
  const int t = threadIdx.x, qmax = a.qmax;
  const size_t o = (size_t)n * qmax;
  if (t < qmax) { a.asked[o + t] = ss.asked[t]; a.answer[o + t] = ss.answer[t]; a.q_asked[o + t] = ss.q[t]; a.gain[o + t] = ss.gain[t]; }
  if (t <= qmax) a.entropy[(size_t)n * (qmax + 1) + t] = ss.entropy[t];
  if (t == 0) { a.n_asked[n] = k; a.stop_reason[n] = reason; }
}

// the argument rules of a session launch, under the entry point's prefix `who` (check_span_in's `own`)
inline int check_session_args(const AlSessionArgs& a, int nsel, const std::string& who) {
  HUAL_REQUIRE(a.gt, who + ": null gt");
  HUAL_REQUIRE(a.asked && a.answer && a.q_asked && a.gain && a.entropy && a.n_asked && a.stop_reason, who + ": null output");
  HUAL_REQUIRE(!a.sel || nsel >= 1, who + ": nsel >= 1");
  HUAL_REQUIRE(a.qmax >= 1 && a.qmax <= SESSION_MAX_Q, who + ": qmax in [1, 16]");
  HUAL_REQUIRE(a.min_gain >= 0.f, who + ": min_gain >= 0");
  return 0;
}

// the arguments both entry points fill alike; eps is checked by the caller
inline void fill_session_args(AlSessionArgs& a, const hual_al_set* set, const float* s0, const float* e0, const int32_t* gt,
                              const int32_t* sel, int qmax, const int32_t* budget, float stop_entropy, float min_gain, float eps,
                              const uint32_t* flip, int32_t* asked, int8_t* answer, float* q_asked, float* gain, float* entropy,
                              int32_t* n_asked, int32_t* stop_reason) {
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.gt = gt; a.sel = sel; a.qmax = qmax; a.budget = budget; a.stop_entropy = stop_entropy; a.min_gain = min_gain;
  a.noisy = eps > 0.f;
  if (a.noisy) {
    const double de = (double)eps;
    a.lam = (float)std::log((1.0 - de) / de);      // hual_al_noisy_tilt's
  }
  a.flip = flip;
  a.asked = asked; a.answer = answer; a.q_asked = q_asked; a.gain = gain; a.entropy = entropy; a.n_asked = n_asked; a.stop_reason = stop_reason;
}

}  // namespace hual
