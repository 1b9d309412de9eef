// hual_al_session (include/hual_seqpan.h): an annotation session per clip - up to qmax questions, each chosen after the previous
// answer, answered from the ground-truth span - in one launch.  The span posterior conditions on the answers, not on a new forward pass,
// so after the annotator has answered frame t the best next frame is defined by the same logits: one 1024-thread workgroup per
// selected sample, as the rest of the family, loops "open the posterior on the list so far, choose the frame, stop or ask" with the
// list of active points and the transcript in LDS.  Not in the train step.  The parts of the loop - the opening, the pass, the stop
// rules, the append and the store - are spansession.h's, shared with hual_al_session_label (spansessionlabel.hip).
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
#include "spansession.h"

#include <cmath>

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_session_kernel(AlSessionArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ QueryStepLds ql;
  __shared__ SessionLds ss;
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  const int cap = session_cap(a, n);
  const int napn0 = a.in.set.ap_off[n + 1] - a.in.set.ap_off[n];
  SpanRow r;
  float zs, ze;                             // this thread's untilted logits
  int reason = session_begin(a, n, cap, lds, ql, ss, r, zs, ze), k = 0;      // (uniform) why the session ended | the questions asked so far
  const int v = r.v;
  __syncthreads();                          // the list, the transcript's fill (and, under the hard rule, ls / le) are in LDS
  while (reason < 0) {                      // (uniform: `reason` is read from LDS behind a barrier at the end of every pass)
    const int napn = napn0 + k;
    QueryStep st;
    int nread;
    const int status = session_pass(a, r, napn, zs, ze, lds, ql, ss, nread, st);
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
        why = session_stop_bits(a, ent, best, bi, k, cap, v);
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
}

}  // namespace

namespace hual {

int launch_al_session(const AlSessionArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_session", [&] { return check_session_args(a, nsel, "al_session"); });
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
  fill_session_args(a, set, s0, e0, gt, sel, qmax, budget, stop_entropy, min_gain, eps, flip, asked, answer, q_asked, gain, entropy, n_asked,
                    stop_reason);
  return launch_al_session(a, nsel, (hipStream_t)stream);
}
