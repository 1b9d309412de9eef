// Active-learning label update kernels (see al.hip).
#pragma once
#include "common.h"

#define HUAL_AL_MAX_T 1024

namespace hual {

// which of AlScoreArgs' sources the model-uncertainty term of a launch is read from
enum AlSource {
  AL_SRC_PAIR,                                // hual_al_score: the two stochastic passes' logits
  AL_SRC_SPREAD,                              // hual_al_score_mc: the bank's min / max / sum of squared deviations
  AL_SRC_INFO,                                // hual_al_score_info: the bank's mean and the mean entropy of the passes beside it
};

struct AlScoreArgs {
  hual_al_set set;                            // N, ld | vlen [N] valid frames | tlen [N] length of the logits record | the active points (CSR)
  const float *s0, *e0;                       // [N, ld] start / end logits of the deterministic pass
  float coff_uncert;
  // the source of the model-uncertainty term: a launch reads the fields of its AlSource, the others stay null
  const float *s1, *e1, *s2, *e2;             // PAIR: [N, ld] logits of the two stochastic passes
  const float *lo[2], *hi[2], *mean[2], *m2[2];   // SPREAD, INFO: [N, ld] per head (0 = start, 1 = end), the bank (hual_al_bank)
  const float* ent[2];                        // INFO: [N, ld] per head, mean entropy of the passes (hual_al_info)
  int stat;                                   // SPREAD: HUAL_AL_STAT_RANGE / _STD; INFO: HUAL_AL_STAT_BALD / _ENTROPY / _EXPECTED_ENTROPY
  float km1;                                  // SPREAD: (float)(K - 1)
  float* uncert_model;                        // SPREAD, INFO: [N, ld] the model-uncertainty term itself (NULL: not written)
  float* sprob;                               // [N, ld]
  float* eprob;                               // [N, ld]
  double* uncert_frame;                       // [N, ld]
  float* uncert_video;                        // [N]
  int32_t* observe;                           // [N] argmax of uncert_frame
};

// hual_al_mc_fold / hual_al_mc_fold_info: one forward's logits [B, T] folded into the rows ids[b] of the bank
struct AlFoldArgs {
  const int32_t* ids;                         // [B] bank rows
  const int32_t* vlen;                        // [B] valid frames of each clip
  const float *s, *e;                         // [B, T] start / end logits
  int B, T, k;                                // k = 0: deterministic pass, 1..K: stochastic passes
  int ld, N;
  int32_t* tlen;                              // [N]
  float *s0, *e0;                             // [N, ld]
  float *lo[2], *hi[2], *mean[2], *m2[2];     // [N, ld] per head (0 = start, 1 = end)
  float* ent[2];                              // [N, ld] per head: mean over the stochastic passes of h2(p_k), in bits (NULL: a plain fold)
};

struct AlRenewArgs {
  const int32_t* sel;                         // [nsel] sample ids to update (NULL: all)
  const float* sprob;
  const float* eprob;
  hual_al_set set;
  const int32_t* old_idx;                     // [N, 2]
  double coff[6];                             // pos.distance, pos.model, pos.old, neg.distance, neg.model, neg.old
  int32_t* new_idx;                           // [N, 2] (rows of unselected samples are left untouched)
};

// what every span-posterior launch reads (spanpost.h opens a row from it): the set and the deterministic pass
struct AlSpanIn {
  hual_al_set set;
  const float *s0, *e0;                       // [N, ld] start / end logits
};

// hual_al_query (spanquery.hip): the posterior over spans given the answered active points, and the frame whose answer carries most information
struct AlQueryArgs {
  AlSpanIn in;
  float *incl, *gain;                         // [N, ld] q(t) and h2(q(t)) in bits, columns [0, tlen[n]) (NULL, both: not written)
  int32_t* query_point;                       // [N] first frame of maximal gain
  float *query_gain, *post_entropy, *agree;   // [N]
};

// hual_al_mbr_label (spanlabel.hip): the span of the consistent set of maximal expected tIoU under the answered-point posterior
struct AlLabelArgs {
  AlSpanIn in;
  const int32_t* sel;                         // [nsel] sample ids to label (NULL: all)
  const int32_t* old_idx;                     // [N, 2] (NULL with old_conf: not scored)
  int32_t* new_idx;                           // [N, 2] (rows of unselected samples are left untouched, as conf and old_conf)
  float *conf, *old_conf;                     // [N]
};

// hual_al_hit_label (spanhitlabel.hip): the hit probability of given spans under the answered-point posterior, and per IoU threshold
// the member of the consistent set of maximal hit probability
struct AlHitArgs {
  AlSpanIn in;
  const int32_t* sel;                         // [nsel] sample ids (NULL: all)
  int num[4], den[4];                         // the thresholds, read on the host before the launch
  int M, k;                                   // 1..4 thresholds | 0..16 candidate slots per sample
  const int32_t* cand_idx;                    // [N, k, 2] (NULL with k == 0)
  float* cand_hit;                            // [N, k, M] (rows of unselected samples are left untouched, as best_idx and best_prob)
  int32_t* best_idx;                          // [N, M, 2] (NULL with best_prob: no search)
  float* best_prob;                           // [N, M]
};

// hual_al_label_gain (spangain.hip): per frame, the tIoU the label of hual_al_mbr_label is expected to gain from the frame's answer
struct AlGainArgs {
  AlSpanIn in;
  const int32_t* sel;                         // [nsel] sample ids to evaluate (NULL: all)
  const int32_t* cand;                        // [N, M] the frames to evaluate, entries outside [0, v) skipped (NULL: every frame)
  int M;
  float* gain;                                // [N, ld] columns [0, tlen[n]) (NULL: not written)
  int32_t* ask_point;                         // [N] first evaluated frame of maximal gain (rows of unselected samples are left untouched)
  float *ask_gain, *value;                    // [N] that gain | V0, the conf of hual_al_mbr_label on the same set
};

// hual_al_span_marginals (spanmarg.hip): the start / end marginals of the span posterior given the answered active points
struct AlMargArgs {
  AlSpanIn in;
  float *y_start, *y_end;                     // [N, ld] columns [0, tlen[n])
  int32_t* status;                            // [N] 1 = live, 0 = poisoned or contradictory
};

// hual_al_session (spansession.hip): several adaptive questions per selected sample, answered from the ground truth, in one launch
struct AlSessionArgs {
  AlSpanIn in;                                // the set with the answers of earlier rounds, the UNTILTED logits
  const int32_t* gt;                          // [N, 2] the ground-truth frame span: the simulated annotator
  const int32_t* sel;                         // [nsel] sample ids (NULL: all)
  int qmax;                                   // 1..16 question slots per sample
  const int32_t* budget;                      // [N] per-sample cap, clamped to [0, qmax] (NULL: qmax)
  float stop_entropy, min_gain;               // bits; stop_entropy < 0: off
  bool noisy;                                 // eps > 0: the noisy annotator's posterior (spannoisy.h) instead of the hard rule
  float lam;                                  // (float)ln((1 - eps) / eps) under noisy
  const uint32_t* flip;                       // [N] bit k flips the k-th answer of the session (NULL: none)
  int32_t* asked;                             // [N, qmax]
  int8_t* answer;                             // [N, qmax]
  float *q_asked, *gain;                      // [N, qmax]
  float* entropy;                             // [N, qmax + 1]
  int32_t *n_asked, *stop_reason;             // [N]
};

// hual_al_session_label (spansessionlabel.hip): a session that also keeps, per pass, the MBR label of the list so far and its hit
// probability, and may stop on the latter
struct AlSessionLabelArgs {
  AlSessionArgs s;                            // the session's own arguments and its seven outputs
  int num[4], den[4];                         // the IoU thresholds, read on the host before the launch
  int M, stop_m;                              // 1..4 thresholds | the column the stop rule reads
  float stop_hit;                             // < 0: off; else the session stops once (float)label_hit[stop_m] >= stop_hit
  int32_t* label;                             // [N, qmax + 1, 2] slot k: the label of the pass before question k; -1: unused / not live
  float* label_conf;                          // [N, qmax + 1]
  float* label_hit;                           // [N, qmax + 1, M]
};

// hual_al_design (spandesign.hip): the frames to ask TOGETHER about every selected sample - a greedy design under the span posterior
struct AlDesignArgs {
  AlSpanIn in;
  const int32_t* sel;                         // [nsel] sample ids (NULL: all)
  int mmax;                                   // 1..16 frames per sample
  const int32_t* forced;                      // [N, mmax] the leading entries >= 0: the design's first frames; -1 ends them (NULL: none)
  float min_gain, stop_entropy;               // bits; stop_entropy < 0: off
  int32_t* frames;                            // [N, mmax] in the order chosen, unused slots -1
  float* info;                                // [N, mmax] I(t_1 .. t_{m+1}) in bits, unused slots -1
  float* post_entropy;                        // [N] hual_al_query's
  int32_t *n_design, *stop_reason;            // [N]
};

// the null and N / ld requirements of an AlSpanIn, refused under the entry point's prefix `who`; between the two, in the order the
// launches have always checked in, the launch's own requirements (`own`: null outputs, nsel, ... - returns 0 or the failure)
template <class Own>
int check_span_in(const AlSpanIn& in, const char* who, Own own) {
  const hual_al_set& s = in.set;
  HUAL_REQUIRE(in.s0 && in.e0 && s.vlen && s.tlen && s.ap_off && s.ap_idx && s.ap_pos, std::string(who) + ": null input");
  if (const int rc = own()) return rc;
  HUAL_REQUIRE(s.N > 0 && s.ld >= 2 && s.ld <= HUAL_AL_MAX_T, std::string(who) + ": need N > 0 and 2 <= ld <= 1024");
  return 0;
}

int launch_al_score(const AlScoreArgs& a, AlSource src, hipStream_t s);
int launch_al_span_marginals(const AlMargArgs& a, hipStream_t s);
int launch_al_label_gain(const AlGainArgs& a, int nsel, hipStream_t s);
int launch_al_mbr_label(const AlLabelArgs& a, int nsel, hipStream_t s);
int launch_al_hit_label(const AlHitArgs& a, int nsel, hipStream_t s);
int launch_al_query(const AlQueryArgs& a, hipStream_t s);
int launch_al_session(const AlSessionArgs& a, int nsel, hipStream_t s);
int launch_al_session_label(const AlSessionLabelArgs& a, int nsel, hipStream_t s);
int launch_al_design(const AlDesignArgs& a, int nsel, hipStream_t s);
int launch_al_mc_fold(const AlFoldArgs& a, hipStream_t s);
int launch_al_renew(const AlRenewArgs& a, int nsel, hipStream_t s);

// binary entropy in bits, every operation rounded on its own (tests/mc_info_ref.py is its float64 yardstick).  The fold, the score and the
// query evaluate this one function: K identical passes leave mean == p and ent == h2(p), and BALD = h2(mean) - ent is then exactly 0.
__device__ __forceinline__ float h2_bits(float p) {
#pragma clang fp contract(off)
  if (p <= 0.0f || p >= 1.0f) return 0.0f;
  const float q = 1.0f - p;
  const float a = p * log2f(p);
  const float b = q * log2f(q);
  return -(a + b);
}

}  // namespace hual
