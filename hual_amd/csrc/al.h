// Active-learning label update kernels (see al.hip).
#pragma once
#include <type_traits>
#include "common.h"

#define HUAL_AL_MAX_T 1024

namespace hual {

struct AlScoreArgs {
  const float *s0, *e0, *s1, *e1, *s2, *e2;   // [N, ld] start / end logits: deterministic pass, two stochastic passes
  int ld, N;
  const int32_t* vlen;                        // [N] valid frames
  const int32_t* tlen;                        // [N] length of the logits record (padded length of its batch)
  const int32_t* ap_off;                      // [N+1] CSR offsets of the active points
  const int32_t* ap_idx;                      // frame index of each active point
  const int8_t* ap_pos;                       // 1 = inside the ground-truth span, 0 = outside
  float coff_uncert;
  float* sprob;                               // [N, ld]
  float* eprob;                               // [N, ld]
  double* uncert_frame;                       // [N, ld]
  float* uncert_video;                        // [N]
  int32_t* observe;                           // [N] argmax of uncert_frame
};

// hual_al_score_mc: the same scoring with the model-uncertainty term read from the per-sample bank of K folded passes
// (the fields al_score_body reads carry the names of AlScoreArgs)
struct AlScoreMcArgs {
  const float *s0, *e0;                       // [N, ld] deterministic logits
  const float *lo_s, *hi_s, *m2_s;            // [N, ld] start head: min / max probability, sum of squared deviations
  const float *lo_e, *hi_e, *m2_e;            // [N, ld] end head
  int ld, N;
  const int32_t* vlen;
  const int32_t* tlen;
  const int32_t* ap_off;
  const int32_t* ap_idx;
  const int8_t* ap_pos;
  float coff_uncert;
  int stat;                                   // HUAL_AL_STAT_RANGE / HUAL_AL_STAT_STD
  float km1;                                  // (float)(K - 1)
  float* sprob;
  float* eprob;
  double* uncert_frame;
  float* uncert_video;
  int32_t* observe;
  float* uncert_model;                        // [N, ld] the model-uncertainty term itself (NULL: not written)
};

// hual_al_mc_fold: one forward's logits [B, T] folded into the rows ids[b] of the bank
struct AlFoldArgs {
  const int32_t* ids;                         // [B] bank rows
  const int32_t* vlen;                        // [B] valid frames of each clip
  const float *s, *e;                         // [B, T] start / end logits
  int B, T, k;                                // k = 0: deterministic pass, 1..K: stochastic passes
  int ld, N;
  int32_t* tlen;                              // [N]
  float *s0, *e0;                             // [N, ld]
  float *lo[2], *hi[2], *mean[2], *m2[2];     // [N, ld] per head (0 = start, 1 = end)
};

// hual_al_mc_fold_info: the same fold plus the running mean of the per-pass binary entropy (the existing arguments keep their offsets)
struct AlFoldInfoArgs : AlFoldArgs {
  float* ent[2];                              // [N, ld] per head: mean over the stochastic passes of h2(p_k), in bits
};

// hual_al_score_info: hual_al_score_mc's scoring with an information-theoretic model-uncertainty term (the fields al_score_kernel
// reads carry the names of AlScoreArgs)
struct AlScoreInfoArgs {
  const float *s0, *e0;                       // [N, ld] deterministic logits
  const float *mean_s, *ent_s;                // [N, ld] start head: mean probability, mean entropy of the passes
  const float *mean_e, *ent_e;                // [N, ld] end head
  int ld, N;
  const int32_t* vlen;
  const int32_t* tlen;
  const int32_t* ap_off;
  const int32_t* ap_idx;
  const int8_t* ap_pos;
  float coff_uncert;
  int stat;                                   // HUAL_AL_STAT_BALD / HUAL_AL_STAT_ENTROPY / HUAL_AL_STAT_EXPECTED_ENTROPY
  float* sprob;
  float* eprob;
  double* uncert_frame;
  float* uncert_video;
  int32_t* observe;
  float* uncert_model;                        // [N, ld] the model-uncertainty term itself (NULL: not written)
};

struct AlRenewArgs {
  const int32_t* sel;                         // [nsel] sample ids to update (NULL: all)
  const float* sprob;
  const float* eprob;
  int ld;
  const int32_t* vlen;
  const int32_t* tlen;
  const int32_t* ap_off;
  const int32_t* ap_idx;
  const int8_t* ap_pos;
  const int32_t* old_idx;                     // [N, 2]
  double coff[6];                             // pos.distance, pos.model, pos.old, neg.distance, neg.model, neg.old
  int32_t* new_idx;                           // [N, 2] (rows of unselected samples are left untouched)
};

int launch_al_score(const AlScoreArgs& a, hipStream_t s);
int launch_al_score_mc(const AlScoreMcArgs& a, hipStream_t s);
int launch_al_mc_fold(const AlFoldArgs& a, hipStream_t s);
int launch_al_score_info(const AlScoreInfoArgs& a, hipStream_t s);
int launch_al_mc_fold_info(const AlFoldInfoArgs& a, hipStream_t s);
int launch_al_renew(const AlRenewArgs& a, int nsel, hipStream_t s);

}  // namespace hual
