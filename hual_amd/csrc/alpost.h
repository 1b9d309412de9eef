// The answered active points of one sample as the span-posterior kernels read them (hual_al_query in al.hip, hual_al_mbr_label in
// spanlabel.hip, hual_al_span_marginals in spanmarg.hip; the contract is in include/hual_seqpan.h): points with a frame index outside [0, v) are ignored, the positives are
// reduced to their hull, the negatives to the nearest one on either side of it or - without a positive - to the gaps between them.
// One definition, so every launch sees the same consistent set A.  hual_al_label_gain (spangain.hip) asks what A would be after one more
// answer: ap_hull and ap_segment take that hypothetical point (hf, hpos) behind the list; hf outside [0, v) - the default - is none.
#pragma once
#include "common.h"

// the positive hull [lo, hi] with the nearest negatives around it (negL = -1 / negR = INT_MAX: none); inside: a negative within the
// hull, which empties A.  npos == 0: no positive inside the clip, the other fields keep their initial values.
struct ApHull {
  int npos, lo, hi, negL, negR;
  bool inside;
};

__device__ __forceinline__ ApHull ap_hull(const int32_t* aidx, const int8_t* apos, int napn, int v, int hf = -1, int hpos = 0) {
  ApHull h;
  h.npos = 0; h.lo = 0x7fffffff; h.hi = -1; h.negL = -1; h.negR = 0x7fffffff; h.inside = false;
  for (int k = 0; k <= napn; ++k) {         // (k == napn: the hypothetical point)
    const int f = k < napn ? aidx[k] : hf;
    if (f < 0 || f >= v || !(k < napn ? apos[k] : hpos)) continue;
    ++h.npos; h.lo = min(h.lo, f); h.hi = max(h.hi, f);
  }
  if (h.npos > 0) {
    for (int k = 0; k <= napn; ++k) {
      const int f = k < napn ? aidx[k] : hf;
      if (f < 0 || f >= v || (k < napn ? apos[k] : hpos)) continue;
      if (f < h.lo) h.negL = max(h.negL, f);
      else if (f > h.hi) h.negR = min(h.negR, f);
      else h.inside = true;
    }
  }
  return h;
}

// frame c's segment [sa, sb]: between the nearest negatives around it; closed: c is itself a negative
struct ApSegment {
  int sa, sb;
  bool closed;
};

__device__ __forceinline__ ApSegment ap_segment(const int32_t* aidx, const int8_t* apos, int napn, int v, int c, int hf = -1,
                                                int hpos = 0) {
  ApSegment s;
  s.sa = 0; s.sb = v - 1; s.closed = false;
  for (int k = 0; k <= napn; ++k) {         // (k == napn: the hypothetical point)
    const int f = k < napn ? aidx[k] : hf;
    if (f < 0 || f >= v || (k < napn ? apos[k] : hpos)) continue;
    if (f < c) s.sa = max(s.sa, f + 1);
    else if (f > c) s.sb = min(s.sb, f - 1);
    else s.closed = true;
  }
  return s;
}
