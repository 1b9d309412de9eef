// The span posterior of one sample given its answered active points, as every launch of the family opens it (hual_al_query in
// spanquery.hip, hual_al_mbr_label in spanlabel.hip, hual_al_label_gain in spangain.hip, hual_al_span_marginals in spanmarg.hip,
// every step of hual_al_session in spansession.hip and of hual_al_session_label in spansessionlabel.hip, hual_al_design in spandesign.hip, every pass of the ensemble launches in
// spanens.hip, hual_al_noisy_tilt in spannoisy.hip, hual_al_hit_label in spanhitlabel.hip, the header of hual_al_evidence_grid in spancalib.hip; the
// contract is in include/hual_seqpan.h): which rows are live, what the consistent set A is, and what Z and Z_A are.  One definition, so
// all launches classify a row alike (tests/test_gpu_span_rows.py); the per-clip launches of the evaluation have theirs in spanclip.h.
//
// The active points: points with a frame index outside [0, v) are ignored, the positives are reduced to their hull, the negatives to the
// nearest one on either side of it or - without a positive - to the gaps between them.  hual_al_label_gain asks what A would be after one
// more answer: ap_hull and ap_segment take that hypothetical point (hf, hpos) behind the list; hf outside [0, v) - the default - is none.
#pragma once
#include "al.h"
#include "spanprob.h"

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

// zf / za <- Z over the whole triangle and Z_A over the consistent set, the sums of al_query_kernel in its order: frame t's share is
// p_e[t] times the sum of p_s over the frames <= t (of its segment); around a positive hull Z_A is the product of its start and end
// masses.  Called by the whole workgroup; smd: 2 * SPAN_WAVES doubles of LDS scratch; its barriers publish what was written before it.
__device__ __forceinline__ void posterior_masses(const int32_t* aidx, const int8_t* apos, int napn, int v, const ApHull& hull,
                                                 const float* ps, const float* pe, double* smd, double& zf, double& za) {
  const int t = threadIdx.x;
  zf = 0.0; za = 0.0;
  if (t < v) {
    const ApSegment sg = ap_segment(aidx, apos, napn, v, t);
    double below = 0.0, seg = 0.0;
    for (int i = 0; i < sg.sa; ++i) below += (double)ps[i];
    for (int i = sg.sa; i <= t; ++i) seg += (double)ps[i];
    zf = (double)pe[t] * (below + seg);
    za = sg.closed ? 0.0 : (double)pe[t] * seg;
  }
  block_reduce<BlockSumD, SPAN_WAVES>(zf, za, smd);
  if (hull.npos > 0) {                      // starts in (negL, lo] x ends in [hi, negR)
    double S = 0.0, E = 0.0;
    for (int i = hull.negL + 1; i <= hull.lo; ++i) S += (double)ps[i];
    for (int j = hull.hi; j < min(hull.negR, v); ++j) E += (double)pe[j];
    za = hull.inside ? 0.0 : S * E;
  }
}

enum SpanRowStatus { SPAN_LIVE, SPAN_POISONED, SPAN_CONTRADICTORY };

// the LDS every kernel of the family holds; its own extras (inv, xh / xg, cum, gs) lie beside it
struct SpanRowLds {
  float ps[256], pe[256];                   // the span distribution's factors (spanprob.h)
  float smf[2 * SPAN_WAVES];                // reduction scratch: the softmax maxima |
  double smd[3 * SPAN_WAVES];               //   up to three float64 sums (the query's Z, Z_A and entropy sum)
};

// one opened row, (uniform) in every field; the kernel declares it and the opening fills it in place.  T, v, row and status are always
// set; the slice and the hull only on a row that stage 1 left LIVE, zf and za only by stage 2 on such a row: READ THEM UNDER
// status == SPAN_LIVE ONLY.  They get no defaults on purpose - a default is merged with the live value where the two paths of a row
// join, the merged values live in VGPRs, and the label kernel then needs 66 of them: one workgroup per CU instead of two
struct SpanRow {
  int T, v;                                 // the row's length as stored | its clipped clip length, 0 on a row that does not fit
  size_t row;                               // offset of the row in an [N, ld] tensor
  int napn;                                 // the sample's active points, in annotation order
  const int32_t* aidx;
  const int8_t* apos;
  ApHull hull;
  double zf, za;                            // Z over the whole triangle | Z_A over the consistent set (open_posterior_row)
  int status;                               // SpanRowStatus
};

// (uniform) every weight underflowed or an infinite logit made them NaN: poisoned, as hual_span_expected_iou; nothing left in A:
// contradictory
__device__ __forceinline__ int posterior_status(double zf, double za) {
  return !span_mass_live(zf) ? SPAN_POISONED : !(za > 0.0) ? SPAN_CONTRADICTORY : SPAN_LIVE;
}

// the header of stage 1: sample n's row, LIVE with its active-point slice, or POISONED - empty, with a NaN logit, or longer than the
// 256 frames the family handles (the host cannot see tlen without a read-back).  All a launch needs that takes probabilities of its
// own (hual_al_evidence_grid: one softmax per temperature).  Called by the whole workgroup; one barrier on a row that is not empty.
__device__ __forceinline__ void open_span_row_header(const hual::AlSpanIn& in, int n, SpanRow& r) {
  r.T = in.set.tlen[n];
  r.row = (size_t)n * in.set.ld;
  const bool fits = r.T >= 1 && r.T <= 256 && r.T <= in.set.ld;
  r.v = fits ? span_clip_len(in.set.vlen[n], r.T) : 0;
  r.status = (r.v == 0 || span_row_poisoned(in.s0, in.e0, r.row, r.v)) ? SPAN_POISONED : SPAN_LIVE;
  if (r.status == SPAN_LIVE) {
    const int ap0 = in.set.ap_off[n];
    r.napn = in.set.ap_off[n + 1] - ap0;
    r.aidx = in.set.ap_idx + ap0;
    r.apos = in.set.ap_pos + ap0;
  }
}

// stage 1: the header, and on a LIVE row lds.ps / lds.pe readable and the hull.  Called by the whole workgroup; its barriers publish
// what was written before it.
__device__ __forceinline__ void open_span_row(const hual::AlSpanIn& in, int n, SpanRowLds& lds, SpanRow& r) {
  open_span_row_header(in, n, r);
  if (r.status == SPAN_LIVE) {
    span_probabilities(in.s0, in.e0, r.row, r.T, r.v, lds.ps, lds.pe, lds.smf, lds.smd);
    r.hull = ap_hull(r.aidx, r.apos, r.napn, r.v);
  }
}

// stage 2: stage 1, then Z and Z_A by posterior_masses and the row's final status
__device__ __forceinline__ void open_posterior_row(const hual::AlSpanIn& in, int n, SpanRowLds& lds, SpanRow& r) {
  open_span_row(in, n, lds, r);
  if (r.status == SPAN_LIVE) {
    posterior_masses(r.aidx, r.apos, r.napn, r.v, r.hull, lds.ps, lds.pe, lds.smd, r.zf, r.za);
    r.status = posterior_status(r.zf, r.za);
  }
}

// (uniform) body(first, last) for every non-empty gap between the negatives of a row without a positive, ascending
template <class Body>
__device__ __forceinline__ void for_each_gap(const SpanRow& r, Body body) {
  for (int cur = 0; cur < r.v;) {
    int nxt = r.v;
    for (int k = 0; k < r.napn; ++k) {
      const int f = r.aidx[k];
      if (!r.apos[k] && f >= cur && f < nxt) nxt = f;
    }
    if (nxt > cur) body(cur, nxt - 1);
    cur = nxt + 1;
  }
}

// body(c) for the columns [0, min(max(T, 0), ld)) a launch writes of a row of any status, the workgroup's threads striding over them
template <class Body>
__device__ __forceinline__ void for_each_column(const SpanRow& r, int ld, Body body) {
  const int Tw = min(max(r.T, 0), ld);
  for (int c = threadIdx.x; c < Tw; c += SPAN_THREADS) body(c);
}
