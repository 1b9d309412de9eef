// hual_al_design (include/hual_seqpan.h): the frames to ask TOGETHER about a clip - for an annotator who is not in the loop (a
// labelling tool, a crowd batch, one viewing of the clip), where the next frame cannot wait for the previous answer.  The answers to
// membership questions are a function of the span, so the information a set of frames D carries about the span is the entropy of its
// answer vector, I(D) = H(a_D), under the span posterior of hual_al_query; the design is greedy: step m takes the first frame of maximal
// I(D + t).  One 1024-thread workgroup per selected sample, as the rest of the family; the row is opened by spanpost.h, and step 0 IS
// hual_al_query (spanstep.h's query_step + query_step_best).  Not in the train step.
//
// The marginal gain, by the chain rule: I(D + t) - I(D) = sum over the outcomes o of D of P(o) h2(q_o(t)), q_o(t) the inclusion
// probability of t under the posterior restricted to o.  The frames of D that carried information - the CUTS - split every segment
// between the set's negatives into cells; an outcome is a rectangle (the span starts in the cell that ends at cut c_p and ends in the
// cell that starts at cut c_r, p <= r: the positive answers are c_p .. c_r) or the all-negative outcome (the span lies strictly
// between two cuts, in whichever gap: one outcome).  With the segmented float64 sums
//    segS[t] = sum of p_s over (the cut or negative below t, t]       segE[t] = sum of p_e over [t, the cut or negative above t)
// - at a cut, its cell's sum - a frame t between the cuts dn < t < up of its segment
//  - splits the START cell of the rectangles (up, r >= up):  segS[up] * (sum over the cuts r >= up of segE[r]) * h2(segS[t] / segS[up])
//  - splits the END cell of the rectangles (p <= dn, dn):    segE[dn] * (sum over the cuts p <= dn of segS[p]) * h2(segE[t] / segE[dn])
//  - splits its triangle of the all-negative outcome:        Z_0 * h2(segS[t] * segE[t] / Z_0),  Z_0 = sum over the frames j that are
//    no cut of p_e[j] segS[j]
// and lies inside (q = 1) or outside (q = 0) every other outcome; the three, over Z_A, are the gain.  Around a positive hull [lo, hi]
// the consistent set is the product (negL, lo] x [hi, negR): lo closes the start cells, hi opens the end cells, there is no
// all-negative outcome, and a frame splits one start cell (every end cell beside it) or one end cell.  Every sum adds terms of one
// sign in float64 and restarts at every cut and negative - no difference of whole-row prefix sums, as in query_step.  Each of the two
// segmented sums is a serial walk of one thread per frame (two quarters of the workgroup), the cuts are at most 16 words of LDS, so a
// candidate costs O(cuts) on top of its walk.
//
// The loop holds barriers, so it is left by every thread in the same iteration: thread 0 alone decides, writes the decision to LDS,
// and all threads read that word behind a barrier.  No break or return under a thread-dependent condition lies between two barriers.
#include "prof.h"
#include "spanstep.h"

using namespace hual;

namespace {

constexpr int DESIGN_MAX_M = 16;            // frames per sample

struct DesignLds {
  double segS[256], segE[256];              // the segmented sums of the step (above)
  double gl[256];                           // the step's marginal gain per frame, bits: what a forced frame is read from
  double bestv[SPAN_WAVES];
  int besti[SPAN_WAVES];
  int32_t cut[DESIGN_MAX_M];                // the placed frames that carried information, in the order placed
  int ncut;
  int32_t frames[DESIGN_MAX_M];             // the design, unused slots -1
  float info[DESIGN_MAX_M];
  int reason;                               // the step's decision: -1 = placed, go on; else the HUAL_AL_STOP_* that ended the design
};

// binary entropy in bits, float64; 0 outside (0, 1) and at a NaN
__device__ __forceinline__ double h2_bits_f64(double q) {
  if (!(q > 0.0 && q < 1.0)) return 0.0;
  const double r = 1.0 - q;
  return -(q * log2(q) + r * log2(r));
}

__global__ __launch_bounds__(SPAN_THREADS) void al_design_kernel(AlDesignArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ QueryStepLds ql;
  __shared__ DesignLds ds;
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  const int mmax = a.mmax;
  if (t < mmax) { ds.frames[t] = -1; ds.info[t] = -1.0f; }
  if (t == 0) ds.ncut = 0;
  SpanRow r;
  open_span_row(a.in, n, lds, r);
  const int v = r.v;
  int reason = -1, m = 0;                   // (uniform) why the design ended | the frames placed so far
  QueryStep st;
  st.q = 0.f; st.g = 0.f; st.za = 0.0; st.hs = 0.0;
  int status = r.status;
  if (status == SPAN_LIVE) {                // step 0: hual_al_query's own arithmetic
    if (t < v) { ql.ls[t] = log2f(lds.ps[t]); ql.le[t] = log2f(lds.pe[t]); }
    query_step(r.aidx, r.apos, r.napn, v, r.hull, lds.ps, lds.pe, ql, lds.smd, st);
    status = st.status;
  }
  if (status != SPAN_LIVE) reason = status == SPAN_CONTRADICTORY ? HUAL_AL_STOP_CONTRADICTORY : HUAL_AL_STOP_POISONED;
  // this thread's frame c: its segment between the set's negatives, and whether an answer at c can say anything at all
  const int kind = t >> 8, c = t & 255;
  ApSegment sg;
  sg.sa = 0; sg.sb = -1; sg.closed = true;
  int npos = 0, lo = 0, hi = 0;
  bool play = false;
  if (reason < 0) {
    sg = ap_segment(r.aidx, r.apos, r.napn, v, c);
    npos = r.hull.npos; lo = r.hull.lo; hi = r.hull.hi;
    play = c < v && !sg.closed && (npos == 0 || (c > r.hull.negL && c < r.hull.negR && (c < lo || c > hi)));
    if (t < v) ds.gl[t] = (double)st.g;     // step 0's gains: the float32 h2_bits of hual_al_query
  }
  // thread 0's own: the running information, the cursor into the forced prefix, hual_al_query's entropy
  double cur = 0.0, hA = 0.0;
  int fc = a.forced ? 0 : mmax;
  float ent32 = -1.0f, qbest = -1.0f;
  int qbi = -1;
  __syncthreads();                          // the fills and step 0's gains are in LDS
  while (reason < 0) {                      // (uniform: `reason` is read from LDS behind a barrier at the end of every pass)
    if (m > 0) {
      const int ncut = ds.ncut;
      bool iscut = false;
      if (c < v && kind < 2) {
        int lower = sg.sa, upper = sg.sb;
        for (int k = 0; k < ncut; ++k) {
          const int f = ds.cut[k];
          if (f < c) lower = max(lower, f + 1);
          else if (f > c) upper = min(upper, f - 1);
          else iscut = true;
        }
        double seg = 0.0;
        if (kind == 0) {
          for (int i = lower; i <= c; ++i) seg += (double)lds.ps[i];
          ds.segS[c] = sg.closed ? 0.0 : seg;
        } else {
          for (int i = c; i <= upper; ++i) seg += (double)lds.pe[i];
          ds.segE[c] = sg.closed ? 0.0 : seg;
        }
      }
      __syncthreads();
      double z0 = 0.0;                      // the all-negative outcome's mass (none around a positive hull)
      if (npos == 0) {                      // (uniform)
        if (t < v && !sg.closed && !iscut) z0 = (double)lds.pe[t] * ds.segS[t];
        z0 = block_reduce<BlockSumD, SPAN_WAVES>(z0, lds.smd);
      }
      double g = 0.0;
      if (t < v && play && !iscut) {
        double num = 0.0;
        if (npos > 0) {
          if (t < lo) {                     // a start cell, beside every end cell
            int up = lo;
            double ER = ds.segE[hi];
            for (int k = 0; k < ncut; ++k) {
              const int f = ds.cut[k];
              if (f > t && f < lo) up = min(up, f);
              if (f > hi && f <= sg.sb) ER += ds.segE[f];
            }
            const double CS = ds.segS[up];
            if (CS > 0.0) num = CS * ER * h2_bits_f64(ds.segS[t] / CS);
          } else {                          // an end cell, beside every start cell
            int dn = hi;
            double SL = ds.segS[lo];
            for (int k = 0; k < ncut; ++k) {
              const int f = ds.cut[k];
              if (f < t && f > hi) dn = max(dn, f);
              if (f < lo && f >= sg.sa) SL += ds.segS[f];
            }
            const double CE = ds.segE[dn];
            if (CE > 0.0) num = CE * SL * h2_bits_f64(ds.segE[t] / CE);
          }
        } else {
          int up = 0x7fffffff, dn = -1;     // the cuts around t in its segment
          for (int k = 0; k < ncut; ++k) {
            const int f = ds.cut[k];
            if (f > t && f <= sg.sb) up = min(up, f);
            if (f < t && f >= sg.sa) dn = max(dn, f);
          }
          if (up != 0x7fffffff) {
            double ER = 0.0;
            for (int k = 0; k < ncut; ++k) {
              const int f = ds.cut[k];
              if (f >= up && f <= sg.sb) ER += ds.segE[f];
            }
            const double CS = ds.segS[up];
            if (CS > 0.0) num += CS * ER * h2_bits_f64(ds.segS[t] / CS);
          }
          if (dn >= 0) {
            double SL = 0.0;
            for (int k = 0; k < ncut; ++k) {
              const int f = ds.cut[k];
              if (f <= dn && f >= sg.sa) SL += ds.segS[f];
            }
            const double CE = ds.segE[dn];
            if (CE > 0.0) num += CE * SL * h2_bits_f64(ds.segE[t] / CE);
          }
          if (z0 > 0.0) num += z0 * h2_bits_f64(ds.segS[t] * ds.segE[t] / z0);
        }
        g = fmax(num / st.za, 0.0);
      }
      if (t < v) ds.gl[t] = g;
      double best = t < v ? g : -1.0;
      int bi = t < v ? t : 0x7fffffff;
      wave_best(best, bi);
      if ((t & 63) == 0) { ds.bestv[t >> 6] = best; ds.besti[t >> 6] = bi; }
      __syncthreads();
    }
    if (t == 0) {
      int why = -1, pick = -1;
      double gain = 0.0;
      if (m == 0) {                         // hual_al_query's frame, gain and entropy as it stores them, and the entropy's float64
        query_step_best(ql, st, qbi, qbest, ent32);
        const double h = log2(st.za) - st.hs / st.za;
        hA = h > 0.0 ? h : 0.0;
      }
      if (m >= mmax) {
        why = HUAL_AL_STOP_BUDGET;
      } else {
        int f = -1;                         // the next forced frame
        while (fc < mmax) {
          const int x = a.forced[(size_t)n * mmax + fc];
          if (x < 0) { fc = mmax; break; }  // ends the prefix
          ++fc;
          if (x < v) { f = x; break; }      // (x >= v: outside the clip, ignored)
        }
        if (f >= 0) {                       // placed without a stop test
          pick = f;
          gain = ds.gl[f];
        } else {
          int bi;
          double best;
          if (m == 0) {
            bi = qbi;
            best = (double)qbest;
          } else {
            best_of_waves(ds.bestv, ds.besti, SPAN_WAVES, best, bi);
          }
          if (a.stop_entropy >= 0.f && hA - cur <= (double)a.stop_entropy) why = HUAL_AL_STOP_ENTROPY;
          else if (!(best > (double)a.min_gain)) why = HUAL_AL_STOP_GAIN;
          else if (bi < 0 || bi >= v) why = HUAL_AL_STOP_GAIN;      // (never on a live row: gl and the cuts are indexed by it)
          else { pick = bi; gain = best; }
        }
      }
      if (why < 0) {                        // place: m < mmax, pick in [0, v), ncut <= m
        cur += gain;
        ds.frames[m] = pick;
        ds.info[m] = (float)cur;
        if (gain > 0.0) ds.cut[ds.ncut++] = pick;      // (a frame of 0 bits - a repeat, an answered one - splits no cell)
      }
      ds.reason = why;
    }
    __syncthreads();
    reason = ds.reason;
    if (reason < 0) ++m;
  }
  __syncthreads();
  const size_t o = (size_t)n * mmax;
  if (t < mmax) { a.frames[o + t] = ds.frames[t]; a.info[o + t] = ds.info[t]; }
  if (t == 0) { a.post_entropy[n] = ent32; a.n_design[n] = m; a.stop_reason[n] = reason; }
}

}  // namespace

namespace hual {

int launch_al_design(const AlDesignArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_design", [&] {
    HUAL_REQUIRE(a.frames && a.info && a.post_entropy && a.n_design && a.stop_reason, "al_design: null output");
    HUAL_REQUIRE(!a.sel || nsel >= 1, "al_design: nsel >= 1");
    HUAL_REQUIRE(a.mmax >= 1 && a.mmax <= DESIGN_MAX_M, "al_design: mmax in [1, 16]");
    HUAL_REQUIRE(a.min_gain >= 0.f, "al_design: min_gain >= 0");
    HUAL_REQUIRE(a.stop_entropy == a.stop_entropy, "al_design: stop_entropy is a number");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  // per sample: two rows of logits in, the design out (8 bytes per slot, 4 more with a forced prefix, the three per-sample words)
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + (a.forced ? 12.0 : 8.0) * a.mmax + 12.0) * grid, al_design_kernel, dim3(grid), dim3(SPAN_THREADS), 0,
              s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_design(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, int mmax,
                              const int32_t* forced, float min_gain, float stop_entropy, int32_t* frames, float* info,
                              float* post_entropy, int32_t* n_design, int32_t* stop_reason, void* stream) {
  HUAL_REQUIRE(set, "hual_al_design: null set");
  AlDesignArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.sel = sel; a.mmax = mmax; a.forced = forced; a.min_gain = min_gain; a.stop_entropy = stop_entropy;
  a.frames = frames; a.info = info; a.post_entropy = post_entropy; a.n_design = n_design; a.stop_reason = stop_reason;
  return launch_al_design(a, nsel, (hipStream_t)stream);
}
