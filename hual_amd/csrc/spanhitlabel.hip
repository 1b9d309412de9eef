// hual_al_hit_label (include/hual_seqpan.h): label reliability - the chance P(IoU(span, truth) >= m | the answers) that a span counts as
// a hit at each of up to 4 exact rational IoU thresholds when the truth is drawn from the span posterior given the answered active
// points, for k given spans per sample (the old label, the MBR label, any other), and per threshold the member of the consistent set A
// that maximises it.  hual_span_hit_prob's quantity (spanhit.hip) on hual_al_query's posterior: the row - its status, probabilities,
// set A and Z_A - is opened by spanpost.h as in every launch of the family; not in the train step.
//
// One 1024-thread workgroup per selected sample, and with the search one per (sample, threshold): blockIdx.y = m searches threshold m,
// and the workgroups with blockIdx.y = 0 also score the candidates, one wave per (slot, threshold).  No workgroup reads what another
// writes.  No pair of spans is enumerated: per start i the ends with (i, j) in A are one interval [elo[i], ehi[i]] - around a positive
// hull [hi, min(negR, v) - 1] for negL < i <= lo, without a positive [i, the end of i's gap] - held in LDS beside the float64 prefix sums
// E of p_e, and a candidate's mass is sum_i p_s[i] * (E[min(j_hi, ehi[i]) + 1] - E[max(j_lo, elo[i])]) with spanmass.h's interval
// [j_lo, j_hi] of hitting ends (sh_mass_within).  The search walks the triangle in spanhit.hip's (length, end) order and skips the spans
// outside A; it ends on the family's (value, key) reduction (block.h).  No atomics, nothing grid wide: the result is a function of the
// inputs alone.  Without an active point no clamp binds and the masses are hual_span_hit_prob's doubles; the divisor is Z_A of
// posterior_masses, the same terms summed in another order than that launch's Z.
#include "prof.h"
#include "spanpost.h"
#include "spanmass.h"

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_hit_label_kernel(AlHitArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ double E[257];                                  // E[x] = sum of p_e[j], j < x
  __shared__ int ce[SH_MAXM][257], fl[SH_MAXM][257];
  __shared__ int elo[256], ehi[256];                         // the ends start i may take in A; elo > ehi: none
  __shared__ double wbv[SPAN_WAVES];
  __shared__ int wbk[SPAN_WAVES];
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (n < 0 || n >= a.in.set.N) return;                      // (uniform) an id outside the set writes nothing
  const int M = a.M, k = a.k;
  const bool candidates = k > 0 && blockIdx.y == 0;          // (uniform)
  sh_build_tables(a.num, a.den, M, ce, fl);                  // (the opening's barriers publish them; an empty row reads none)
  SpanRow r;
  open_posterior_row(a.in, n, lds, r);
  if (r.status != SPAN_LIVE) {
    if (candidates && t < k * M) a.cand_hit[(size_t)n * k * M + t] = -1.0f;
    if (a.best_idx && t == 0) {
      const size_t o = (size_t)n * M + blockIdx.y;
      a.best_idx[2 * o] = -1; a.best_idx[2 * o + 1] = -1;
      a.best_prob[o] = -1.0f;
    }
    return;
  }
  const float *ps = lds.ps, *pe = lds.pe;
  const int v = r.v;
  const double za = r.za;
  if (t <= v) {        // the prefix sums, each one serial sum in ascending order (spanhit.hip's)
    double s = 0.0;
    for (int j = 0; j < t; ++j) s += (double)pe[j];
    E[t] = s;
  }
  if (t < v) {
    int jl = 256, jh = -1;
    if (r.hull.npos > 0) {
      if (t > r.hull.negL && t <= r.hull.lo) { jl = r.hull.hi; jh = min(r.hull.negR, v) - 1; }
    } else {
      const ApSegment sg = ap_segment(r.aidx, r.apos, r.napn, v, t);
      if (!sg.closed) { jl = t; jh = sg.sb; }
    }
    elo[t] = jl; ehi[t] = jh;
  }
  __syncthreads();
  // ---- the candidates: one wave per (slot, threshold) pair
  if (candidates) {
    for (int p = w; p < k * M; p += SPAN_WAVES) {
      const int q = p / M, m = p - q * M;
      const size_t slot = (size_t)n * k + q;
      const int ca = a.cand_idx[2 * slot], cb = a.cand_idx[2 * slot + 1];      // (uniform over the wave)
      float val = -1.0f;
      if (ca >= 0 && ca <= cb && cb < v) {
        double acc = sh_mass_within(ca, cb, v, ps, E, ce[m], fl[m], elo, ehi, lane, 64);
        acc = wave_sum64_f64(acc);
        val = (float)fmin(1.0, fmax(0.0, acc / za));
      }
      if (lane == 0) a.cand_hit[slot * M + m] = val;
    }
  }
  // ---- the member of A of maximal hit mass at threshold blockIdx.y
  if (a.best_idx) {
    const int m = blockIdx.y;
    double bv = -1.0; int bk = SH_NONE;
    const int nt = tri_row_off(v, v);
    for (int c = t; c < nt; c += SPAN_THREADS) {      // by length, then by end (spanhit.hip's order); the spans outside A are skipped
      int len, e;
      tri_entry(c, v, len, e);
      const int s = e - len;
      if (e < elo[s] || e > ehi[s]) continue;
      const int key = (s << 8) | e;
      const double mass = sh_mass_within(s, e, v, ps, E, ce[m], fl[m], elo, ehi, 0, 1);
      if (FirstIndexMax()(mass, key, bv, bk)) { bv = mass; bk = key; }      // (the key a * 256 + b: first in row-major order)
    }
    wave_best(bv, bk);
    if (lane == 0) { wbv[w] = bv; wbk[w] = bk; }
    __syncthreads();
    if (t == 0) {
      best_of_waves(wbv, wbk, SPAN_WAVES, bv, bk);
      const size_t o = (size_t)n * M + m;
      const bool found = bk != SH_NONE;      // (a live row has Z_A > 0, so A has a member)
      a.best_idx[2 * o] = found ? bk >> 8 : -1;
      a.best_idx[2 * o + 1] = found ? bk & 255 : -1;
      a.best_prob[o] = found ? (float)fmin(1.0, fmax(0.0, bv / za)) : -1.0f;
    }
  }
}

}  // namespace

namespace hual {

int launch_al_hit_label(const AlHitArgs& a, int nsel, hipStream_t s) {
  const int rc = check_span_in(a.in, "al_hit_label", [&] {
    HUAL_REQUIRE(a.k == 0 || (a.cand_idx && a.cand_hit), "al_hit_label: null pointer (cand_idx, cand_hit with k >= 1)");
    HUAL_REQUIRE(!a.best_idx == !a.best_prob, "al_hit_label: best_idx and best_prob are given together or not at all");
    HUAL_REQUIRE(a.k >= 1 || a.best_idx, "al_hit_label: nothing to do (k == 0 and no best_* outputs)");
    HUAL_REQUIRE(nsel >= 1, "al_hit_label: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  const int grid = a.sel ? nsel : a.in.set.N;      // without a list every sample is selected
  const double bytes = (8.0 * a.in.set.ld + 12.0 * a.k + 4.0 * a.k * a.M + (a.best_idx ? 12.0 * a.M : 0.0) + (a.sel ? 4.0 : 0.0)) * grid;
  HUAL_LAUNCH(0.0, bytes, al_hit_label_kernel, dim3(grid, a.best_idx ? a.M : 1), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_hit_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel,
                                 const int32_t* thresholds, int M, const int32_t* cand_idx, int k, float* cand_hit, int32_t* best_idx,
                                 float* best_prob, void* stream) {
  HUAL_REQUIRE(set && thresholds, "hual_al_hit_label: null pointer (set, thresholds)");
  HUAL_REQUIRE(k >= 0 && k <= SPAN_MAXK, "hual_al_hit_label: 0 <= k <= 16");
  HUAL_REQUIRE(M >= 1 && M <= SH_MAXM, "hual_al_hit_label: 1 <= M <= 4");
  AlHitArgs a{};
  for (int m = 0; m < M; ++m) {
    a.num[m] = thresholds[2 * m]; a.den[m] = thresholds[2 * m + 1];
    HUAL_REQUIRE(a.num[m] >= 1 && a.num[m] <= a.den[m] && a.den[m] <= SH_MAXDEN,
                 "hual_al_hit_label: thresholds are (num, den) with 1 <= num <= den <= 1024");
  }
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  a.sel = sel; a.M = M; a.k = k; a.cand_idx = cand_idx; a.cand_hit = cand_hit; a.best_idx = best_idx; a.best_prob = best_prob;
  return launch_al_hit_label(a, nsel, (hipStream_t)stream);
}
