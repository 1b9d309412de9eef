// The hit mass of a span at an exact rational IoU threshold, as hual_span_hit_prob (spanhit.hip) and hual_span_hit_cover (spancover.hip)
// take it, and hual_al_hit_label (spanhitlabel.hip) within a consistent set: the thresholds passed by value, the two division tables,
// the interval of hitting ends per start and the sum over the starts.
// One definition, so the first step of the cover search is the Bayes search of spanhit.hip instruction for instruction (as spanstep.h
// is shared by the query and the session kernels).
#pragma once
#include "common.h"
#include "spanclip.h"

constexpr int SH_MAXM = 4, SH_MAXDEN = 1024;
constexpr int SH_NONE = 0x7fffffff;      // key of "no candidate" (mass -1: below every real mass, which is >= 0)

struct ShThresholds { int num[SH_MAXM], den[SH_MAXM]; };      // by value: read on the host before the launch

// The starts and ends that hit the candidate (a, b), 0 <= a <= b < v, at threshold num / den: den * inter >= num * union in integers,
// inter and union of the half-open frame intervals.  num >= 1 asks inter >= 1, so i <= b and j >= max(a, i), and the union is one
// interval.  With lo = min(a, i), hi = max(a, i):
//   j <= b: inter = j + 1 - hi, union = b + 1 - lo =: U; a hit iff j >= hi - 1 + ceil(num U / den) =: j_lo   (rising in j)
//   j >= b: inter = b + 1 - hi =: I, union = j + 1 - lo; a hit iff j <= lo - 1 + floor(den I / num) =: j_hi   (falling in j)
// The two agree at j = b, so the hits of start i are [j_lo, min(j_hi, v - 1)] when b itself hits (j_lo <= b) and none otherwise.
//   i <= a: I = n := b + 1 - a is fixed; j_lo <= b iff num (b + 1 - i) <= den n iff i >= b + 1 - fl[n]
//   i >= a: U = n is fixed;              j_lo <= b iff i <= b + 1 - ce[n]
// ce[x] = ceil(num x / den), fl[x] = floor(den x / num) (capped at 256: only min(., v - 1) reads it), 1 <= x <= 256; ce[x] <= x <= fl[x].

// the two division tables of M thresholds, by the whole workgroup (entry 0 is never read)
__device__ __forceinline__ void sh_build_tables(const int* num, const int* den, int M, int (*ce)[257], int (*fl)[257]) {
  for (int x = threadIdx.x; x < M * 257; x += SPAN_THREADS) {
    const int m = x / 257, n = x - m * 257;
    ce[m][n] = (num[m] * n + den[m] - 1) / den[m];
    fl[m][n] = min(256, (den[m] * n) / num[m]);
  }
}

// this thread's share of the hit mass of (a, b): the starts first, first + step, .. of the hitting range, walked from a outwards
__device__ __forceinline__ double sh_mass(int a, int b, int v, const float* ps, const double* E, const int* ce, const int* fl, int first,
                                          int step) {
  const int n = b + 1 - a, F = fl[n], C = ce[n];
  const int imin = max(0, b + 1 - F), imax = b + 1 - C;      // imin <= a <= imax <= b
  double acc = 0.0;
  for (int i = a - first; i >= imin; i -= step) {            // i <= a: j_lo = a - 1 + ce[b + 1 - i] in [a, b], j_hi = i - 1 + F >= b
    const int jlo = a - 1 + ce[b + 1 - i], jhi = min(v - 1, i - 1 + F);
    acc += (double)ps[i] * (E[jhi + 1] - E[jlo]);
  }
  for (int i = a + step - first; i <= imax; i += step) {     // i > a: j_lo = i - 1 + C in (a, b], j_hi = a - 1 + fl[b + 1 - i] >= b
    const int jlo = i - 1 + C, jhi = min(v - 1, a - 1 + fl[b + 1 - i]);
    acc += (double)ps[i] * (E[jhi + 1] - E[jlo]);
  }
  return acc;
}

// sh_mass over the truths of a consistent set A (hual_al_hit_label, spanhitlabel.hip): per start i the ends with (i, j) in A are one
// interval [elo[i], ehi[i]] (elo > ehi: i starts no member), and the hitting ends of that start are sh_mass's interval clamped to it.
// The same starts in the same order, from a outwards: with elo[i] = i and ehi[i] = v - 1 - no active point - no clamp binds, no term
// is skipped and the sum is sh_mass's double.
__device__ __forceinline__ double sh_mass_within(int a, int b, int v, const float* ps, const double* E, const int* ce, const int* fl,
                                                 const int* elo, const int* ehi, int first, int step) {
  const int n = b + 1 - a, F = fl[n], C = ce[n];
  const int imin = max(0, b + 1 - F), imax = b + 1 - C;
  double acc = 0.0;
  for (int i = a - first; i >= imin; i -= step) {
    const int jlo = max(a - 1 + ce[b + 1 - i], elo[i]), jhi = min(min(v - 1, i - 1 + F), ehi[i]);
    if (jhi >= jlo) acc += (double)ps[i] * (E[jhi + 1] - E[jlo]);
  }
  for (int i = a + step - first; i <= imax; i += step) {
    const int jlo = max(i - 1 + C, elo[i]), jhi = min(min(v - 1, a - 1 + fl[b + 1 - i]), ehi[i]);
    if (jhi >= jlo) acc += (double)ps[i] * (E[jhi + 1] - E[jlo]);
  }
  return acc;
}

// the ends [jlo, jhi] that hit (a, b) from the start i < v, sh_mass's interval of that start; false: none
__device__ __forceinline__ bool sh_interval(int a, int b, int v, int i, const int* ce, const int* fl, int& jlo, int& jhi) {
  const int n = b + 1 - a, F = fl[n], C = ce[n];
  if (i < max(0, b + 1 - F) || i > b + 1 - C) return false;
  if (i <= a) { jlo = a - 1 + ce[b + 1 - i]; jhi = min(v - 1, i - 1 + F); }
  else { jlo = i - 1 + C; jhi = min(v - 1, a - 1 + fl[b + 1 - i]); }
  return true;
}
