// The maximal expected tIoU over the candidates of one region of the consistent set A, shared by the kernels that maximise it
// (hual_al_mbr_label in spanlabel.hip, hual_al_label_gain in spangain.hip; the contract is in include/hual_seqpan.h).  One definition,
// so the value of a label and the value the label would have after one more answer are the same arithmetic.
//
// No pair of spans is enumerated.  A is a union of regions {sa <= i <= ihi, jlo <= j <= sb, i <= j} (a gap between negatives:
// ihi = sb, jlo = sa; a positive hull: (negL, lo] x [hi, negR)), and a candidate (a, e) overlaps only the spans of its own region.
// With, for a fixed end e,
//   G_e[m] = sum_{j = max(m, jlo) .. e} p_e[j] (j - m + 1)        H_e[l] = sum_{j = e + 1 .. sb} p_e[j] / (j - l + 1)
// the IoU-weighted mass Z_A R(a, e) is the sum of the four cases of (i < a or i >= a) x (j <= e or j > e):
//   G_e[a] sum_{i < a} p_s[i] / (e - i + 1)  +  (e - a + 1) sum_{i < a} p_s[i] H_e[i]
//   +  sum_{i = a .. min(ihi, e)} p_s[i] G_e[i] / (e - a + 1)  +  H_e[a] sum_{i = a .. min(ihi, e)} p_s[i] (e - i + 1)
// The workgroup walks e down from sb; the quad of frame l keeps H_e[l] in a register (one term added per step), sums G_e[l] over j,
// publishes p_s[l] H_e[l] and p_s[l] G_e[l] in LDS, and after a barrier sums its own two prefixes and two suffixes over i.  Every sum
// adds terms of one sign in float64 in a fixed order (a lane takes every fourth term, the quad is folded by two shuffles): no difference
// of prefix sums, no atomics, nothing grid wide.  At most v^3 / 2 additions for the full triangle.
#pragma once
#include "spanpost.h"

constexpr int AM_QUAD = 4;      // lanes per frame

// the sum over the four lanes of a frame, in every one of them
__device__ __forceinline__ double quad_sum(double x) {
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  return x;
}

// the candidates (a, e) of one region, a = the quad's frame g: best / bi <- the first maximal R = (IoU-weighted mass) / za in row-major
// order, bi = a * 256 + e.  Called by the whole workgroup with uniform arguments; starts and ends on a barrier-free state of xh / xg
// (its last statement of an iteration is a barrier).
__device__ __forceinline__ void label_region(int sa, int ihi, int jlo, int sb, const float* ps, const float* pe, const double* inv,
                                             double* xh, double* xg, double za, double& best, int& bi) {
  const int g = threadIdx.x / AM_QUAD, q = threadIdx.x % AM_QUAD;
  double H = 0.0;                           // H_e[g]
  for (int e = sb; e >= jlo; --e) {
    const int m = min(ihi, e);
    const bool on = g >= sa && g <= m;
    double G = 0.0;                         // G_e[g]
    if (on)
      for (int j = max(g, jlo) + q; j <= e; j += AM_QUAD) G += (double)pe[j] * (double)(j - g + 1);
    G = quad_sum(G);
    if (on && q == 0) { xh[g] = (double)ps[g] * H; xg[g] = (double)ps[g] * G; }
    __syncthreads();
    double p1 = 0.0, p2 = 0.0, s3 = 0.0, s4 = 0.0;
    if (on) {
      for (int i = sa + q; i < g; i += AM_QUAD) { p1 += (double)ps[i] * inv[e - i + 1]; p2 += xh[i]; }
      for (int i = g + q; i <= m; i += AM_QUAD) { s3 += xg[i]; s4 += (double)ps[i] * (double)(e - i + 1); }
    }
    p1 = quad_sum(p1); p2 = quad_sum(p2); s3 = quad_sum(s3); s4 = quad_sum(s4);
    if (on) {
      const double len = (double)(e - g + 1);
      const double r = (G * p1 + len * p2 + s3 / len + H * s4) / za;
      if (r >= best) { best = r; bi = g * 256 + e; }      // e descends: among equal values the smallest e stays
    }
    __syncthreads();                        // xh / xg are rewritten by the next step
    if (g <= e) H += (double)pe[e] * inv[e - g + 1];
  }
}
