// hual_al_evidence_grid (spancalib.hip; the contract is in include/hual_seqpan.h): the evidence of a set's answers on a grid of
// temperatures and error rates, and its sum over the set - the likelihood a caller maximises to calibrate the span posterior.
// Here: the argument record, and the arithmetic of sums whose terms carry an integer power of r = (1 - eps) / eps.
#pragma once
#include "spanpost.h"

namespace hual {

constexpr int CALIB_MAX_TAU = 32;             // temperatures per launch
constexpr int CALIB_MAX_EPS = 16;             // error rates per launch: one wave of the workgroup each
constexpr int CALIB_POW = 128;                // r^-d is tabulated for 0 <= d <= CALIB_POW, evaluated beyond
constexpr int CALIB_FOLD_THREADS = 256;

struct AlGridArgs {
  AlSpanIn in;                                // the set with its answers, the unscaled logits
  const int32_t* sel;                         // [nsel] sample ids (NULL: all)
  int nsel;                                   // entries of sel, N without a list
  int A, B;                                   // the grid: A temperatures x B error rates, cell c = a * B + b
  float inv_tau[CALIB_MAX_TAU];               // 1 / tau, float32 as torch multiplies by it
  double lnr[CALIB_MAX_EPS], ln_eps[CALIB_MAX_EPS], ln_1meps[CALIB_MAX_EPS];      // ln r, ln eps, ln(1 - eps) in float64 (the host's)
  double* table;                              // [N, A * B] ln P(the answers | the row at 1 / tau, eps), NaN in a poisoned cell
  int32_t* status;                            // [N] 1: every cell of the row is finite
  double* total;                              // [A * B] the sum of the selected rows of status 1
  int32_t* counts;                            // [4] rows summed, answers summed, rows excluded, the first cell of maximal total
};

int launch_al_evidence_grid(const AlGridArgs& a, hipStream_t s);

// x * k: one float32 product rounded on its own, torch's x * k - never the first half of a fused multiply-add with the softmax's
// subtraction of the row maximum behind it (tilt_logit in spannoisy.h says how the contraction is kept off)
__device__ __forceinline__ float scale_logit(float x, float k) {
#pragma clang fp contract(off)
  const float p = x * k;
  return p;
}

// r^-d, d >= 0: from the wave's table (LDS) where it reaches, the same expression beyond
__device__ __forceinline__ double r_pow_neg(const double* tab, int d, double lnr) {
  return d <= CALIB_POW ? tab[d] : exp(-(double)d * lnr);
}

// (m, k) += (m2, k2), a pair standing for m r^k with m >= 0: the sum is carried against the larger exponent, so the factor is <= 1 and
// nothing overflows; a zero mantissa carries no exponent (a frame of probability 0 must not scale the others towards 0).  Only where
// the exponents differ is a power of r read.  Commutative bit for bit: a butterfly leaves the same pair in every lane.
__device__ __forceinline__ void rpow_add(double& m, int& k, double m2, int k2, const double* tab, double lnr) {
#pragma clang fp contract(off)                // (both orders of the arguments round alike)
  if (m2 == 0.0) return;
  if (m == 0.0) { m = m2; k = k2; return; }
  const int d = k - k2;
  if (d == 0) m += m2;
  else if (d > 0) m += m2 * r_pow_neg(tab, d, lnr);
  else { m = m * r_pow_neg(tab, -d, lnr) + m2; k = k2; }
}

}  // namespace hual
