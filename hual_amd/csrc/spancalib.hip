// hual_al_evidence_grid (include/hual_seqpan.h): ln P(the answers of a sample | softmax(s0 / tau), softmax(e0 / tau), eps) on a grid of
// A temperatures x B error rates, and the sum of every cell over the set: the likelihood L(tau, eps) that calibrates the span posterior
// the rest of the family reads.  Not in the train step.
//
// al_evidence_grid_kernel - one 1024-thread workgroup per selected sample.  G(t), the count hual_al_noisy_tilt carries, depends on
// neither tau nor eps: counted once.  Per temperature: the float32 product s0 * (1 / tau) rounded on its own and the family's softmax of
// it (span_probabilities_of: bit for bit span_probabilities of the scaled row).  Then wave b owns the cell (a, b): with r = (1 - eps[b])
// / eps[b] the evidence is
//   ln [ eps^npos (1 - eps)^nneg sum_j p_e[j] r^G(j) sum_{i <= j} p_s[i] r^-G(i-1) / Z ]
// and the inner sum is a prefix scan over pairs (mantissa, integer exponent of r) - rpow_add, spancalib.h -, four frames per lane, the
// lanes' totals scanned across the wave.  The powers r^-d a sum needs where exponents differ come from a table in LDS, filled once per
// workgroup: d is at most twice the number of answers, and past the table the same expression is evaluated.  So a cell costs O(v +
// answers) float64 operations and one logarithm pair, where hual_al_noisy_tilt evaluates an exp per (start, end) pair.  Sums of terms of
// one sign in a fixed order, no atomics.
//
// al_evidence_fold_kernel - one workgroup per cell - sums the cell over the selected rows whose every cell is finite, in a fixed order;
// al_evidence_best_kernel - one wave - takes the first cell of maximal total.
#include "prof.h"
#include "spancalib.h"

#include <cmath>

using namespace hual;

namespace {

__global__ __launch_bounds__(SPAN_THREADS) void al_evidence_grid_kernel(AlGridArgs a) {
  __shared__ SpanRowLds lds;
  __shared__ int gs[257];                   // gs[t + 1] = G(t), gs[0] = G(-1) = 0
  __shared__ double pw[CALIB_MAX_EPS][CALIB_POW + 1];      // pw[b][d] = r_b^-d
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
  if (n < 0 || n >= a.in.set.N) return;     // (uniform) an id outside the set writes nothing
  const int AB = a.A * a.B;
  double* cells = a.table + (size_t)n * AB;
  SpanRow r;
  open_span_row_header(a.in, n, r);         // (the probabilities are per temperature, below)
  if (r.status != SPAN_LIVE) {              // (uniform) x * (1 / tau) is a NaN exactly where x is
    for (int c = t; c < AB; c += SPAN_THREADS) cells[c] = NAN;
    if (t == 0) a.status[n] = 0;
    return;
  }
  const int T = r.T, v = r.v, napn = r.napn;
  const size_t row = r.row;
  const int32_t* aidx = r.aidx;
  const int8_t* apos = r.apos;
  int G = 0, npos = 0, nneg = 0;            // (npos / nneg uniform: every thread walks the whole list)
  for (int k = 0; k < napn; ++k) {
    const int f = aidx[k];
    if (f < 0 || f >= v) continue;
    const int sgn = apos[k] ? 1 : -1;
    if (sgn > 0) ++npos; else ++nneg;
    if (f <= t) G += sgn;
  }
  if (t < v) gs[t + 1] = G;
  if (t == 0) gs[0] = 0;
  for (int x = t; x < a.B * (CALIB_POW + 1); x += SPAN_THREADS) {
    const int b = x / (CALIB_POW + 1), d = x % (CALIB_POW + 1);
    pw[b][d] = exp(-(double)d * a.lnr[b]);
  }
  const float s_raw = t < v ? a.in.s0[row + t] : 0.f, e_raw = t < v ? a.in.e0[row + t] : 0.f;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const bool mine = w < a.B;                // (uniform per wave) wave b owns the cells (., b)
  const double lnr = mine ? a.lnr[w] : 0.0;
  const double* tab = pw[mine ? w : 0];
  const double base = mine ? (double)npos * a.ln_eps[w] + (double)nneg * a.ln_1meps[w] : 0.0;
  bool finite = true;
  for (int ia = 0; ia < a.A; ++ia) {
    __syncthreads();                        // gs and pw are published; the waves are done with the probabilities before
    const float k = a.inv_tau[ia];
    span_probabilities_of([&] { return scale_logit(s_raw, k); }, [&] { return scale_logit(e_raw, k); }, T, v, lds.ps, lds.pe, lds.smf, lds.smd);
    if (!mine) continue;
    const float *ps = lds.ps, *pe = lds.pe;
    // the lane's frames 4 lane .. 4 lane + 3: the prefixes within them of p_s r^-G(i-1) (as pairs) and of p_s (plain, for Z)
    double pm[4], pp[4];
    int pk[4];
    double m = 0.0, p = 0.0;
    int e = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * lane + q;
      if (j < v) {
        rpow_add(m, e, (double)ps[j], -gs[j], tab, lnr);
        p += (double)ps[j];
      }
      pm[q] = m; pk[q] = e; pp[q] = p;
    }
    // inclusive scan of the lanes' totals across the wave, then the total of the lanes below
    double sm = m, sp = p;
    int sk = e;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double om = __shfl_up(sm, off), op = __shfl_up(sp, off);
      const int ok = __shfl_up(sk, off);
      if (lane >= off) {
        rpow_add(sm, sk, om, ok, tab, lnr);
        sp += op;
      }
    }
    double xm = __shfl_up(sm, 1), xp = __shfl_up(sp, 1);
    int xk = __shfl_up(sk, 1);
    if (lane == 0) { xm = 0.0; xp = 0.0; xk = 0; }
    // frame j's term p_e[j] r^G(j) (the inner sum up to j), and its share of Z
    double tm = 0.0, zf = 0.0;
    int tk = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * lane + q;
      if (j < v) {
        double im = xm;
        int ik = xk;
        rpow_add(im, ik, pm[q], pk[q], tab, lnr);
        const double pj = (double)pe[j];
        rpow_add(tm, tk, pj * im, ik + gs[j + 1], tab, lnr);
        zf += pj * (xp + pp[q]);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double om = __shfl_xor(tm, off);
      const int ok = __shfl_xor(tk, off);
      rpow_add(tm, tk, om, ok, tab, lnr);
      zf += __shfl_xor(zf, off);
    }
    double ev = NAN;                        // hual_al_noisy_tilt's rule: every weight underflowed, or an infinite logit made them NaN
    if (span_mass_live(zf)) ev = npos + nneg == 0 ? 0.0 : base + (double)tk * lnr + log(tm) - log(zf);
    if (lane == 0) cells[ia * a.B + w] = ev;
    finite = finite && __builtin_isfinite(ev);
  }
  const int live = __syncthreads_and(finite);
  if (t == 0) a.status[n] = live ? 1 : 0;
}

// the answers of sample n that count: those at a frame inside [0, v) (called on rows of status 1 only: they fit)
__device__ __forceinline__ int counted_answers(const hual_al_set& s, int n) {
  const int v = span_clip_len(s.vlen[n], s.tlen[n]);
  int c = 0;
  for (int k = s.ap_off[n]; k < s.ap_off[n + 1]; ++k) c += s.ap_idx[k] >= 0 && s.ap_idx[k] < v;
  return c;
}

__global__ __launch_bounds__(CALIB_FOLD_THREADS) void al_evidence_fold_kernel(AlGridArgs a) {
  __shared__ double smd[3 * (CALIB_FOLD_THREADS / 64)];
  const int c = blockIdx.x, t = threadIdx.x, AB = a.A * a.B;
  double sum = 0.0, rows = 0.0, answers = 0.0, excluded = 0.0;      // (the counts as float64: exact far beyond 2^31)
  for (int k = t; k < a.nsel; k += CALIB_FOLD_THREADS) {
    const int n = a.sel ? a.sel[k] : k;
    if (n < 0 || n >= a.in.set.N) continue;
    if (a.status[n] == 1) {
      sum += a.table[(size_t)n * AB + c];
      if (c == 0) { rows += 1.0; answers += (double)counted_answers(a.in.set, n); }
    } else if (c == 0) {
      excluded += 1.0;
    }
  }
  sum = block_reduce<BlockSumD, CALIB_FOLD_THREADS / 64>(sum, smd);
  if (t == 0) a.total[c] = sum;
  if (c == 0) {                             // (uniform)
    block_reduce<BlockSumD, CALIB_FOLD_THREADS / 64>(rows, answers, excluded, smd);
    if (t == 0) { a.counts[0] = (int)rows; a.counts[1] = (int)answers; a.counts[2] = (int)excluded; }
  }
}

__global__ __launch_bounds__(64) void al_evidence_best_kernel(AlGridArgs a) {
  const int AB = a.A * a.B;
  double best = -INFINITY;
  int at = 0x7fffffff;
  FirstIndexMax better;
  for (int c = threadIdx.x; c < AB; c += 64) {
    const double x = a.total[c];
    if (better(x, c, best, at)) { best = x; at = c; }
  }
  wave_best(best, at);
  if (threadIdx.x == 0) a.counts[3] = (a.counts[0] > 0 && at < AB) ? at : -1;
}

}  // namespace

namespace hual {

int launch_al_evidence_grid(const AlGridArgs& a, hipStream_t s) {
  const int AB = a.A * a.B;
  // per selected sample: two rows of logits in, the row of cells out; the fold reads every cell once
  HUAL_LAUNCH(0.0, (8.0 * a.in.set.ld + 8.0 * AB + 4.0) * a.nsel, al_evidence_grid_kernel, dim3(a.nsel), dim3(SPAN_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  HUAL_LAUNCH(0.0, (8.0 * AB + 4.0) * a.nsel + 8.0 * AB, al_evidence_fold_kernel, dim3(AB), dim3(CALIB_FOLD_THREADS), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  HUAL_LAUNCH(0.0, 8.0 * AB + 8.0, al_evidence_best_kernel, dim3(1), dim3(64), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

extern "C" int hual_al_evidence_grid(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel,
                                     const float* inv_tau, int A, const float* eps, int B, double* table, int32_t* status,
                                     double* total, int32_t* counts, void* stream) {
  HUAL_REQUIRE(set, "hual_al_evidence_grid: null set");
  AlGridArgs a{};
  a.in.set = *set; a.in.s0 = s0; a.in.e0 = e0;
  const int rc = check_span_in(a.in, "al_evidence_grid", [&] {
    HUAL_REQUIRE(inv_tau && eps, "al_evidence_grid: null grid");
    HUAL_REQUIRE(table && status && total && counts, "al_evidence_grid: null output");
    HUAL_REQUIRE(nsel >= 1, "al_evidence_grid: nsel >= 1");
    return 0;
  });
  if (rc) return rc;
  HUAL_REQUIRE(A >= 1 && A <= CALIB_MAX_TAU, "al_evidence_grid: A in [1, 32]");
  HUAL_REQUIRE(B >= 1 && B <= CALIB_MAX_EPS, "al_evidence_grid: B in [1, 16]");
  for (int i = 0; i < A; ++i) {
    HUAL_REQUIRE(inv_tau[i] > 0.f && inv_tau[i] < INFINITY, "al_evidence_grid: inv_tau finite and > 0");      // (a NaN fails the comparison)
    a.inv_tau[i] = inv_tau[i];
  }
  for (int i = 0; i < B; ++i) {
    HUAL_REQUIRE(eps[i] > 0.f && eps[i] <= 0.5f, "al_evidence_grid: eps in (0, 0.5]");
    const double de = (double)eps[i];
    a.lnr[i] = std::log((1.0 - de) / de); a.ln_eps[i] = std::log(de); a.ln_1meps[i] = std::log1p(-de);
  }
  a.sel = sel; a.nsel = sel ? nsel : set->N;      // without a list every sample is selected
  a.A = A; a.B = B;
  a.table = table; a.status = status; a.total = total; a.counts = counts;
  return launch_al_evidence_grid(a, (hipStream_t)stream);
}
