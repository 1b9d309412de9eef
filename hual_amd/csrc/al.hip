// Active-learning label update on the GPU: the per-sample scoring of /root/reference/update_label.py:125-169
// (get_uncert_rank) and the pseudo-label re-derivation of :85-123 (renew_label), with their helpers from
// /root/reference/utils/utils_hual.py (fill_isactivate :37-59, get_segment :63-76, center_width_gauss :79-89,
// get_distance_score(_shift) :92-124, get_uncert_model :144-161).  The reference walks the training set sample by sample
// in Python (and re-sorts inside the loop); here one workgroup owns one sample, the whole training set is one launch.
//
// Arithmetic types follow numpy's in the reference, because the results are argmax indices:
//   * gaussians: float32 on the float32 grid np.linspace(-1, 1, T) (python scalars are weak operands -> cast to f32),
//     normalised by their maximum over ALL T grid points, then scaled by width/vlen;
//   * model uncertainty: float32 sigmoid differences; probabilities: float32 1/(1+exp(-x));
//   * score mixtures / uncert_frame: float64 sums of float32 terms.
// Active points arrive as one CSR list per sample (frame index + positive flag), in the order they were annotated.
#include "al.h"
#include "prof.h"

using namespace hual;

#define AL_THREADS 256
#define AL_MAX_SEG 64
#define AL_WAVES (AL_THREADS / 64)

namespace {

struct ApInfo {
  int npos, nneg;
  int lo, hi;          // hull of the positive points
  int negL, negR;      // nearest negative left of lo (-1: none) / right of hi (INT_MAX: none)
};

__device__ __forceinline__ ApInfo scan_ap(const int32_t* idx, const int8_t* pos, int n) {
  ApInfo a;
  a.npos = 0; a.nneg = 0; a.lo = 0x7fffffff; a.hi = -1; a.negL = -1; a.negR = 0x7fffffff;
  for (int k = 0; k < n; ++k) {
    if (pos[k]) { ++a.npos; a.lo = min(a.lo, idx[k]); a.hi = max(a.hi, idx[k]); }
    else ++a.nneg;
  }
  if (a.npos > 0) {
    for (int k = 0; k < n; ++k) {
      if (pos[k]) continue;
      if (idx[k] < a.lo) a.negL = max(a.negL, idx[k]);
      if (idx[k] > a.hi) a.negR = min(a.negR, idx[k]);
    }
  }
  return a;
}

// fill_isactivate (utils_hual.py:37-59) evaluated at frame t
__device__ __forceinline__ int isactive_at(const ApInfo& a, const int32_t* idx, const int8_t* pos, int n, int t, int vlen) {
  if (t >= vlen) return -100;
  if (a.npos > 0) {
    if (t <= a.negL || t >= a.negR) return -1;
    return (t >= a.lo && t <= a.hi) ? 1 : 0;
  }
  for (int k = 0; k < n; ++k)
    if (!pos[k] && idx[k] == t) return -1;
  return 0;
}

// grid point t of np.linspace(-1, 1, T, dtype=float32): float64 arange * step + start, last point = stop, then cast
__device__ __forceinline__ float grid_x(int t, int T) {
  if (t == T - 1) return 1.0f;
  const double step = 2.0 / (double)(T - 1);
  return (float)((double)t * step + (-1.0));
}

// center_width_gauss (utils_hual.py:79-89) for all T frames into out[] (LDS).  Block-uniform call.
__device__ void gauss_block(double center, double width, int vlen, int T, float* out, float* red) {
  double sig = (double)vlen / (double)T;
  sig *= width / (double)vlen * 0.4;
  const double u = (center / (double)(T - 1)) * 2.0 - 1.0;
  const float uf = (float)u;
  const float den = (float)(2.0 * (sig * sig));
  const float nrm = (float)(sqrt(2.0 * 3.141592653589793) * sig);
  const float peak = (float)(width / (double)vlen);
  float mx = -1.0f;
  for (int t = threadIdx.x; t < T; t += AL_THREADS) {
    const float d = grid_x(t, T) - uf;
    const float w = expf(-(d * d) / den) / nrm;
    out[t] = w;
    mx = fmaxf(mx, w);
  }
  mx = block_reduce<BlockMaxF, AL_WAVES>(mx, red);
  for (int t = threadIdx.x; t < T; t += AL_THREADS) out[t] = t < vlen ? (out[t] / mx) * peak : 0.0f;
  __syncthreads();
}

// get_segment (utils_hual.py:63-76): maximal runs of isactive == 0, found by one thread (T <= 1024, a few hundred cycles)
__device__ void find_segments(const ApInfo& a, const int32_t* idx, const int8_t* pos, int n, int vlen, int T, int* seg,
                              int* nseg) {
  if (threadIdx.x == 0) {
    int k = 0, start = -1;
    for (int t = 0; t <= T; ++t) {
      const int v = t < T ? isactive_at(a, idx, pos, n, t, vlen) : -100;
      if (v == 0 && start < 0) start = t;
      else if (v != 0 && start >= 0) {
        if (k < AL_MAX_SEG) { seg[2 * k] = start; seg[2 * k + 1] = t - 1; ++k; }
        start = -1;
      }
    }
    *nseg = k;
  }
  __syncthreads();
}

// get_distance_score / one half of get_distance_score_shift: dist[t] (float32 values) for center shifted by
// width*shift/2 (shift = 0: utils_hual.py:92-103)
__device__ void distance_block(const int* seg, int nseg, double shift, int vlen, int T, float* dist, float* tmp, float* red) {
  for (int t = threadIdx.x; t < T; t += AL_THREADS) dist[t] = 0.0f;
  __syncthreads();
  for (int s = 0; s < nseg; ++s) {
    const int a = seg[2 * s], b = seg[2 * s + 1];
    const double width = (double)(b - a + 1);
    const double center = (double)(b - a) / 2.0 + (double)a + width * shift / 2.0;
    gauss_block(center, width, vlen, T, tmp, red);
    for (int t = a + (int)threadIdx.x; t <= b; t += AL_THREADS) dist[t] = tmp[t];
    __syncthreads();
  }
}

__device__ __forceinline__ float sigmoid_np(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace

// ------------------------------------------------------------------------------------------------------
// get_uncert_rank body (update_label.py:125-169) for one sample per block
// ------------------------------------------------------------------------------------------------------
namespace {

// the model-uncertainty term of frame i = row + t, by its source
template <AlSource SRC>
__device__ __forceinline__ float model_uncert(const AlScoreArgs& a, size_t i) {
  if constexpr (SRC == AL_SRC_PAIR) {
    // the two stochastic passes' logits (get_uncert_model, utils_hual.py:144-161)
    return fabsf(sigmoid_np(a.s1[i]) - sigmoid_np(a.s2[i])) + fabsf(sigmoid_np(a.e1[i]) - sigmoid_np(a.e2[i]));
  } else if constexpr (SRC == AL_SRC_SPREAD) {
    // the bank of K folded passes.  RANGE at K = 2 is the expression above bit for bit: hi - lo = fmaxf(p1, p2) - fminf(p1, p2) is the
    // same subtraction as |p1 - p2| up to its sign.  STD is sqrt(2) times the sample deviation (ddof = 1): |p1 - p2| at K = 2 up to
    // rounding, and of an expectation that does not grow with K.
    if (a.stat == HUAL_AL_STAT_RANGE) return (a.hi[0][i] - a.lo[0][i]) + (a.hi[1][i] - a.lo[1][i]);
    return sqrtf(2.0f) * (sqrtf(a.m2[0][i] / a.km1) + sqrtf(a.m2[1][i] / a.km1));
  } else {
    // the bank's mean probability and the mean entropy of the passes beside it (hual_al_info), in bits per head: total (ENTROPY) =
    // epistemic (BALD, the mutual information) + aleatoric (EXPECTED_ENTROPY).  Jensen keeps BALD >= 0 in exact arithmetic; the clamp
    // only removes negative rounding residue.
    if (a.stat == HUAL_AL_STAT_EXPECTED_ENTROPY) return a.ent[0][i] + a.ent[1][i];
    const float hs = h2_bits(a.mean[0][i]), he = h2_bits(a.mean[1][i]);
    if (a.stat == HUAL_AL_STAT_ENTROPY) return hs + he;
    return fmaxf(0.0f, hs - a.ent[0][i]) + fmaxf(0.0f, he - a.ent[1][i]);
  }
}

// the term itself for the caller (McBank.uncert); the pair form has no such output
template <AlSource SRC>
__device__ __forceinline__ void keep_uncert(const AlScoreArgs& a, size_t i, float um) {
  if constexpr (SRC != AL_SRC_PAIR)
    if (a.uncert_model) a.uncert_model[i] = um;
}

}  // namespace

template <AlSource SRC>
__global__ __launch_bounds__(AL_THREADS) void al_score_kernel(AlScoreArgs a) {
  extern __shared__ float lds[];            // dist[T] | tmp[T]
  __shared__ float red[AL_WAVES];
  __shared__ double redd[AL_WAVES];
  __shared__ double vs[AL_WAVES];
  __shared__ int redi[AL_WAVES];
  __shared__ int seg[2 * AL_MAX_SEG];
  __shared__ int nseg;
  const int n = blockIdx.x;
  const int T = a.set.tlen[n], V = a.set.vlen[n];
  float* dist = lds;
  float* tmp = lds + a.set.ld;
  const int ap0 = a.set.ap_off[n], napn = a.set.ap_off[n + 1] - ap0;
  const int32_t* aidx = a.set.ap_idx + ap0;
  const int8_t* apos = a.set.ap_pos + ap0;
  const ApInfo ap = scan_ap(aidx, apos, napn);
  find_segments(ap, aidx, apos, napn, V, T, seg, &nseg);
  distance_block(seg, nseg, 0.0, V, T, dist, tmp, red);

  const size_t row = (size_t)n * a.set.ld;
  double vsum = 0.0;
  double best = -1.0;
  int besti = 0x7fffffff;
  for (int t = threadIdx.x; t < T; t += AL_THREADS) {
    a.sprob[row + t] = sigmoid_np(a.s0[row + t]);
    a.eprob[row + t] = sigmoid_np(a.e0[row + t]);
    float um = 0.0f;
    if (t < V)
      um = model_uncert<SRC>(a, row + t);
    keep_uncert<SRC>(a, row + t, um);
    vsum += (double)um;
    const double uf = (double)dist[t] + (double)(um * a.coff_uncert);
    a.uncert_frame[row + t] = uf;
    if (uf > best) { best = uf; besti = t; }       // ascending t per thread: first maximum kept
  }
  // block reduction: argmax of uncert_frame with first-index ties; sum of the model uncertainty, whose barrier publishes both
  wave_best(best, besti);
  if ((threadIdx.x & 63) == 0) { redd[threadIdx.x >> 6] = best; redi[threadIdx.x >> 6] = besti; }
  vsum = block_reduce<BlockSumD, AL_WAVES, false>(vsum, vs);
  if (threadIdx.x == 0) {
    best_of_waves(redd, redi, AL_WAVES, best, besti);
    a.uncert_video[n] = (float)vsum;
    a.observe[n] = besti;
  }
}

// ------------------------------------------------------------------------------------------------------
// One forward's logits folded into the bank: min / max / Welford mean and sum of squared deviations of the per-frame
// probabilities, one workgroup per clip, rows disjoint (no atomics).  Only columns [0, T) of the rows ids[b] are written.
// ------------------------------------------------------------------------------------------------------
namespace {

// Welford's update with every operation rounded on its own: tests/mc_uncert_ref.py restates it in numpy, which never fuses.  What must
// stay unfused: `mean + d / k` (a division, then an add) and above all `m2 + d * (p - mean)` - as an fma the product would enter the sum
// unrounded, and at K = 2 m2 would no longer be the float32 product d * (d / 2) whose root times sqrt(2) is |p1 - p2| to an ulp.
__device__ __forceinline__ void welford_step(float p, float k, float& mean, float& m2) {
#pragma clang fp contract(off)
  const float d = p - mean;
  mean = mean + d / k;
  const float r = p - mean;
  const float q = d * r;
  m2 = m2 + q;
}

// the running mean of the per-pass entropy, rounded like Welford's mean above: a subtraction, a division, an add
__device__ __forceinline__ void mean_step(float x, float k, float& mean) {
#pragma clang fp contract(off)
  const float d = x - mean;
  mean = mean + d / k;
}

}  // namespace

// INFO = false: hual_al_mc_fold, which never reads a.ent; INFO = true: hual_al_mc_fold_info, which also folds the entropy h2(p) of the
// pass into ent - p is computed once and shared
template <bool INFO>
__global__ __launch_bounds__(AL_THREADS) void al_mc_fold_kernel(AlFoldArgs a) {
  const int b = blockIdx.x;
  const int n = a.ids[b];
  if (n < 0 || n >= a.N) return;                      // an id outside the bank writes nothing
  const int V = a.vlen[b];
  const size_t row = (size_t)n * a.ld, src = (size_t)b * a.T;
  if (a.k == 0) {
    for (int t = threadIdx.x; t < a.T; t += AL_THREADS) {
      a.s0[row + t] = a.s[src + t];
      a.e0[row + t] = a.e[src + t];
    }
    if (threadIdx.x == 0) a.tlen[n] = a.T;
    return;
  }
  const float kf = (float)a.k;
  for (int t = threadIdx.x; t < a.T; t += AL_THREADS) {
    const float p[2] = {t < V ? sigmoid_np(a.s[src + t]) : 0.0f, t < V ? sigmoid_np(a.e[src + t]) : 0.0f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (a.k == 1) {
        a.lo[h][row + t] = p[h]; a.hi[h][row + t] = p[h]; a.mean[h][row + t] = p[h]; a.m2[h][row + t] = 0.0f;
      } else {
        float mean = a.mean[h][row + t], m2 = a.m2[h][row + t];
        welford_step(p[h], kf, mean, m2);
        a.lo[h][row + t] = fminf(a.lo[h][row + t], p[h]);
        a.hi[h][row + t] = fmaxf(a.hi[h][row + t], p[h]);
        a.mean[h][row + t] = mean;
        a.m2[h][row + t] = m2;
      }
      if constexpr (INFO) {
        const float e = h2_bits(p[h]);
        if (a.k == 1) {
          a.ent[h][row + t] = e;
        } else {
          float ent = a.ent[h][row + t];
          mean_step(e, kf, ent);
          a.ent[h][row + t] = ent;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// renew_label (update_label.py:85-123) for one selected sample per block
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_renew_kernel(AlRenewArgs a) {
  extern __shared__ float lds[];            // ds[T] | de[T] | tmp[T] | (8-byte aligned) ss[T] | es[T] doubles
  __shared__ float red[AL_WAVES];
  __shared__ double redd[2][AL_WAVES];
  __shared__ int redi[2][AL_WAVES];
  __shared__ int seg[2 * AL_MAX_SEG];
  __shared__ int nseg;
  const int n = a.sel ? a.sel[blockIdx.x] : (int)blockIdx.x;
  const int T = a.set.tlen[n], V = a.set.vlen[n];
  const int ldp = (a.set.ld + 1) & ~1;
  float* ds = lds;
  float* de = lds + ldp;
  float* tmp = lds + 2 * ldp;
  double* ss = reinterpret_cast<double*>(lds + 4 * ldp);
  double* es = ss + ldp;
  const int ap0 = a.set.ap_off[n], napn = a.set.ap_off[n + 1] - ap0;
  const int32_t* aidx = a.set.ap_idx + ap0;
  const int8_t* apos = a.set.ap_pos + ap0;
  const ApInfo ap = scan_ap(aidx, apos, napn);
  const bool has_pos = ap.npos > 0;
  const double a1 = has_pos ? a.coff[0] : a.coff[3];
  const float a2 = (float)(has_pos ? a.coff[1] : a.coff[4]);
  const float a3 = (float)(has_pos ? a.coff[2] : a.coff[5]);
  const double shift = has_pos ? -0.3 : 0.9;
  const size_t row = (size_t)n * a.set.ld;

  find_segments(ap, aidx, apos, napn, V, T, seg, &nseg);
  distance_block(seg, nseg, -shift, V, T, ds, tmp, red);     // start: centre - width*shift/2
  distance_block(seg, nseg, shift, V, T, de, tmp, red);      // end:   centre + width*shift/2
  // score = distance*a1 + prob*a2 + gaussian around the old index * a3   (float64 + float32 + float32)
  gauss_block((double)a.old_idx[2 * n], 0.5 * (double)V, V, T, tmp, red);
  for (int t = threadIdx.x; t < T; t += AL_THREADS)
    ss[t] = ((double)ds[t] * a1 + (double)(a.sprob[row + t] * a2)) + (double)(tmp[t] * a3);
  __syncthreads();
  gauss_block((double)a.old_idx[2 * n + 1], 0.5 * (double)V, V, T, tmp, red);
  for (int t = threadIdx.x; t < T; t += AL_THREADS)
    es[t] = ((double)de[t] * a1 + (double)(a.eprob[row + t] * a2)) + (double)(tmp[t] * a3);
  __syncthreads();

  double bs = -1.0, be = -1.0;
  int bsi = 0x7fffffff, bei = 0x7fffffff;
  if (has_pos) {
    // mask_activepoints, positive branch (update_label.py:69-82), then two plain argmaxes
    for (int t = threadIdx.x; t < T; t += AL_THREADS) {
      double s = ss[t], e = es[t];
      if (t > ap.lo || t <= ap.negL) s = 0.0;
      if (t < ap.hi || t >= ap.negR) e = 0.0;
      if (s > bs) { bs = s; bsi = t; }
      if (e > be) { be = e; bei = t; }
    }
  } else {
    // negative branch: damp around every negative point, then the best span that contains no negative point
    for (int k = 0; k < napn; ++k) {
      gauss_block((double)aidx[k], 0.3 * (double)V, V, T, tmp, red);
      for (int t = threadIdx.x; t < T; t += AL_THREADS) {
        const double m = (double)(1.0f - tmp[t]);
        ss[t] = m * ss[t];
        es[t] = m * es[t];
      }
      __syncthreads();
    }
    for (int t = threadIdx.x; t < T; t += AL_THREADS) {
      double rmax = 0.0, cmax = 0.0;
      bool cut = t >= V;
      int lo = -1, hi = V;                    // nearest cuts around t (update_label.py:113: sorted(neg + [-1, vlen]))
      for (int k = 0; k < napn; ++k) {
        const int c = aidx[k];
        if (c == t) cut = true;
        if (c < t) lo = max(lo, c);
        if (c > t) hi = min(hi, c);
      }
      if (!cut) {
        const double st = ss[t], et = es[t];
        for (int j = t; j < hi; ++j) rmax = fmax(rmax, st * es[j]);
        for (int i = lo + 1; i <= t; ++i) cmax = fmax(cmax, ss[i] * et);
      }
      if (rmax > bs) { bs = rmax; bsi = t; }
      if (cmax > be) { be = cmax; bei = t; }
    }
  }
  wave_best(bs, bsi);
  wave_best(be, bei);
  if ((threadIdx.x & 63) == 0) {
    redd[0][threadIdx.x >> 6] = bs; redi[0][threadIdx.x >> 6] = bsi;
    redd[1][threadIdx.x >> 6] = be; redi[1][threadIdx.x >> 6] = bei;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    best_of_waves(redd[0], redi[0], AL_WAVES, bs, bsi);
    best_of_waves(redd[1], redi[1], AL_WAVES, be, bei);
    a.new_idx[2 * n] = bsi;
    a.new_idx[2 * n + 1] = bei;
  }
}

namespace hual {

int launch_al_score(const AlScoreArgs& a, AlSource src, hipStream_t s) {
  HUAL_REQUIRE(a.s0 && a.e0 && a.set.vlen && a.set.tlen && a.set.ap_off, "al_score: null input");
  if (src == AL_SRC_PAIR) HUAL_REQUIRE(a.s1 && a.e1 && a.s2 && a.e2, "al_score: null input");
  if (src == AL_SRC_SPREAD) {
    HUAL_REQUIRE(a.stat == HUAL_AL_STAT_RANGE || a.stat == HUAL_AL_STAT_STD, "al_score: stat is HUAL_AL_STAT_RANGE or HUAL_AL_STAT_STD");
    for (int h = 0; h < 2; ++h) HUAL_REQUIRE(a.lo[h] && a.hi[h] && a.m2[h], "al_score: null input");
  }
  if (src == AL_SRC_INFO) {
    HUAL_REQUIRE(a.stat == HUAL_AL_STAT_BALD || a.stat == HUAL_AL_STAT_ENTROPY || a.stat == HUAL_AL_STAT_EXPECTED_ENTROPY,
                 "al_score: stat is HUAL_AL_STAT_BALD, HUAL_AL_STAT_ENTROPY or HUAL_AL_STAT_EXPECTED_ENTROPY");
    HUAL_REQUIRE(a.mean[0] && a.mean[1], "al_score: null input");
    HUAL_REQUIRE(a.ent[0] && a.ent[1], "al_score: null info->ent_s or info->ent_e");
  }
  HUAL_REQUIRE(a.sprob && a.eprob && a.uncert_frame && a.uncert_video && a.observe, "al_score: null output");
  HUAL_REQUIRE(a.set.N > 0 && a.set.ld >= 2 && a.set.ld <= HUAL_AL_MAX_T, "al_score: need N > 0 and 2 <= ld <= 1024");
  const dim3 grid(a.set.N), block(AL_THREADS);
  const size_t lds = 2 * a.set.ld * sizeof(float);
  // per frame: the pair form reads six logits, the bank forms up to eight (and may write the term)
  switch (src) {
    case AL_SRC_PAIR: HUAL_LAUNCH(0.0, 40.0 * a.set.N * a.set.ld, al_score_kernel<AL_SRC_PAIR>, grid, block, lds, s, a); break;
    case AL_SRC_SPREAD: HUAL_LAUNCH(0.0, 44.0 * a.set.N * a.set.ld, al_score_kernel<AL_SRC_SPREAD>, grid, block, lds, s, a); break;
    case AL_SRC_INFO: HUAL_LAUNCH(0.0, 44.0 * a.set.N * a.set.ld, al_score_kernel<AL_SRC_INFO>, grid, block, lds, s, a); break;
  }
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

// with a.ent set the launch also folds the passes' entropy: per frame one more store per head at k = 1, one more load and store per head
// at k >= 2
int launch_al_mc_fold(const AlFoldArgs& a, hipStream_t s) {
  HUAL_REQUIRE(a.ids && a.vlen && a.s && a.e, "al_mc_fold: null input");
  HUAL_REQUIRE(a.tlen && a.s0 && a.e0, "al_mc_fold: null bank");
  for (int h = 0; h < 2; ++h) HUAL_REQUIRE(a.lo[h] && a.hi[h] && a.mean[h] && a.m2[h], "al_mc_fold: null bank");
  HUAL_REQUIRE(!a.ent[0] == !a.ent[1], "al_mc_fold: ent_s and ent_e are both set or both null");
  HUAL_REQUIRE(a.N > 0 && a.ld >= 2 && a.ld <= HUAL_AL_MAX_T, "al_mc_fold: need N > 0 and 2 <= ld <= 1024");
  HUAL_REQUIRE(a.B > 0 && a.T >= 2 && a.T <= a.ld, "al_mc_fold: need B > 0 and 2 <= T_b <= ld");
  HUAL_REQUIRE(a.k >= 0, "al_mc_fold: pass index k >= 0");
  const dim3 grid(a.B), block(AL_THREADS);
  if (a.ent[0])
    HUAL_LAUNCH(0.0, (a.k == 0 ? 16.0 : a.k == 1 ? 48.0 : 88.0) * a.B * a.T, al_mc_fold_kernel<true>, grid, block, 0, s, a);
  else
    HUAL_LAUNCH(0.0, (a.k == 0 ? 16.0 : a.k == 1 ? 40.0 : 72.0) * a.B * a.T, al_mc_fold_kernel<false>, grid, block, 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_al_renew(const AlRenewArgs& a, int nsel, hipStream_t s) {
  HUAL_REQUIRE(a.sprob && a.eprob && a.set.vlen && a.set.tlen && a.set.ap_off && a.old_idx && a.new_idx, "al_renew: null pointer");
  HUAL_REQUIRE(a.set.ld >= 2 && a.set.ld <= HUAL_AL_MAX_T, "al_renew: need 2 <= ld <= 1024");
  if (nsel <= 0) return 0;
  const int ldp = (a.set.ld + 1) & ~1;
  HUAL_LAUNCH(0.0, 16.0 * nsel * a.set.ld, al_renew_kernel, dim3(nsel), dim3(AL_THREADS), 4 * ldp * sizeof(float) + 2 * ldp * sizeof(double),
              s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

namespace {

// the set, the deterministic logits and the outputs of every hual_al_score* entry point
AlScoreArgs score_args(const hual_al_set* set, const float* s0, const float* e0, float coff_uncert, float* sprob, float* eprob,
                              double* uncert_frame, float* uncert_video, int32_t* observe_point) {
  AlScoreArgs a{};
  a.set = *set; a.s0 = s0; a.e0 = e0; a.coff_uncert = coff_uncert;
  a.sprob = sprob; a.eprob = eprob; a.uncert_frame = uncert_frame; a.uncert_video = uncert_video; a.observe = observe_point;
  return a;
}

// the bank's per-head statistics into the arguments of a score (read) or of a fold (written)
template <class Args>
void bank_stats(Args& a, const hual_al_bank* bank) {
  a.lo[0] = bank->lo_s; a.hi[0] = bank->hi_s; a.mean[0] = bank->mean_s; a.m2[0] = bank->m2_s;
  a.lo[1] = bank->lo_e; a.hi[1] = bank->hi_e; a.mean[1] = bank->mean_e; a.m2[1] = bank->m2_e;
}

}  // namespace

extern "C" {

int hual_al_score(const hual_al_set* set, const float* s0, const float* e0, const float* s1, const float* e1,
                  const float* s2, const float* e2, float coff_uncert, float* sprob, float* eprob, double* uncert_frame,
                  float* uncert_video, int32_t* observe_point, void* stream) {
  HUAL_REQUIRE(set, "hual_al_score: null set");
  AlScoreArgs a = score_args(set, s0, e0, coff_uncert, sprob, eprob, uncert_frame, uncert_video, observe_point);
  a.s1 = s1; a.e1 = e1; a.s2 = s2; a.e2 = e2;
  return launch_al_score(a, AL_SRC_PAIR, (hipStream_t)stream);
}

int hual_al_score_mc(const hual_al_set* set, const float* s0, const float* e0, const hual_al_bank* bank, int K, int stat,
                     float coff_uncert, float* sprob, float* eprob, double* uncert_frame, float* uncert_video,
                     int32_t* observe_point, float* uncert_model, void* stream) {
  HUAL_REQUIRE(set && bank, "hual_al_score_mc: null pointer");
  HUAL_REQUIRE(K >= 2, "hual_al_score_mc: K >= 2 stochastic passes (one sample has no spread)");
  HUAL_REQUIRE(bank->N == set->N && bank->ld == set->ld, "hual_al_score_mc: bank and set differ in N or ld");
  AlScoreArgs a = score_args(set, s0, e0, coff_uncert, sprob, eprob, uncert_frame, uncert_video, observe_point);
  bank_stats(a, bank);
  a.stat = stat; a.km1 = (float)(K - 1); a.uncert_model = uncert_model;
  return launch_al_score(a, AL_SRC_SPREAD, (hipStream_t)stream);
}

int hual_al_score_info(const hual_al_set* set, const float* s0, const float* e0, const hual_al_bank* bank, const hual_al_info* info,
                       int K, int stat, float coff_uncert, float* sprob, float* eprob, double* uncert_frame, float* uncert_video,
                       int32_t* observe_point, float* uncert_model, void* stream) {
  HUAL_REQUIRE(set && bank, "hual_al_score_info: null pointer");
  HUAL_REQUIRE(info, "hual_al_score_info: null info");
  HUAL_REQUIRE(K >= (stat == HUAL_AL_STAT_BALD ? 2 : 1),
               "hual_al_score_info: K >= 2 stochastic passes for BALD (one sample has no disagreement), K >= 1 for the entropies");
  HUAL_REQUIRE(bank->N == set->N && bank->ld == set->ld, "hual_al_score_info: bank and set differ in N or ld");
  AlScoreArgs a = score_args(set, s0, e0, coff_uncert, sprob, eprob, uncert_frame, uncert_video, observe_point);
  bank_stats(a, bank);
  a.ent[0] = info->ent_s; a.ent[1] = info->ent_e;
  a.stat = stat; a.uncert_model = uncert_model;
  return launch_al_score(a, AL_SRC_INFO, (hipStream_t)stream);
}

static int fold(const hual_al_bank* bank, const hual_al_info* info, const int32_t* ids, const int32_t* v_len, const float* start_logits,
                const float* end_logits, int B, int T_b, int k, void* stream) {
  AlFoldArgs a{};
  a.ids = ids; a.vlen = v_len; a.s = start_logits; a.e = end_logits; a.B = B; a.T = T_b; a.k = k;
  a.ld = bank->ld; a.N = bank->N; a.tlen = bank->tlen; a.s0 = bank->s0; a.e0 = bank->e0;
  bank_stats(a, bank);
  if (info) { a.ent[0] = info->ent_s; a.ent[1] = info->ent_e; }
  return launch_al_mc_fold(a, (hipStream_t)stream);
}

int hual_al_mc_fold(const hual_al_bank* bank, const int32_t* ids, const int32_t* v_len, const float* start_logits,
                    const float* end_logits, int B, int T_b, int k, void* stream) {
  HUAL_REQUIRE(bank, "hual_al_mc_fold: null bank");
  return fold(bank, nullptr, ids, v_len, start_logits, end_logits, B, T_b, k, stream);
}

// a null array must never turn this call into a plain fold: refused here, before launch_al_mc_fold chooses by a.ent
int hual_al_mc_fold_info(const hual_al_bank* bank, const hual_al_info* info, const int32_t* ids, const int32_t* v_len,
                         const float* start_logits, const float* end_logits, int B, int T_b, int k, void* stream) {
  HUAL_REQUIRE(bank, "hual_al_mc_fold_info: null bank");
  HUAL_REQUIRE(info, "hual_al_mc_fold_info: null info");
  HUAL_REQUIRE(info->ent_s && info->ent_e, "hual_al_mc_fold_info: null info->ent_s or info->ent_e");
  return fold(bank, info, ids, v_len, start_logits, end_logits, B, T_b, k, stream);
}

int hual_al_renew(const hual_al_set* set, const int32_t* sel, int nsel, const float* sprob, const float* eprob,
                  const int32_t* old_idx, const double* coff6, int32_t* new_idx, void* stream) {
  HUAL_REQUIRE(set && coff6, "hual_al_renew: null pointer");
  AlRenewArgs a{};
  a.sel = sel; a.sprob = sprob; a.eprob = eprob; a.set = *set; a.old_idx = old_idx; a.new_idx = new_idx;
  for (int k = 0; k < 6; ++k) a.coff[k] = coff6[k];
  return launch_al_renew(a, sel ? nsel : set->N, (hipStream_t)stream);
}

}  // extern "C"
