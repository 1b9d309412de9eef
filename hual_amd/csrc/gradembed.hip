// hual_al_grad_embed (include/hual_seqpan.h): the gradient embedding of every (clip, query) sample of a batch for batch-mode
// acquisition (BADGE, Ash et al. 2020) - the gradient of the localizing loss with respect to the start_dense / end_dense kernels under
// a hypothesised span, g = sum_t (p(t) - y(t)) h(t) per head, its squared length, and the expected squared gradient length under
// y ~ p, sum_t p(t) |h(t) - mu|^2 with mu = sum_t p(t) h(t).  Read-only on the forward: head.hs / head.he and the logits as the
// label-free forward left them.
//
// One workgroup of 256 threads per sample: thread (head, column) = (tid >> 7, tid & 127).  The probabilities are span_probabilities'
// (spanprob.h, one body, NW = 4: the same bits as every span launch) and sit in LDS; a thread then walks the clip's frames in
// ascending t, so the 128 threads of a head read one h row as one 512-byte segment.  Two passes: mu and g in float32, then
// p (h - mu)^2 - the second read of the rows is served from L2 -, never E|h|^2 - |mu|^2.  The squares are taken and summed in float64:
// per wave by wave_sum64_f64_desc, the four waves in ascending order (block_reduce).  No atomics, nothing grid wide.
#include "common.h"
#include "prof.h"
#include "spanprob.h"

namespace {

constexpr int GE_THREADS = 256;
constexpr int GE_WAVES = GE_THREADS / 64;
constexpr int GE_H = 128;            // columns of head.hs / head.he

struct GeArgs {
  const float* hs;
  const float* he;
  const float* zs;
  const float* ze;
  const int32_t* v_len;
  const int32_t* hyp;
  const int32_t* rows;               // null: sample b writes row b
  int N, T, ld, ld_desc;
  float* desc;
  float* gnorm2;
  float* egl;
};

__global__ __launch_bounds__(GE_THREADS) void grad_embed_kernel(GeArgs a) {
  __shared__ float ps[256], pe[256], smf[2 * GE_WAVES];
  __shared__ double smd[2 * GE_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int row = a.rows ? a.rows[b] : b;
  if (row < 0 || row >= a.N) return;                         // (workgroup-uniform) a foreign id writes nothing
  const int v = span_clip_len(a.v_len[b], a.T);
  const size_t zrow = (size_t)b * a.ld;
  // the poison rule of the span family, widened to every non-finite logit among the clip's frames (x - x is 0 for a finite x only)
  const bool bad = tid < v && ((a.zs[zrow + tid] - a.zs[zrow + tid]) != 0.f || (a.ze[zrow + tid] - a.ze[zrow + tid]) != 0.f);
  if (__syncthreads_or(bad) || v < 1) {
    a.desc[(size_t)row * a.ld_desc + tid] = __builtin_nanf("");
    if (tid == 0) { a.gnorm2[row] = -1.f; a.egl[row] = -1.f; }
    return;
  }
  span_probabilities_of<GE_WAVES>([&] { return a.zs[zrow + tid]; }, [&] { return a.ze[zrow + tid]; }, a.T, v, ps, pe, smf, smd);
  const int head = tid >> 7, col = tid & (GE_H - 1);
  const float* p = head ? pe : ps;
  const float* h = (head ? a.he : a.hs) + (size_t)b * a.T * GE_H + col;
  const int y = a.hyp[2 * b + head];                         // outside [0, v): no label for this head, g = mu
  float mu = 0.f, g = 0.f;
  for (int t = 0; t < v; ++t) {
    const float pt = p[t], ht = h[(size_t)t * GE_H];
    mu = __fmaf_rn(pt, ht, mu);
    g = __fmaf_rn(t == y ? pt - 1.f : pt, ht, g);
  }
  double e = 0.0;
  for (int t = 0; t < v; ++t) {
    const double d = (double)(h[(size_t)t * GE_H] - mu);
    e += (double)p[t] * (d * d);
  }
  double n2 = (double)g * (double)g;
  block_reduce<BlockSumD, GE_WAVES>(n2, e, smd);
  a.desc[(size_t)row * a.ld_desc + tid] = g;
  if (tid == 0) { a.gnorm2[row] = (float)n2; a.egl[row] = (float)e; }
}

}  // namespace

extern "C" int hual_al_grad_embed(const float* hs, const float* he, const float* s_logits, const float* e_logits, const int32_t* v_len,
                                  const int32_t* hyp, const int32_t* rows, int B, int T, int ld, int N, float* desc, int ld_desc,
                                  float* gnorm2, float* egl, void* stream) {
  HUAL_REQUIRE(hs && he && s_logits && e_logits && v_len && hyp && desc && gnorm2 && egl,
               "hual_al_grad_embed: null pointer (hs, he, s_logits, e_logits, v_len, hyp, desc, gnorm2, egl)");
  HUAL_REQUIRE(B >= 1 && N >= 1, "hual_al_grad_embed: B >= 1 and N >= 1");
  HUAL_REQUIRE(T >= 1 && T <= 256, "hual_al_grad_embed: 1 <= T <= 256");
  HUAL_REQUIRE(ld >= T && ld <= 1024, "hual_al_grad_embed: T <= ld <= 1024");
  HUAL_REQUIRE(ld_desc >= 2 * GE_H, "hual_al_grad_embed: ld_desc >= 256");
  GeArgs a{hs, he, s_logits, e_logits, v_len, hyp, rows, N, T, ld, ld_desc, desc, gnorm2, egl};
  HUAL_LAUNCH(8.0 * B * T * 2 * GE_H, 4.0 * B * (2.0 * T * GE_H + 2.0 * T + 2 * GE_H), grad_embed_kernel, dim3(B), dim3(GE_THREADS), 0,
              (hipStream_t)stream, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}
