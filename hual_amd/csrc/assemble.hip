// Device-side batch assembly: what TrainLoader.process_batch (/root/reference/utils/data_loader.py:30-98) and
// pad_seq / pad_char_seq / pad_video_seq (/root/reference/utils/data_utils.py:130-172) do with numpy per step, from a
// training set that stays RESIDENT in HBM (Charades: 12.4 k clips x 64 x 1024 fp32 = 3.2 GB of the 288 GB).  The host
// only picks the sample ids of the batch and its padded sizes (T, L, C = maxima of lengths it already knows).
// ONE launch (round 5: two launches + the caller's copy of the previous step's spans were three eager operations between two
// replayed step graphs, ~13 us of idle device each - the epoch loop ran at 0.938 of the resident-batch rate for 26 us of kernels):
//   blocks [0, B)      : one block per sample - word ids, char ids, lengths, soft start/end labels, 4-class match
//                        labels, inner labels (bit exact with the reference's float32 results)
//   block  B           : optional carry - copies `carry_n` 8-byte words (the spans the PREVIOUS step left in its fetch buffer) to
//                        their place in the caller's epoch-long bank
//   blocks (B, ..)     : [B,T,V] zero-padded gather of the feature rows (HBM bound: reads the valid rows once, writes B*T*V floats
//                        once, 16-byte accesses)
#include "assemble.h"
#include "prof.h"

using namespace hual;

__device__ __forceinline__ void assemble_video_body(const AssembleArgs& a, int blk, int nblk) {
  const int v4 = a.vdim >> 2;
  const size_t total = (size_t)a.B * a.T * v4;
  const int32_t* sel = a.cursor ? a.sel + a.cursor[0] : a.sel;
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)nblk * blockDim.x) {
    const int c = (int)(i % v4);
    const size_t r = i / v4;
    const int t = (int)(r % a.T), b = (int)(r / a.T);
    const int vid = a.sample_vid[sel[b]];
    const int64_t r0 = a.feat_off[vid];
    const int n = (int)(a.feat_off[vid + 1] - r0);
    float4 v = f4zero();
    if (t < n) v = ld4(a.feat_bank + (size_t)(r0 + t) * a.vdim + 4 * c);
    st4(a.video + r * a.vdim + 4 * c, v);
  }
}

__device__ __forceinline__ void assemble_side_body(const AssembleArgs& a, int b) {
  const int s = (a.cursor ? a.sel + a.cursor[0] : a.sel)[b];
  const int vid = a.sample_vid[s];
  const int n = (int)(a.feat_off[vid + 1] - a.feat_off[vid]);
  if (threadIdx.x == 0) a.lens[b] = n;
  // ---- word / char ids, 0 = PAD (data_utils.py:130-155)
  const int w0 = a.word_off[s], nw = a.word_off[s + 1] - w0;
  for (int l = threadIdx.x; l < a.L; l += blockDim.x) a.word_ids[(size_t)b * a.L + l] = l < nw ? a.word_bank[w0 + l] : 0;
  for (int i = threadIdx.x; i < a.L * a.C; i += blockDim.x) {
    const int l = i / a.C, c = i % a.C;
    int v = 0;
    if (l < nw) {
      const int c0 = a.char_off[w0 + l], nc = a.char_off[w0 + l + 1] - c0;
      if (c < nc) v = a.char_bank[c0 + c];
    }
    a.char_ids[(size_t)b * a.L * a.C + i] = v;
  }
  if (!a.y1) return;            // test batches carry no labels (data_loader.py:145-164)
  // ---- labels (data_loader.py:55-94)
  const int st = a.s_ind[s], et = a.e_ind[s];
  const float yf = (float)((1.0 - (double)n * 1e-10 - 0.5) / 2.0);     // python double, stored into a float32 array
  const int ext = 2;
  const int st_l = max(0, st - ext);
  int st_r = min(st + ext, n - 1);
  const int et_l = max(0, et - ext);
  const int et_r = min(et + ext, n - 1);
  if (st_r >= et_l) st_r = max(st, et_l - 1);
  // the sample's soft-label weight: 0 (or no banks) leaves the reference's labels untouched, and its bank rows unread
  const float lam = a.soft_w ? a.soft_w[s] : 0.f;
  const int nsoft = lam == 0.f ? 0 : min(n, a.soft_ld);
  for (int t = threadIdx.x; t < a.T; t += blockDim.x) {
    const float base = t < n ? 1e-10f : 0.0f;
    float ys = base, ye = base;
    if (t == st) {
      ys = ys + 0.5f;
      if (st == 0) ys = ys + yf;
      if (st >= n - 1) ys = ys + yf;
    } else if ((t == st - 1) || (t == st + 1 && st < n - 1)) {
      ys = yf;
    }
    if (t == et) {
      ye = ye + 0.5f;
      if (et == 0) ye = ye + yf;
      if (et >= n - 1) ye = ye + yf;
    } else if ((t == et - 1) || (t == et + 1 && et < n - 1)) {
      ye = yf;
    }
    if (t < nsoft) {            // three float32 operations, each rounded on its own (no contraction)
      const size_t so = (size_t)s * a.soft_ld + t;
      ys = __fadd_rn(ys, __fmul_rn(lam, __fsub_rn(a.soft_y1[so], ys)));
      ye = __fadd_rn(ye, __fmul_rn(lam, __fsub_rn(a.soft_y2[so], ye)));
    }
    // later writes win: B-M (1), then I-M (2) + inner, then E-M (3)
    int m = 0, in = 0;
    if (t >= st_l && t <= st_r) m = 1;
    if (t > st_r && t < et_l) { m = 2; in = 1; }
    if (t >= et_l && t <= et_r) m = 3;
    const size_t o = (size_t)b * a.T + t;
    a.y1[o] = ys;
    a.y2[o] = ye;
    a.match[o] = m;
    a.inner[o] = (float)in;
  }
}

__global__ __launch_bounds__(256) void assemble_kernel(AssembleArgs a) {
  const int blk = blockIdx.x;
  if (blk < a.B) { assemble_side_body(a, blk); return; }
  if (blk == a.B) {
    for (int i = threadIdx.x; i < a.carry_n; i += blockDim.x) a.carry_dst[i] = a.carry_src[i];
    return;
  }
  assemble_video_body(a, blk - a.B - 1, (int)gridDim.x - a.B - 1);
}

namespace hual {

int launch_assemble(const AssembleArgs& a, hipStream_t s) {
  HUAL_REQUIRE(a.feat_bank && a.feat_off && a.sample_vid && a.word_off && a.word_bank && a.char_off && a.char_bank && a.sel,
               "assemble: null dataset pointer");
  HUAL_REQUIRE(a.video && a.lens && a.word_ids && a.char_ids, "assemble: null output pointer");
  HUAL_REQUIRE(a.B > 0 && a.T > 0 && a.L > 0 && a.C > 0 && a.vdim > 0 && a.vdim % 4 == 0, "assemble: bad shape");
  HUAL_REQUIRE(!a.y1 || (a.y2 && a.match && a.inner && a.s_ind && a.e_ind), "assemble: labels need y1, y2, match, inner, s_ind, e_ind");
  HUAL_REQUIRE(!a.soft_w || (a.soft_y1 && a.soft_y2 && a.soft_ld >= 1), "assemble: soft labels need y1, y2, w and ld >= 1");
  const size_t total = (size_t)a.B * a.T * (a.vdim >> 2);
  const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  const double valid_guess = 0.75;     // bytes read depend on the lengths; reported figure assumes 3/4 valid rows
  HUAL_REQUIRE(a.carry_n == 0 || (a.carry_n > 0 && a.carry_src && a.carry_dst), "assemble: carry needs source, destination and a count");
  HUAL_LAUNCH(0.0, 4.0 * (double)a.B * a.T * a.vdim * (1.0 + valid_guess), assemble_kernel, dim3(grid + a.B + 1), dim3(256), 0, s, a);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace hual

namespace {

// the dataset, the batch and its feeds: what every entry point below hands to the launch
AssembleArgs assemble_args(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video, int32_t* video_seq_len,
                           int32_t* word_ids, int32_t* char_ids, float* y1, float* y2, int32_t* match_labels, float* inner_labels) {
  AssembleArgs a{};
  a.feat_bank = ds->feat_bank; a.feat_off = ds->feat_off; a.vdim = ds->vdim; a.sample_vid = ds->sample_vid;
  a.word_off = ds->word_off; a.word_bank = ds->word_bank; a.char_off = ds->char_off; a.char_bank = ds->char_bank;
  a.s_ind = ds->s_ind; a.e_ind = ds->e_ind;
  a.sel = sel; a.B = B; a.T = T; a.L = L; a.C = C;
  a.video = video; a.lens = video_seq_len; a.word_ids = word_ids; a.char_ids = char_ids;
  a.y1 = y1; a.y2 = y2; a.match = match_labels; a.inner = inner_labels;
  return a;
}

// the banks of a _soft entry point.  A null array must never turn the call into a plain assembly: refused here, before
// launch_assemble chooses by a.soft_w
int soft_args(AssembleArgs& a, const hual_soft_labels* soft, const std::string& who) {
  HUAL_REQUIRE(soft, who + ": null soft labels");
  HUAL_REQUIRE(soft->y1 && soft->y2 && soft->w, who + ": null soft->y1, soft->y2 or soft->w");
  HUAL_REQUIRE(soft->ld >= 1, who + ": soft->ld >= 1");
  HUAL_REQUIRE(a.y1, who + ": soft labels need the label feeds y1, y2, match_labels, inner_labels");
  a.soft_y1 = soft->y1; a.soft_y2 = soft->y2; a.soft_w = soft->w; a.soft_ld = soft->ld;
  return 0;
}

}  // namespace

extern "C" {

int hual_assemble_batch(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                        int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                        int32_t* match_labels, float* inner_labels, void* stream) {
  return hual_assemble_batch_carry(ds, sel, B, T, L, C, video, video_seq_len, word_ids, char_ids, y1, y2, match_labels, inner_labels,
                                   nullptr, nullptr, 0, stream);
}

int hual_assemble_batch_carry(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                              int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                              int32_t* match_labels, float* inner_labels, const int64_t* carry_src, int64_t* carry_dst, int carry_n,
                              void* stream) {
  HUAL_REQUIRE(ds, "hual_assemble_batch: null dataset");
  AssembleArgs a = assemble_args(ds, sel, B, T, L, C, video, video_seq_len, word_ids, char_ids, y1, y2, match_labels, inner_labels);
  a.carry_src = carry_src; a.carry_dst = carry_dst; a.carry_n = carry_n;
  return launch_assemble(a, (hipStream_t)stream);
}

int hual_assemble_batch_cursor(const hual_dataset* ds, const int32_t* ids, const int64_t* cursor, int B, int T, int L, int C, float* video,
                               int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                               int32_t* match_labels, float* inner_labels, void* stream) {
  HUAL_REQUIRE(ds && cursor, "hual_assemble_batch_cursor: null dataset / cursor");
  AssembleArgs a = assemble_args(ds, ids, B, T, L, C, video, video_seq_len, word_ids, char_ids, y1, y2, match_labels, inner_labels);
  a.cursor = cursor;
  return launch_assemble(a, (hipStream_t)stream);
}

int hual_assemble_batch_soft(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                             int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                             int32_t* match_labels, float* inner_labels, const int64_t* carry_src, int64_t* carry_dst, int carry_n,
                             const hual_soft_labels* soft, void* stream) {
  HUAL_REQUIRE(ds, "hual_assemble_batch_soft: null dataset");
  AssembleArgs a = assemble_args(ds, sel, B, T, L, C, video, video_seq_len, word_ids, char_ids, y1, y2, match_labels, inner_labels);
  a.carry_src = carry_src; a.carry_dst = carry_dst; a.carry_n = carry_n;
  if (int rc = soft_args(a, soft, "hual_assemble_batch_soft")) return rc;
  return launch_assemble(a, (hipStream_t)stream);
}

int hual_assemble_batch_cursor_soft(const hual_dataset* ds, const int32_t* ids, const int64_t* cursor, int B, int T, int L, int C,
                                    float* video, int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                                    int32_t* match_labels, float* inner_labels, const hual_soft_labels* soft, void* stream) {
  HUAL_REQUIRE(ds && cursor, "hual_assemble_batch_cursor_soft: null dataset / cursor");
  AssembleArgs a = assemble_args(ds, ids, B, T, L, C, video, video_seq_len, word_ids, char_ids, y1, y2, match_labels, inner_labels);
  a.cursor = cursor;
  if (int rc = soft_args(a, soft, "hual_assemble_batch_cursor_soft")) return rc;
  return launch_assemble(a, (hipStream_t)stream);
}

}  // extern "C"
