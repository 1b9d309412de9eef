// One clip of a [B,T] batch as every per-clip span launch opens it (hual_span_topk in topk.hip, hual_span_expected_iou in spanconf.hip,
// hual_span_hit_prob in spanhit.hip, hual_span_hit_cover in spancover.hip; the contract is in include/hual_seqpan.h): which clips are open, the index of the span triangle,
// the k <= 16 proposal slots and their stable in-place reorder.  One definition, so all launches classify a clip alike
// (tests/test_gpu_span_clips.py); the span-posterior launches have theirs in spanpost.h.
#pragma once
#include "spanprob.h"

constexpr int SPAN_MAXK = 16;               // proposal slots per clip

// one opened clip, (uniform): its clipped length, the offset of its row in the logits; open: v > 0 and no NaN logit below v
struct SpanClip { int v; size_t row; bool open; };

// Clip blockIdx.x, open with ps / pe [256] readable (span_probabilities; smf / smd: its scratch) or not.  before(v) runs in front of the
// poison test, whose barrier is the FIRST of the kernel: it publishes what before() and the kernel wrote to LDS until then
// (load_slots, the tables of spanhit.hip).  Called by the whole workgroup; an open clip ends on a barrier.
template <class Before>
__device__ __forceinline__ SpanClip open_span_clip(const float* __restrict__ zs_, const float* __restrict__ ze_,
                                                   const int32_t* __restrict__ vlen_, int T, float* ps, float* pe, float* smf, double* smd,
                                                   Before before) {
  SpanClip c;
  c.v = span_clip_len(vlen_[blockIdx.x], T);
  c.row = (size_t)blockIdx.x * T;
  before(c.v);
  const int nanlogit = span_row_poisoned(zs_, ze_, c.row, c.v);
  c.open = c.v > 0 && !nanlogit;
  if (c.open) span_probabilities(zs_, ze_, c.row, T, c.v, ps, pe, smf, smd);      // (the numbers of hual_span_argmax)
  return c;
}

// first flat index of row i of the triangle i <= j < v in row-major order (row i holds v - i entries); i == v: the triangle's size
__device__ __forceinline__ int tri_row_off(int i, int v) { return i * v - (i * (i - 1)) / 2; }

// the row holding flat index c: the largest i in [0, v) with off(i) <= c, off ascending - tri_row_off(., v) or topk.hip's banded form
template <class Off>
__device__ __forceinline__ int tri_locate(int c, int v, Off off) {
  int lo = 0, hi = v - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off(mid) <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// (i, j) of flat index c of the full triangle, 0 <= c < v (v + 1) / 2
__device__ __forceinline__ void tri_entry(int c, int v, int& i, int& j) {
  i = tri_locate(c, v, [v](int r) { return tri_row_off(r, v); });
  j = i + (c - tri_row_off(i, v));
}

// the proposal slots of one clip in LDS
struct SpanSlots {
  long long sa[SPAN_MAXK], sb[SPAN_MAXK];   // the incoming slots as given (an invalid one is carried along unchanged)
  float ssc[SPAN_MAXK];
  int ca[SPAN_MAXK], cb[SPAN_MAXK];         // the slot's span, or ca = -1 for an invalid slot
};

// thread t < k: slot t of clip b into s.  Inside open_span_clip's before(): store_slot writes back in place, which is safe only
// because every slot is in LDS before the kernel's first barrier.
__device__ __forceinline__ void load_slots(SpanSlots& s, int b, int k, int v, const int64_t* start_index, const int64_t* end_index,
                                           const float* score) {
  const int t = threadIdx.x;
  if (t >= k) return;
  const size_t slot = (size_t)b * k + t;
  const long long a = start_index[slot], e = end_index[slot];
  const bool ok = a >= 0 && a <= e && e < v;
  s.sa[t] = a; s.sb[t] = e;
  s.ssc[t] = score ? score[slot] : 0.f;
  s.ca[t] = ok ? (int)a : -1; s.cb[t] = ok ? (int)e : -1;
}

// the stable descending rank of slot t < k by value(q): the slots that go before it (invalid slots hold -1, below every value)
template <class Value>
__device__ __forceinline__ int slot_rank(int k, int t, Value value) {
  const float mine = value(t);
  int pos = 0;
  for (int q = 0; q < k; ++q) pos += (value(q) > mine || (value(q) == mine && q < t)) ? 1 : 0;
  return pos;
}

// slot t as it came in goes to position pos of clip b
__device__ __forceinline__ void store_slot(const SpanSlots& s, int t, int b, int k, int pos, int64_t* start_index, int64_t* end_index,
                                           float* score) {
  const size_t o = (size_t)b * k + pos;
  start_index[o] = s.sa[t]; end_index[o] = s.sb[t];
  if (score) score[o] = s.ssc[t];
}
