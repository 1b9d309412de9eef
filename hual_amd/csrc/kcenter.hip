// hual_kcenter_greedy and hual_kcenter_sample (include/hual_seqpan.h): the host side of the core-set selection - argument checks,
// the workspace layout and the launch sequence.  The kernels are kcenter.h's; hual_kcenter_greedy instantiates <false, false>.
#include "kcenter.h"
#include "prof.h"

namespace {

inline uint64_t kc_round16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

struct KcCall {
  const float* x;
  int N, D, ld;
  const float* weight;
  const int32_t* init;
  int n_init, n_select;
  int32_t* picked;
  float* pick_dist;
  float* mind;
  int32_t* assign;
  void* workspace;
  uint64_t workspace_bytes;
  void* stream;
};

// the launch sequence of one selection: opening, init updates, steps, closing update
template <bool SAMPLE, bool ORIGIN>
int kc_enqueue(const KcCall& c, const KcRng& rng) {
  hipStream_t st = (hipStream_t)c.stream;
  const int N = c.N, D = c.D;
  KcArgs a{};
  a.x = c.x; a.weight = c.weight; a.N = N; a.D = D; a.ld = c.ld;
  a.vec = (D % 4 == 0 && c.ld % 4 == 0 && ((uintptr_t)c.x & 15) == 0) ? 1 : 0;
  a.mind = c.mind; a.assign = c.assign; a.picked = c.picked; a.pick_dist = c.pick_dist;
  char* ws = (char*)c.workspace;
  a.counter = (uint32_t*)ws;
  a.taken = (int32_t*)(ws + 16);
  a.partial = (float4*)(ws + 16 + kc_round16(4ull * (uint64_t)N));
  const int grid = hual::cdiv(N, KC_ROWS);
  const double row_bytes = 4.0 * D * N;
  HUAL_LAUNCH(0.0, row_bytes + 12.0 * N, kcenter_open_kernel<ORIGIN>, dim3(grid), dim3(KC_THREADS), 0, st, a);
  for (int j = 0; j < c.n_init; ++j)                         // the init rows, in their order: update only, each marked taken
    HUAL_LAUNCH(3.0 * D * N, row_bytes + 8.0 * N, (kcenter_step_kernel<SAMPLE, ORIGIN>), dim3(grid), dim3(KC_THREADS), 0, st, a, c.init + j, 1, 0,
                0, rng);
  for (int s = 0; s < c.n_select; ++s)
    HUAL_LAUNCH(3.0 * D * N, row_bytes + 16.0 * N, (kcenter_step_kernel<SAMPLE, ORIGIN>), dim3(grid), dim3(KC_THREADS), 0, st, a,
                s ? (const int32_t*)(c.picked + s - 1) : (const int32_t*)nullptr, 0, 1, s, rng);
  // the closing update: mind and assign account for the last pick too
  HUAL_LAUNCH(3.0 * D * N, row_bytes + 8.0 * N, (kcenter_step_kernel<SAMPLE, ORIGIN>), dim3(grid), dim3(KC_THREADS), 0, st, a,
              (const int32_t*)(c.picked + c.n_select - 1), 0, 0, 0, rng);
  HUAL_CHECK_HIP(hipGetLastError());
  return 0;
}

// the argument rules the two entry points share -> 0, 1 (n_select == 0: nothing is owed) or an error
int kc_check(const KcCall& c, const char* who) {      // (HUAL_REQUIRE puts a message together only where its rule fails)
  HUAL_REQUIRE(c.N >= 1, std::string(who) + ": N >= 1");
  HUAL_REQUIRE(c.D >= 1 && c.D <= KC_MAXD, std::string(who) + ": 1 <= D <= 4096");
  HUAL_REQUIRE(c.ld >= c.D, std::string(who) + ": ld >= D");
  HUAL_REQUIRE(c.n_select >= 0 && c.n_select <= c.N, std::string(who) + ": 0 <= n_select <= N");
  HUAL_REQUIRE(c.n_init >= 0 && c.n_init <= c.N, std::string(who) + ": 0 <= n_init <= N");
  HUAL_REQUIRE(c.n_init == 0 || c.init, std::string(who) + ": null pointer (init with n_init >= 1)");
  if (c.n_select == 0) return 1;                             // nothing is owed: nothing is written
  HUAL_REQUIRE(c.x && c.picked && c.pick_dist && c.mind && c.assign && c.workspace,
               std::string(who) + ": null pointer (x, picked, pick_dist, mind, assign, workspace)");
  HUAL_REQUIRE(c.workspace_bytes >= hual_kcenter_workspace_bytes(c.N), std::string(who) + ": workspace smaller than hual_kcenter_workspace_bytes(N)");
  HUAL_REQUIRE(((uintptr_t)c.workspace & 15) == 0, std::string(who) + ": workspace must be 16-byte aligned");
  return 0;
}

}  // namespace

extern "C" uint64_t hual_kcenter_workspace_bytes(int N) {
  if (N < 1) return 0;
  return 16 + kc_round16(4ull * (uint64_t)N) + 16ull * (uint64_t)hual::cdiv(N, KC_ROWS);
}

extern "C" int hual_kcenter_greedy(const float* x, int N, int D, int ld, const float* weight, const int32_t* init, int n_init, int n_select,
                                   int32_t* picked, float* pick_dist, float* mind, int32_t* assign, void* workspace, uint64_t workspace_bytes,
                                   void* stream) {
  const KcCall c{x, N, D, ld, weight, init, n_init, n_select, picked, pick_dist, mind, assign, workspace, workspace_bytes, stream};
  const int rc = kc_check(c, "hual_kcenter_greedy");
  if (rc) return rc < 0 ? rc : 0;
  return kc_enqueue<false, false>(c, KcRng{0u, 0u, 0u});
}

extern "C" int hual_kcenter_sample(const float* x, int N, int D, int ld, const float* weight, const int32_t* init, int n_init, int n_select,
                                   uint64_t seed, uint32_t offset, int sample, int origin, int32_t* picked, float* pick_dist, float* mind,
                                   int32_t* assign, void* workspace, uint64_t workspace_bytes, void* stream) {
  const KcCall c{x, N, D, ld, weight, init, n_init, n_select, picked, pick_dist, mind, assign, workspace, workspace_bytes, stream};
  const int rc = kc_check(c, "hual_kcenter_sample");
  if (rc) return rc < 0 ? rc : 0;
  const KcRng rng{(uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), offset};
  if (sample) return origin ? kc_enqueue<true, true>(c, rng) : kc_enqueue<true, false>(c, rng);
  return origin ? kc_enqueue<false, true>(c, rng) : kc_enqueue<false, false>(c, rng);
}
