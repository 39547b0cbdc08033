// pulsar-tlaplus_amd/csrc/liveness.hip -- PROPERTY Termination on the GPU:
// TLC's liveness check (tlc2.tool.liveness) of <>P, compaction.tla:303-307,
// over the spec's state graph.
//
// P is the guard of Terminating (terminating_enabled, compaction.tla:205-214
// and :304-307 are the same conjunction).  A behavior violates <>P iff it
// never reaches a P state, so every counterexample lives in G', the states
// reachable from Init through not-P states only.  (TLC builds the product of
// the state graph with the tableau of the negated property, []~P; its
// consistent part is exactly G'.)  Fairness decides which infinite paths of
// G' are behaviors:
//   - none (Spec, compaction.tla:233): a behavior may stutter forever, so
//     every state of G' ends a counterexample; the shortest is the first
//     not-P initial state followed by stuttering;
//   - WF_vars(Next) (or SF_vars(Next): <<Next>>_vars is enabled in a state or
//     not, so the two agree here): a fair behavior stutters forever only where
//     <<Next>>_vars is disabled -- a state all of whose successors equal it
//     ("stuck") -- and otherwise takes infinitely many non-stuttering steps.
//     <>P fails iff G' holds a stuck state or a cycle of non-stuttering steps.
//
// The GPU pass:
//   1. BFS over G' (k_lv_init, k_lv_expand per level): successors that
//      satisfy P end the path and are not stored; the others go through an
//      HBM FPSet (kernels.h fpset_put) into a level-ordered store with parent
//      references, exactly like the safety engine's, and every edge into a
//      not-P state adds 1 to that state's in-degree (indexed by FPSet slot, so
//      no index lookup is needed while the level is being built).  A state
//      with no non-stuttering successor is flagged stuck.
//   2. Cycle test by Kahn peeling (k_lv_zero, k_lv_peel): repeatedly remove
//      the states of in-degree 0 and decrement their successors; G' is
//      acyclic iff every state is removed.
//   3. Counterexample: the shallowest stuck state (least packed word among
//      the stuck states of the shallowest level) and its BFS path from Init;
//      or, for a cycle, the states left after peeling (k_lv_zero with left =
//      1, gathered by k_lv_gather) are copied to the host, peeled again from
//      the other side (states with no successor left), and walked from the
//      shallowest one until a state repeats: the lasso is the BFS path to the
//      repeated state plus the cycle back to it.
// Counterexample choice and the output text are [TLC-ext] (TLC picks its
// own); holds / fails, |G'|, its edge count and the shallowest stuck depth are
// cross-checked with the oracle's Tarjan SCC restatement (oracle/tlc_oracle.c
// -liveness).
//
// The file also checks the properties a user defines: <>Q, []<>Q, P ~> Q over
// compiled state predicates (tlcg_check_property: the reachable graph, then a
// seeded pass in index space) and [][A]_v over a compiled two-state program
// (tlcg_check_action_property: the reachable graph, then every step once).
// The three passes share two host drivers: Reach, the BFS of phase 1 with its
// grow-and-redo loop, which all three run; and peel_verdict, phases 2 and 3,
// which Termination and the property pass run through a view each (TermView,
// PropView) that says how their G' is indexed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_model.h"
#include "kernels.h"
#include "liveness_graph.h"
#include "tlcgpu.h"

using namespace tlcg;

namespace {

using u32 = uint32_t;
constexpr int LV_BLOCK = 256;

enum LvFlag { LV_FPSET = 1, LV_STORE = 2, LV_EVAL = 4, LV_LOOKUP = 8 };

// the counters of a G' (the reach BFS's, and the property pass's sub-BFS's)
struct LvCtrHead {
  unsigned long long n;      // states of G' stored (the sub-BFS: entries of `order`)
  unsigned long long edges;  // non-stuttering edges into states of G'
  unsigned long long stuck;  // stuck states, summed over the levels (the host takes the difference per level)
  unsigned long long next;   // entries appended to the next peel list
  unsigned long long key_hi, key_lo, pick;  // least flagged state of a level, then its stored index
};
struct LvCtr : LvCtrHead {
  unsigned long long first_init;  // Init index of the first not-P initial state
  unsigned int flags;
  unsigned int pad;
};
static_assert(sizeof(LvCtrHead) == 56 && sizeof(LvCtr) == 72, "the kernels' counter layout");

// G: the graph policy (liveness_graph.h)
template <typename G>
struct LvBufs {
  using W = typename G::word;
  G g;
  u64* slots;     // FPSet, 2^log2 slots (8 B, or 16 B wide)
  int log2;
  W* store;       // states of G' in BFS order
  u64* parent;    // parent_gidx << ord_bits | ordinal, NO_PARENT for initial states
  u32* slot_of;   // FPSet slot of each stored state
  u32* gidx_of;   // stored index of the state in each FPSet slot
  u32* indeg;     // per FPSet slot: edges from states of G'
  unsigned char* stuck;  // per state: fairness lets a behavior stutter here forever
  u64 cap;        // store capacity
  LvCtr* ctr;
};

// Block-aggregated claim of indices in a global counter: one atomic per
// block per call instead of one per wave (a single counter serializes its
// atomics).  Every thread of the block calls it (uniform control flow) with
// NP predicates; at[j] gets the index of each true one, in (wave, j, lane)
// order.
template <int NP>
__device__ __forceinline__ void block_claim(const bool* pred, u64* at, unsigned long long* ctr) {
  __shared__ unsigned s_wcnt[LV_BLOCK / 64];
  __shared__ unsigned long long s_base;
  const int w = (int)(threadIdx.x >> 6);
  u64 m[NP];
  unsigned tot = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    m[j] = __ballot(pred[j]);
    tot += (unsigned)__popcll(m[j]);
  }
  if (__lane_id() == 0) s_wcnt[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0;
    for (int i = 0; i < LV_BLOCK / 64; ++i) sum += s_wcnt[i];
    s_base = sum ? atomicAdd(ctr, (unsigned long long)sum) : 0ull;
  }
  __syncthreads();
  u64 base = s_base;
  for (int i = 0; i < w; ++i) base += s_wcnt[i];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    at[j] = base + (u64)__popcll(m[j] & lanemask_lt());
    base += (u64)__popcll(m[j]);
  }
  __syncthreads();  // (s_wcnt / s_base are reused by the next call)
}

// FPSet lookup of a state known to be present (all inserts finished in an
// earlier launch, so plain loads see every slot).
template <typename W>
__device__ __forceinline__ u64 lv_lookup(const u64* slots, int log2, W t) {
  const u64 mask = (1ull << log2) - 1;
  u64 i = mixw<W>(t) >> (64 - log2);
  for (int p = 0; p < MAX_PROBE; ++p) {
    if constexpr (sizeof(W) == 8) {
      const u64 v = slots[i];
      if (v == ((u64)t | SLOT_TAG)) return i;
      if (v == 0) return ~0ull;
    } else {
      const u64 hi = slots[2 * i];
      if (hi == 0) return ~0ull;
      if ((hi & ~WIDE_READY) == ((u64)(t >> 64) | SLOT_TAG) && slots[2 * i + 1] == (u64)t) return i;
    }
    i = (i + 1) & mask;
  }
  return ~0ull;
}

// insert t (a not-P state) with parent reference pref; every thread of the
// block calls it (want = this lane has a state to insert)
template <typename G>
__device__ __forceinline__ void lv_insert(const LvBufs<G>& B, bool want, typename G::word t, u64 pref, bool edge) {
  using W = typename G::word;
  u64 slot = 0;
  int r = 0;
  if (want) {
    r = fpset_put<W>(B.slots, B.log2, t, mixw<W>(t), &slot);
    if (r < 0) atomicOr(&B.ctr->flags, (unsigned)LV_FPSET);
    else if (edge) atomicAdd(&B.indeg[slot], 1u);
  }
  const bool fresh = want && r == 1;
  u64 g = 0;
  block_claim<1>(&fresh, &g, &B.ctr->n);
  if (fresh) {
    if (g >= B.cap) {
      atomicOr(&B.ctr->flags, (unsigned)LV_STORE);
    } else {
      B.store[g] = t;
      B.parent[g] = pref;
      B.slot_of[g] = (u32)slot;
      B.gidx_of[slot] = (u32)g;
    }
  }
}

// A batch of up to LV_BATCH candidates of one lane: their first FPSet slots
// are loaded together (and CASed together where empty), so a lane waits on
// one scattered round trip per batch instead of one per candidate; collisions
// go on probing (fpset_put_from).  Wide states take the wave-uniform
// two-word insert one by one.  slot[j] gets the candidate's slot, fresh[j]
// whether this lane inserted it.
constexpr int LV_BATCH = 4;
template <typename G>
__device__ __forceinline__ void lv_put_batch(const LvBufs<G>& B, const bool* want, const typename G::word* t,
                                             u64* slot, bool* fresh) {
  using W = typename G::word;
  if constexpr (sizeof(W) == 8) {
    const int sh = 64 - B.log2;
    const u64 mask = (1ull << B.log2) - 1;
    u64 v[LV_BATCH];
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) {
      slot[j] = mix64((u64)t[j]) >> sh;
      v[j] = want[j] ? __builtin_nontemporal_load(&B.slots[slot[j]]) : 1;
    }
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j)
      if (want[j] && v[j] == 0)
        v[j] = atomicCAS((unsigned long long*)&B.slots[slot[j]], 0ull, (unsigned long long)((u64)t[j] | SLOT_TAG));
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) {
      fresh[j] = false;
      if (!want[j]) continue;
      const u64 key = (u64)t[j] | SLOT_TAG;
      if (v[j] == 0) {
        fresh[j] = true;
      } else if (v[j] != key) {
        const int r = fpset_put_from(B.slots, mask, key, (slot[j] + 1) & mask, &slot[j]);
        if (r < 0) {
          atomicOr(&B.ctr->flags, (unsigned)LV_FPSET);
          slot[j] = ~0ull;
        }
        fresh[j] = r == 1;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) {
      fresh[j] = false;
      if (!want[j]) continue;
      const int r = fpset_put<W>(B.slots, B.log2, t[j], mixw<W>(t[j]), &slot[j]);
      if (r < 0) {
        atomicOr(&B.ctr->flags, (unsigned)LV_FPSET);
        slot[j] = ~0ull;
      }
      fresh[j] = r == 1;
    }
  }
}

// the same for lookups of states known to be present: first slots together
template <typename G>
__device__ __forceinline__ void lv_lookup_batch(const LvBufs<G>& B, const bool* want, const typename G::word* t,
                                                u64* slot) {
  using W = typename G::word;
  if constexpr (sizeof(W) == 8) {
    const int sh = 64 - B.log2;
    const u64 mask = (1ull << B.log2) - 1;
    u64 v[LV_BATCH];
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) {
      slot[j] = mix64((u64)t[j]) >> sh;
      v[j] = want[j] ? B.slots[slot[j]] : 0;
    }
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) {
      if (!want[j]) continue;
      const u64 key = (u64)t[j] | SLOT_TAG;
      if (v[j] == key) continue;
      u64 i = slot[j];
      slot[j] = ~0ull;
      for (int p = 1; p < MAX_PROBE && v[j] != 0; ++p) {
        i = (i + 1) & mask;
        v[j] = B.slots[i];
        if (v[j] == key) {
          slot[j] = i;
          break;
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < LV_BATCH; ++j) slot[j] = want[j] ? lv_lookup<W>(B.slots, B.log2, t[j]) : ~0ull;
  }
}

template <typename G>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_init(LvBufs<G> B) {
  using W = typename G::word;
  const u64 n_init = B.g.n_init();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n_init; base += stride) {
    const u64 i = base + threadIdx.x;
    bool want = false;
    W s = 0;
    if (i < n_init) {
      s = B.g.init(i);
      want = !B.g.is_p(s);
    }
    // the first not-P initial state: the wave's lowest such index, one atomic per wave
    const u64 wm = __ballot(want);
    if (wm && __lane_id() == __ffsll((long long)wm) - 1) atomicMin(&B.ctr->first_init, (unsigned long long)i);
    lv_insert(B, want, s, NO_PARENT, false);
  }
}

// one BFS level of G': states [a, b)
template <typename G>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_expand(LvBufs<G> B, u64 a, u64 b, int fair) {
  using W = typename G::word;
  const G& gr = B.g;
  const int kmax = gr.moves_bound(), ord_bits = gr.ord_bits();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  // edges and stuck states are summed in registers over the whole loop and
  // added once per wave at the end (atomics on one counter serialize)
  u64 edges = 0, nstuck = 0;
  bool err = false;
  for (u64 base = a + (u64)blockIdx.x * LV_BLOCK; base < b; base += stride) {
    const u64 g = base + threadIdx.x;
    const bool live = g < b;
    const W s = live ? B.store[g] : (W)0;
    int moves = 0;
    bool serr = false;
    for (int k0 = 0; k0 < kmax; k0 += LV_BATCH) {
      W t[LV_BATCH];
      int ord[LV_BATCH];
      bool want[LV_BATCH], fresh[LV_BATCH];
      u64 slot[LV_BATCH];
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        t[j] = 0;
        ord[j] = 0;
        const int r = live && k0 + j < kmax ? gr.move(s, k0 + j, &t[j], &ord[j]) : 0;
        serr |= r == 2;
        moves += r == 1;
        want[j] = r == 1 && !gr.is_p(t[j]);
        edges += want[j];
      }
      lv_put_batch(B, want, t, slot, fresh);
      u64 ats[LV_BATCH];
      block_claim<LV_BATCH>(fresh, ats, &B.ctr->n);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        if (want[j] && slot[j] != ~0ull) atomicAdd(&B.indeg[slot[j]], 1u);
        const u64 at = ats[j];
        if (fresh[j]) {
          if (at >= B.cap) {
            atomicOr(&B.ctr->flags, (unsigned)LV_STORE);
          } else {
            B.store[at] = t[j];
            B.parent[at] = (g << ord_bits) | (u64)ord[j];
            B.slot_of[at] = (u32)slot[j];
            B.gidx_of[slot[j]] = (u32)at;
          }
        }
      }
    }
    err |= serr;
    const bool stuck = live && !serr && (fair == TLCG_FAIR_NONE || moves == 0);
    if (live) B.stuck[g] = stuck;
    nstuck += stuck;
  }
  if (err) atomicOr(&B.ctr->flags, (unsigned)LV_EVAL);
  const u64 e = wave_sum_u64(edges), sk = wave_sum_u64(nstuck);
  if (__lane_id() == 0) {
    if (e) atomicAdd(&B.ctr->edges, (unsigned long long)e);
    if (sk) atomicAdd(&B.ctr->stuck, (unsigned long long)sk);
  }
}

// The least flagged state (flag: a byte per stored state) of level [a, b) --
// stored indices, or positions in `order` where there is one: its high word,
// then its low word, then its stored index.  All three passes pick with it.
template <typename W>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_pick(const W* store, const u32* order, const unsigned char* flag,
                                                      LvCtrHead* ctr, u64 a, u64 b, int phase) {
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 i = a + (u64)blockIdx.x * LV_BLOCK + threadIdx.x; i < b; i += stride) {
    const u64 g = order ? order[i] : i;
    if (!flag[g]) continue;
    const W s = store[g];
    const u64 hi = sizeof(W) == 8 ? 0 : (u64)((unsigned __int128)s >> 64), lo = (u64)s;
    if (phase == 0) atomicMin(&ctr->key_hi, (unsigned long long)hi);
    else if (phase == 1) { if (hi == ctr->key_hi) atomicMin(&ctr->key_lo, (unsigned long long)lo); }
    else if (hi == ctr->key_hi && lo == ctr->key_lo) ctr->pick = g;
  }
}

// the states at stored indices pos[0 .. n), or at those positions of `order`
// (the host has checked that they lie inside the store)
template <typename W>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_gather(const W* store, const u32* order, const u32* pos, u64 n,
                                                        W* out) {
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 i = (u64)blockIdx.x * LV_BLOCK + threadIdx.x; i < n; i += stride)
    out[i] = store[order ? order[pos[i]] : pos[i]];
}

// Kahn peeling: the states of in-degree 0 (after the rounds, with left = 1:
// the ones that kept an in-edge, which lie on or after a cycle) ...
template <typename G>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_zero(LvBufs<G> B, u64 n, u32* list, int left) {
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 g = base + threadIdx.x;
    const bool z = g < n && (B.indeg[B.slot_of[g]] == 0) != (left != 0);
    u64 at = 0;
    block_claim<1>(&z, &at, &B.ctr->next);
    if (z) list[at] = (u32)g;
  }
}

// ... then, per round, remove them: each successor in G' loses one in-edge,
// and the ones that reach 0 form the next round
template <typename G>
__global__ __launch_bounds__(LV_BLOCK) void k_lv_peel(LvBufs<G> B, const u32* list, u64 n, u32* next) {
  using W = typename G::word;
  const G& gr = B.g;
  const int kmax = gr.moves_bound();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 i = base + threadIdx.x;
    const bool live = i < n;
    const W s = live ? B.store[list[i]] : (W)0;
    for (int k0 = 0; k0 < kmax; k0 += LV_BATCH) {
      W t[LV_BATCH];
      bool want[LV_BATCH];
      u64 slot[LV_BATCH];
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        t[j] = 0;
        int ord = 0;
        want[j] = live && k0 + j < kmax && gr.move(s, k0 + j, &t[j], &ord) == 1 && !gr.is_p(t[j]);
      }
      lv_lookup_batch(B, want, t, slot);
      bool freed[LV_BATCH];
      u32 tg[LV_BATCH];
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        freed[j] = false;
        tg[j] = 0;
        if (want[j]) {
          if (slot[j] == ~0ull) {
            atomicOr(&B.ctr->flags, (unsigned)LV_LOOKUP);
          } else if (atomicSub(&B.indeg[slot[j]], 1u) == 1u) {
            freed[j] = true;
            tg[j] = B.gidx_of[slot[j]];
          }
        }
      }
      u64 ats[LV_BATCH];
      block_claim<LV_BATCH>(freed, ats, &B.ctr->next);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j)
        if (freed[j]) next[ats[j]] = tg[j];
    }
  }
}

// TLCG_LV_GRID=n caps the grid of every kernel of the pass (a test hook: one
// block then takes every grid-stride chunk); 0 or unset: no cap
unsigned lv_grid_cap() {
  const char* v = std::getenv("TLCG_LV_GRID");
  const long c = v ? std::atol(v) : 0;
  return c > 0 ? (unsigned)std::min<long>(c, 256 * 32) : 256 * 32;
}
unsigned lv_grid(u64 n, unsigned cap) {
  const u64 blocks = (n + LV_BLOCK - 1) / LV_BLOCK;
  return (unsigned)std::max<u64>(1, std::min<u64>(blocks, cap));
}

struct DevMem {
  std::vector<void*> ptrs;
  ~DevMem() { clear(); }
  void clear() {
    for (void* p : ptrs) hipFree(p);
    ptrs.clear();
  }
  template <typename T>
  bool alloc(T** p, u64 count) {
    *p = nullptr;
    if (hipMalloc((void**)p, std::max<u64>(count, 1) * sizeof(T)) != hipSuccess) return false;
    ptrs.push_back(*p);
    return true;
  }
};

#define LV_CHECK(x)                                                              \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      *err = std::string(#x ": ") + hipGetErrorString(e_);                       \
      return -4;                                                                 \
    }                                                                            \
  } while (0)

// device time of a stretch of launches on the null stream
struct LvTimer {
  hipEvent_t a = nullptr, b = nullptr;
  ~LvTimer() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
  hipError_t start() {
    hipError_t e = hipSuccess;
    if (!a && (e = hipEventCreate(&a)) != hipSuccess) return e;
    if (!b && (e = hipEventCreate(&b)) != hipSuccess) return e;
    return hipEventRecord(a, 0);
  }
  hipError_t stop(float* ms) {
    hipError_t e = hipEventRecord(b, 0);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    return e == hipSuccess ? hipEventElapsedTime(ms, a, b) : e;
  }
};

struct LvTrace {
  std::vector<u128> states;
  std::vector<int> actions;
  int loop_to = -1, back_action = -1;
};

// BFS path from Init to stored state g (states and the actions into them)
template <typename G>
int path_to(const LvBufs<G>& B, const G& hg, u64 g, LvTrace* tr, std::string* err) {
  using W = typename G::word;
  const int ord_bits = hg.ord_bits();
  std::vector<std::pair<W, u64>> rev;
  for (;;) {
    W s;
    u64 p;
    LV_CHECK(hipMemcpy(&s, B.store + g, sizeof(W), hipMemcpyDeviceToHost));
    LV_CHECK(hipMemcpy(&p, B.parent + g, sizeof(u64), hipMemcpyDeviceToHost));
    rev.push_back({s, p});
    if (p == NO_PARENT || rev.size() > 1u << 20) break;
    g = p >> ord_bits;
  }
  for (size_t i = rev.size(); i-- > 0;) {
    tr->states.push_back((u128)rev[i].first);
    const u64 p = rev[i].second;
    tr->actions.push_back(p == NO_PARENT ? TLCG_ACT_INIT
                                         : hg.action_of((int)(p & ((1ull << ord_bits) - 1))));
  }
  return 0;
}

// a pass's counters as the device has them now
template <typename C>
int read_ctr(C* h, const C* d_ctr, std::string* err) {
  LV_CHECK(hipMemcpy(h, d_ctr, sizeof *h, hipMemcpyDeviceToHost));
  return 0;
}

// what a pass calls itself and the states it counts, for its messages
struct LvNames {
  const char *prefix, *check, *counted;
};
constexpr LvNames NM_LIVENESS{"liveness", "the liveness check", "not-P states"};
constexpr LvNames NM_PROPERTY{"property", "the property check", "reachable states"};
constexpr LvNames NM_ACTION{"action property", "the action property check", "reachable states"};

// Phase 1 of every pass: the BFS over G' (for ReachAll: over the whole graph)
// into buffers sized by opts, redone with a store and FPSet four times as
// large when either fills up, and with half the capacity when the device
// cannot hold them.  After run() returns 0: B, h (the counters as last read),
// the levels and ms (the kernel time of the attempt that fit) stand; mem owns
// every buffer and tm is free for the caller's own stretches.
template <typename G>
struct Reach {
  using W = typename G::word;
  DevMem mem;
  LvBufs<G> B;
  LvCtr h;
  std::vector<u64> level_base;   // level l is store[level_base[l], level_base[l + 1]); the last entry repeats
  std::vector<u64> level_stuck;  // stuck states per level
  float ms = 0.f;
  LvTimer tm;
  const unsigned grid_cap = lv_grid_cap();
  unsigned grid(u64 n) const { return lv_grid(n, grid_cap); }

  // dg: the graph as the kernels read it; fair: what makes a state stuck;
  // extra(mem, cap): allocates the pass's own buffers that are sized by the
  // capacity (false: they do not fit, which halves the capacity as well)
  template <typename Extra>
  int run(const G& dg, const tlcg_opts* o, int fair, const LvNames& nm, Extra extra, std::string* err) {
    const std::string pre = std::string(nm.prefix) + ": ";
    u64 cap = o && o->state_capacity ? o->state_capacity : (u64)1 << 22;
    int log2 = o && o->log2_fpset_slots > 0 ? o->log2_fpset_slots : 0;
    for (int attempt = 0;; ++attempt) {
      if (cap >= (1ull << 32) - 1) {
        *err = std::string(nm.check) + " indexes states with 32 bits: more than 2^32 - 1 " + nm.counted;
        return -5;
      }
      int lg = log2;
      if (lg <= 0 || attempt > 0) {
        lg = 10;
        while ((1ull << lg) < 2 * cap) ++lg;
      }
      if (lg > 32) lg = 32;
      mem.clear();  // (the last attempt's buffers go before this one's come)
      B.g = dg;
      B.log2 = lg;
      B.cap = cap;
      const u64 nslots = 1ull << lg;
      if (!mem.alloc(&B.slots, nslots * (sizeof(W) / 8)) || !mem.alloc(&B.store, cap) || !mem.alloc(&B.parent, cap) ||
          !mem.alloc(&B.slot_of, cap) || !mem.alloc(&B.gidx_of, nslots) || !mem.alloc(&B.indeg, nslots) ||
          !mem.alloc(&B.stuck, cap) || !mem.alloc(&B.ctr, 1) || !extra(mem, cap)) {
        if (cap > (1ull << 20) && attempt < 8) {
          // what HBM holds beside the caller's other buffers: a smaller start,
          // grown x4 below only if G' needs it
          cap /= 2;
          log2 = 0;
          continue;
        }
        *err = pre + "device allocation failed (" + std::to_string(cap) + " states, 2^" + std::to_string(lg) +
               " FPSet slots)";
        return -5;
      }
      LV_CHECK(hipMemset(B.slots, 0, nslots * sizeof(W)));
      LV_CHECK(hipMemset(B.indeg, 0, nslots * sizeof(u32)));
      h = LvCtr{};
      h.first_init = ~0ull;
      LV_CHECK(hipMemcpy(B.ctr, &h, sizeof h, hipMemcpyHostToDevice));
      auto grow = [&]() { return (h.flags & (LV_FPSET | LV_STORE)) != 0; };
      LV_CHECK(tm.start());
      k_lv_init<G><<<grid(dg.n_init()), LV_BLOCK>>>(B);
      LV_CHECK(hipGetLastError());
      if (read_ctr(&h, B.ctr, err)) return -4;
      level_base = {0, std::min<u64>(h.n, cap)};
      level_stuck.clear();
      bool again = grow();
      while (!again && level_base.back() > level_base[level_base.size() - 2]) {
        const u64 a = level_base[level_base.size() - 2], b = level_base.back(), stuck_before = h.stuck;
        k_lv_expand<G><<<grid(b - a), LV_BLOCK>>>(B, a, b, fair);
        LV_CHECK(hipGetLastError());
        if (read_ctr(&h, B.ctr, err)) return -4;
        if (h.flags & LV_EVAL) {
          *err = pre + "an evaluation error while computing a successor (run the safety check first)";
          return -6;
        }
        if ((again = grow())) break;
        level_stuck.push_back(h.stuck - stuck_before);  // (the device's count runs on over the levels)
        level_base.push_back(h.n);
      }
      LV_CHECK(tm.stop(&ms));
      if (!again) return 0;
      cap *= 4;  // redo with a larger store and FPSet
    }
  }
};

// the least flagged state of level [a, b) into h->pick (~0: none); d_ctr / h:
// a pass's counters on the device and as last read
template <typename W, typename C>
int pick_least(const W* store, const u32* order, const unsigned char* flag, C* d_ctr, C* h, u64 a, u64 b,
               unsigned grid, std::string* err) {
  h->key_hi = h->key_lo = h->pick = ~0ull;
  LV_CHECK(hipMemcpy(d_ctr, h, sizeof *h, hipMemcpyHostToDevice));
  for (int ph = 0; ph < 3; ++ph) k_lv_pick<W><<<grid, LV_BLOCK>>>(store, order, flag, d_ctr, a, b, ph);
  LV_CHECK(hipGetLastError());
  LV_CHECK(hipMemcpy(h, d_ctr, sizeof *h, hipMemcpyDeviceToHost));
  return 0;
}

// Phases 2 and 3 over a G' that has been built level by level: Kahn peeling,
// the verdict into *lv and the counterexample into *tr.  level / level_stuck:
// G' levels and their stuck states, as Reach keeps them; la, lb: peel lists of
// level.back() entries each; ms_before: kernel time so far, to which the time
// since the caller's r.tm.start() is added.  V, the view of the pass's G':
//   r, d_ctr, h      its Reach; its counters on the device and as last read
//   order, n_all     G' in BFS order as stored indices (null: G' is the store), their bound
//   stuck            the stuck byte per stored state
//   zero(n, list, left), peel(list, n, next)   launch the peel kernels
//   path(g, tr, err), stutter(tr, err)   the trace to stored state g, the no-fairness trace
template <typename G, typename V>
int peel_verdict(V& v, const G& hg, int fair, const std::vector<u64>& level, const std::vector<u64>& level_stuck,
                 u32* la, u32* lb, float ms_before, const LvNames& nm, tlcg_liveness* lv, LvTrace* tr,
                 std::string* err) {
  using W = typename G::word;
  const std::string pre = std::string(nm.prefix) + ": ";
  auto& r = v.r;
  auto& h = v.h;
  const u64 n = level.back();
  LV_CHECK(hipMemset(&v.d_ctr->next, 0, sizeof(unsigned long long)));
  v.zero(n, la, 0);
  LV_CHECK(hipGetLastError());
  if (read_ctr(&h, v.d_ctr, err)) return -4;
  u64 removed = 0, cur = h.next;
  int rounds = 0;
  while (cur) {
    removed += cur;
    ++rounds;
    LV_CHECK(hipMemset(&v.d_ctr->next, 0, sizeof(unsigned long long)));
    v.peel(la, cur, lb);
    LV_CHECK(hipGetLastError());
    if (read_ctr(&h, v.d_ctr, err)) return -4;
    if (h.flags & LV_LOOKUP) {
      *err = pre + "a successor in G' is missing from the FPSet";
      return -6;
    }
    cur = h.next;
    std::swap(la, lb);
  }
  float ms = 0.f;
  LV_CHECK(r.tm.stop(&ms));
  lv->stuck = 0;
  for (u64 x : level_stuck) lv->stuck += x;
  lv->peel_rounds = rounds;
  lv->on_cycles = n - removed;
  lv->kernel_ms = ms_before + ms;
  if (lv->stuck) {
    lv->holds = 0;
    lv->kind = TLCG_LIVE_STUTTERING;
    // without fairness every state of G' may stutter forever; with it, the
    // least stuck state of the shallowest level that has one
    if (fair == TLCG_FAIR_NONE) return v.stutter(tr, err);
    size_t l = 0;
    while (level_stuck[l] == 0) ++l;
    const u64 a = level[l], b = level[l + 1];
    if (const int rc = pick_least(r.B.store, v.order, v.stuck, v.d_ctr, &h, a, b, r.grid(b - a), err)) return rc;
    if (h.pick >= v.n_all) {
      *err = pre + "no stuck state found in its level";
      return -6;
    }
    return v.path(h.pick, tr, err);
  }
  if (removed == n) {
    lv->holds = 1;
    lv->kind = TLCG_LIVE_HOLDS;
    return 0;
  }
  // a cycle: the states left after peeling, by their place in G' BFS order
  lv->holds = 0;
  lv->kind = TLCG_LIVE_CYCLE;
  const u64 left = n - removed;
  if (left > (1ull << 26)) {
    *err = pre + std::to_string(left) + " states lie on or after cycles; the lasso extraction takes at most 2^26";
    return -5;
  }
  LV_CHECK(hipMemset(&v.d_ctr->next, 0, sizeof(unsigned long long)));
  v.zero(n, la, 1);
  LV_CHECK(hipGetLastError());
  std::vector<u32> pos(left), ord_h(v.order ? n : 0);
  std::vector<W> st(left);
  LV_CHECK(hipMemcpy(pos.data(), la, left * sizeof(u32), hipMemcpyDeviceToHost));
  if (v.order) LV_CHECK(hipMemcpy(ord_h.data(), v.order, n * sizeof(u32), hipMemcpyDeviceToHost));
  std::sort(pos.begin(), pos.end());
  auto stored = [&](u64 p) -> u64 { return v.order ? ord_h[p] : p; };
  for (u64 i = 0; i < left; ++i)
    if (pos[i] >= n || stored(pos[i]) >= v.n_all) {
      *err = pre + "a state left after peeling lies outside G'";
      return -6;
    }
  // their states, gathered on the device in that order and copied at once
  W* d_st = nullptr;
  if (!r.mem.alloc(&d_st, left)) {
    *err = pre + "device allocation failed (the states left after peeling)";
    return -5;
  }
  LV_CHECK(hipMemcpy(la, pos.data(), left * sizeof(u32), hipMemcpyHostToDevice));
  k_lv_gather<W><<<r.grid(left), LV_BLOCK>>>(r.B.store, v.order, la, left, d_st);
  LV_CHECK(hipGetLastError());
  LV_CHECK(hipMemcpy(st.data(), d_st, left * sizeof(W), hipMemcpyDeviceToHost));
  // (the walk stays among the states left, so a ReachAll host graph, which
  // has no P or Q of its own, serves it)
  u64 entry = 0;
  std::vector<u128> cyc;
  std::vector<int> cyc_act;
  int back = -1;
  if (lasso_walk(hg, st, pos, &entry, &cyc, &cyc_act, &back, err) != 0) return -6;
  // the path to the cycle's entry, then around the cycle back to it
  if (const int rc = v.path(stored(entry), tr, err)) return rc;
  tr->loop_to = (int)tr->states.size() - 1;
  tr->states.insert(tr->states.end(), cyc.begin(), cyc.end());
  tr->actions.insert(tr->actions.end(), cyc_act.begin(), cyc_act.end());
  tr->back_action = back;
  return 0;
}

// Termination's G' is the store itself: stored indices, in-degree by FPSet slot
template <typename G>
struct TermView {
  Reach<G>& r;
  const G& hg;
  LvCtr* d_ctr;
  LvCtr& h;
  const u32* order;
  u64 n_all;
  const unsigned char* stuck;
  void zero(u64 n, u32* list, int left) { k_lv_zero<G><<<r.grid(n), LV_BLOCK>>>(r.B, n, list, left); }
  void peel(const u32* list, u64 n, u32* next) { k_lv_peel<G><<<r.grid(n), LV_BLOCK>>>(r.B, list, n, next); }
  int path(u64 g, LvTrace* tr, std::string* err) { return path_to(r.B, hg, g, tr, err); }
  // the first not-P initial state in Init order, then stuttering
  int stutter(LvTrace* tr, std::string*) {
    tr->states.push_back((u128)hg.init(h.first_init));
    tr->actions.push_back(TLCG_ACT_INIT);
    return 0;
  }
};

// dg: the graph as the kernels read it, hg: as the host reads it (the same
// object for ModelGraph; device and host copies of the arrays for ExplicitGraph)
template <typename G>
int run_liveness(const G& dg, const G& hg, const tlcg_opts* o, int fair, tlcg_liveness* out, LvTrace* tr,
                 std::string* err) {
  Reach<G> r;
  if (const int rc = r.run(dg, o, fair, NM_LIVENESS, [](DevMem&, u64) { return true; }, err)) return rc;
  const u64 n = r.h.n;
  out->states_notp = n;
  out->init_notp = r.level_base[1];
  out->edges_notp = r.h.edges;
  out->depth = (int32_t)(r.level_base.size() - 2);  // (the last entry repeats: the empty level that ended the BFS)
  u32 *la = nullptr, *lb = nullptr;
  if (!r.mem.alloc(&la, n) || !r.mem.alloc(&lb, n)) {
    *err = "liveness: device allocation failed (peel lists)";
    return -5;
  }
  LV_CHECK(r.tm.start());
  TermView<G> v{r, hg, r.B.ctr, r.h, nullptr, n, r.B.stuck};
  return peel_verdict(v, hg, fair, r.level_base, r.level_stuck, la, lb, r.ms, NM_LIVENESS, out, tr, err);
}

// the counterexample into the caller's arrays; returns its whole length
int32_t trace_copy_out(const LvTrace& tr, int words, uint64_t* states, int32_t* actions, int32_t cap, int32_t* len) {
  const int32_t all = (int32_t)tr.states.size();
  if (states && actions && len) {
    const int32_t n = std::min<int32_t>(cap, all);
    for (int32_t i = 0; i < n; ++i) {
      split_words(tr.states[i], states + (size_t)i * words, words);
      actions[i] = tr.actions[i];
    }
    *len = n;
  }
  return all;
}
void lv_copy_out(const LvTrace& tr, int words, tlcg_liveness* out, uint64_t* states, int32_t* actions, int32_t cap,
                 int32_t* len) {
  out->trace_len = trace_copy_out(tr, words, states, actions, cap, len);
  out->loop_to = tr.loop_to;
  out->back_action = tr.back_action;
}

// what an extern "C" entry returns when it fails: the message into the caller's buffer
struct Fail {
  char* err;
  int32_t cap;
  int operator()(int rc, const std::string& e) const {
    if (err && cap > 0) std::snprintf(err, (size_t)cap, "%s", e.c_str());
    return rc;
  }
};

// the selftest entries refuse a malformed graph before the device is touched
bool graph_ok(const uint32_t* row, const uint32_t* col, uint32_t n, uint32_t n_init, std::string* err) {
  ExplicitGraph<u64> shape{};
  return explicit_graph_shape(row, col, n, n_init, &shape, err);
}

template <typename W>
int run_model(const HostModel& hm, const tlcg_opts* o, int fair, tlcg_liveness* out, LvTrace* tr, std::string* err) {
  const ModelGraph<W> g{hm.L, hm.n_init};
  return run_liveness(g, g, o, fair, out, tr, err);
}

// n values of the caller's (src null: room for them only) into device memory that mem owns
template <typename T>
int upload(DevMem& mem, const T* src, u64 n, const T** dst, std::string* err) {
  T* d = nullptr;
  if (!mem.alloc(&d, n)) {
    *err = "graph: device allocation failed";
    return -5;
  }
  if (n && src) LV_CHECK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
  *dst = d;
  return 0;
}

// the caller's CSR graph, checked: *hg over the caller's arrays, *dg over
// copies of them in device memory; both without a P
template <typename W>
int upload_graph(const uint32_t* row, const uint32_t* col, uint32_t n, uint32_t n_init, DevMem& mem,
                 ExplicitGraph<W>* hg, ExplicitGraph<W>* dg, std::string* err) {
  *hg = ExplicitGraph<W>{};
  if (!explicit_graph_shape(row, col, n, n_init, hg, err)) return -1;
  hg->row = row;
  hg->col = col;
  *dg = *hg;
  if (const int rc = upload(mem, row, (u64)n + 1, &dg->row, err)) return rc;
  return upload(mem, col, row[n], &dg->col, err);
}

template <typename W>
int run_explicit(const uint32_t* row, const uint32_t* col, const uint8_t* is_p, uint32_t n, uint32_t n_init,
                 const tlcg_opts* o, int fair, tlcg_liveness* out, LvTrace* tr, std::string* err) {
  DevMem mem;
  ExplicitGraph<W> hg, dg;
  if (const int rc = upload_graph(row, col, n, n_init, mem, &hg, &dg, err)) return rc;
  hg.p = is_p;
  if (const int rc = upload(mem, is_p, n, &dg.p, err)) return rc;
  return run_liveness(dg, hg, o, fair, out, tr, err);
}

// ---------------------------------------------------------------- user-defined properties
// <>Q, []<>Q and P ~> Q over predicates the user defines (tlcgpu.h
// tlcg_check_property).  A behavior violates such a property iff from a seed
// state on it stays in ~Q states; S, the seeds, are the initial ~Q states, the
// reachable ~Q states, or the reachable P /\ ~Q states, and G' is what S
// reaches through ~Q states.  The verdicts are the ones above with S in
// Init's place.  S is not known before the reachable states are, so the pass
// is
//   1. reach: the BFS above over the whole graph (ReachAll: no P), which
//      leaves the FPSet, the store with parents, slot_of / gidx_of;
//   2. classify (k_pp_classify): P and Q of every stored state, once, by the
//      compiled program (user_inv.h) into a class byte; later kernels read
//      the byte only;
//   3. seed (k_pp_seed): the seeds' indices into `order`, their member bits;
//   4. sub-BFS in index space (k_pp_expand per level of G'): a successor's
//      index is gidx_of of its FPSet slot; a Q successor ends the path; every
//      other one gets an in-edge and is claimed by an atomicOr on its member
//      bit -- the lane that sets it appends the index to `order` and writes
//      the G' parent.  No second FPSet, no second store;
//   5. Kahn peeling over `order` with the per-index in-degree (k_pp_zero,
//      k_pp_peel);
//   6. counterexample: the G' path (or the lasso) back to its root seed,
//      behind the reach BFS path from Init to that seed.
// 1 is Reach, 5 and 6 are peel_verdict through PropView.
// Per reachable state beside the reach pass's buffers: class byte, member
// bit, order entry, G' parent, two peel list entries: 21.1 B.  The in-degree
// and stuck arrays of the reach pass are reused, indexed by stored index (the
// FPSet has at least as many slots as states).

// G without a P: every state is kept
template <typename G>
struct ReachAll {
  using word = typename G::word;
  G g;
  TLCG_HDM u64 n_init() const { return g.n_init(); }
  TLCG_HDM word init(u64 i) const { return g.init(i); }
  TLCG_HDM bool is_p(word) const { return false; }
  TLCG_HDM int moves_bound() const { return g.moves_bound(); }
  TLCG_HDM int move(word s, int k, word* t, int* ord) const { return g.move(s, k, t, ord); }
  TLCG_HDM int ord_bits() const { return g.ord_bits(); }
  TLCG_HDM int action_of(int ord) const { return g.action_of(ord); }
};

enum PpClass { PC_P = 1, PC_Q = 2, PC_ERR = 4 };

// the class of a state: by the compiled P (entry 0) and Q (entry 1) ...
template <typename W>
struct ProgClass {
  Layout L;
  const UserProg* prog;  // device memory
  __device__ unsigned classify(W s) const {
    const int p = eval_user<W>(L, *prog, 0, s), q = eval_user<W>(L, *prog, 1, s);
    return (p == EV_TRUE ? PC_P : 0u) | (q == EV_TRUE ? PC_Q : 0u) | (p == EV_ERROR || q == EV_ERROR ? PC_ERR : 0u);
  }
};
// ... or, for an explicit graph, by the caller's bytes per node (p null: P is TRUE)
template <typename W>
struct ByteClass {
  const unsigned char *p, *q;  // device memory
  __device__ unsigned classify(W s) const {
    const uint32_t v = ExplicitGraph<W>::node_of(s);
    return (!p || p[v] ? PC_P : 0u) | (q[v] ? PC_Q : 0u);
  }
};

struct PpCtr : LvCtrHead {
  unsigned long long first_seed;  // least stored index of a seed
  unsigned long long first_err;   // least stored index of a state where P or Q fails to evaluate
  unsigned int flags;
  unsigned int pad;
};
static_assert(sizeof(PpCtr) == 80, "the kernels' counter layout");

struct PpBufs {
  unsigned char* cls;    // per stored state: PC_*
  u32* member;           // bit per stored state: in G'
  u32* order;            // G' in BFS order from the seeds: stored indices
  u64* gparent;          // per stored state: G' parent index << ord_bits | ordinal, NO_PARENT for a seed
  u32* indeg;            // per stored state: edges from states of G'
  unsigned char* stuck;  // per stored state: fairness lets a behavior stutter here forever
  u64 n_all;             // stored (reachable) states
  PpCtr* ctr;
};

// the wave's least index among its lanes with `hit` (lanes hold ascending indices)
__device__ __forceinline__ void wave_first(bool hit, u64 i, unsigned long long* least) {
  const u64 wm = __ballot(hit);
  if (wm && __lane_id() == __ffsll((long long)wm) - 1) atomicMin(least, (unsigned long long)i);
}

template <typename R, typename C>
__global__ __launch_bounds__(LV_BLOCK) void k_pp_classify(LvBufs<R> B, C cl, PpBufs pp) {
  const u64 n = pp.n_all, stride = (u64)gridDim.x * LV_BLOCK;
  bool seen = false;  // (wave-uniform: later chunks hold larger indices)
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 g = base + threadIdx.x;
    unsigned c = 0;
    if (g < n) {
      c = cl.classify(B.store[g]);
      pp.cls[g] = (unsigned char)c;
    }
    const bool bad = (c & PC_ERR) != 0;
    if (!seen && __ballot(bad)) {
      wave_first(bad, g, &pp.ctr->first_err);
      seen = true;
    }
  }
}

// the seeds among stored states [0, b): ~Q, and P where the form has one
__global__ __launch_bounds__(LV_BLOCK) void k_pp_seed(PpBufs pp, u64 b, int form) {
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  bool seen = false;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < b; base += stride) {
    const u64 g = base + threadIdx.x;
    const unsigned c = g < b ? pp.cls[g] : (unsigned)PC_Q;
    const bool seed = !(c & PC_Q) && (form != TLCG_PROP_LEADS_TO || (c & PC_P));
    if (!seen && __ballot(seed)) {
      wave_first(seed, g, &pp.ctr->first_seed);
      seen = true;
    }
    u64 at = 0;
    block_claim<1>(&seed, &at, &pp.ctr->n);
    if (seed && at < pp.n_all) {  // (always: a stored index is claimed once)
      pp.order[at] = (u32)g;
      pp.gparent[g] = NO_PARENT;
      atomicOr(&pp.member[g >> 5], 1u << (g & 31));
    }
  }
}

// one BFS level of G': order[a, b)
template <typename R>
__global__ __launch_bounds__(LV_BLOCK) void k_pp_expand(LvBufs<R> B, PpBufs pp, u64 a, u64 b, int fair) {
  using W = typename R::word;
  const R& gr = B.g;
  const int kmax = gr.moves_bound(), ord_bits = gr.ord_bits();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  u64 edges = 0, nstuck = 0;
  bool err = false, lost = false;
  for (u64 base = a + (u64)blockIdx.x * LV_BLOCK; base < b; base += stride) {
    const u64 i = base + threadIdx.x;
    const bool live = i < b;
    const u64 g = live ? pp.order[i] : 0;
    const W s = live ? B.store[g] : (W)0;
    int moves = 0;
    for (int k0 = 0; k0 < kmax; k0 += LV_BATCH) {
      W t[LV_BATCH];
      int ord[LV_BATCH];
      bool want[LV_BATCH], fresh[LV_BATCH];
      u64 slot[LV_BATCH];
      u32 tg[LV_BATCH];
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        t[j] = 0;
        ord[j] = 0;
        const int r = live && k0 + j < kmax ? gr.move(s, k0 + j, &t[j], &ord[j]) : 0;
        err |= r == 2;
        moves += r == 1;
        want[j] = r == 1;
      }
      lv_lookup_batch(B, want, t, slot);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        fresh[j] = false;
        tg[j] = 0;
        if (!want[j]) continue;
        const u32 x = slot[j] == ~0ull ? ~0u : B.gidx_of[slot[j]];
        if (x >= pp.n_all) {  // (every successor of a stored state is stored)
          lost = true;
          continue;
        }
        if (pp.cls[x] & PC_Q) continue;  // a Q state ends the path
        ++edges;
        atomicAdd(&pp.indeg[x], 1u);
        const u32 bit = 1u << (x & 31);
        fresh[j] = !(atomicOr(&pp.member[x >> 5], bit) & bit);
        tg[j] = x;
      }
      u64 ats[LV_BATCH];
      block_claim<LV_BATCH>(fresh, ats, &pp.ctr->n);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j)
        if (fresh[j]) {
          if (ats[j] >= pp.n_all) {
            lost = true;
          } else {
            pp.order[ats[j]] = tg[j];
            pp.gparent[tg[j]] = (g << ord_bits) | (u64)ord[j];
          }
        }
    }
    const bool stuck = live && (fair == TLCG_FAIR_NONE || moves == 0);
    if (live) pp.stuck[g] = stuck;
    nstuck += stuck;
  }
  if (err) atomicOr(&pp.ctr->flags, (unsigned)LV_EVAL);
  if (lost) atomicOr(&pp.ctr->flags, (unsigned)LV_LOOKUP);
  const u64 e = wave_sum_u64(edges), sk = wave_sum_u64(nstuck);
  if (__lane_id() == 0) {
    if (e) atomicAdd(&pp.ctr->edges, (unsigned long long)e);
    if (sk) atomicAdd(&pp.ctr->stuck, (unsigned long long)sk);
  }
}

// Kahn peeling over G': the states of in-degree 0 (stored indices), or with
// left = 1 the ones that kept an in-edge (positions in `order`: G' BFS order)
__global__ __launch_bounds__(LV_BLOCK) void k_pp_zero(PpBufs pp, u64 n, u32* list, int left) {
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 i = base + threadIdx.x;
    const u32 g = i < n ? pp.order[i] : 0;
    const bool z = i < n && (pp.indeg[g] == 0) != (left != 0);
    u64 at = 0;
    block_claim<1>(&z, &at, &pp.ctr->next);
    if (z) list[at] = left ? (u32)i : g;
  }
}

template <typename R>
__global__ __launch_bounds__(LV_BLOCK) void k_pp_peel(LvBufs<R> B, PpBufs pp, const u32* list, u64 n, u32* next) {
  using W = typename R::word;
  const R& gr = B.g;
  const int kmax = gr.moves_bound();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  bool lost = false;
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 i = base + threadIdx.x;
    const bool live = i < n;
    const W s = live ? B.store[list[i]] : (W)0;
    for (int k0 = 0; k0 < kmax; k0 += LV_BATCH) {
      W t[LV_BATCH];
      bool want[LV_BATCH], freed[LV_BATCH];
      u64 slot[LV_BATCH];
      u32 tg[LV_BATCH];
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        t[j] = 0;
        int ord = 0;
        want[j] = live && k0 + j < kmax && gr.move(s, k0 + j, &t[j], &ord) == 1;
      }
      lv_lookup_batch(B, want, t, slot);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j) {
        freed[j] = false;
        tg[j] = 0;
        if (!want[j]) continue;
        const u32 x = slot[j] == ~0ull ? ~0u : B.gidx_of[slot[j]];
        if (x >= pp.n_all) {
          lost = true;
          continue;
        }
        if (pp.cls[x] & PC_Q) continue;
        // (a not-Q successor of a state of G' is in G': the sub-BFS counted this edge)
        if (atomicSub(&pp.indeg[x], 1u) == 1u) {
          freed[j] = true;
          tg[j] = x;
        }
      }
      u64 ats[LV_BATCH];
      block_claim<LV_BATCH>(freed, ats, &pp.ctr->next);
#pragma unroll
      for (int j = 0; j < LV_BATCH; ++j)
        if (freed[j]) {
          if (ats[j] >= pp.n_all) lost = true;
          else next[ats[j]] = tg[j];
        }
    }
  }
  if (lost) atomicOr(&pp.ctr->flags, (unsigned)LV_LOOKUP);
}

// The path inside G' from its root seed to stored state g, behind the reach
// BFS path from Init to that seed; *seed_at = the seed's place in the trace
template <typename R>
int pp_path(const LvBufs<R>& B, const PpBufs& pp, const R& hg, u64 g, LvTrace* tr, int* seed_at, std::string* err) {
  using W = typename R::word;
  const int ord_bits = hg.ord_bits();
  std::vector<std::pair<u64, u64>> rev;  // (stored index, G' parent reference)
  for (;;) {
    u64 p;
    LV_CHECK(hipMemcpy(&p, pp.gparent + g, sizeof(u64), hipMemcpyDeviceToHost));
    rev.push_back({g, p});
    if (p == NO_PARENT || rev.size() > 1u << 20) break;
    g = p >> ord_bits;
    if (g >= pp.n_all) {
      *err = "property: a G' parent reference leaves the store";
      return -6;
    }
  }
  if (const int rc = path_to(B, hg, rev.back().first, tr, err)) return rc;
  *seed_at = (int)tr->states.size() - 1;
  for (size_t i = rev.size() - 1; i-- > 0;) {
    W s;
    LV_CHECK(hipMemcpy(&s, B.store + rev[i].first, sizeof(W), hipMemcpyDeviceToHost));
    tr->states.push_back((u128)s);
    tr->actions.push_back(hg.action_of((int)(rev[i].second & ((1ull << ord_bits) - 1))));
  }
  return 0;
}

// the property pass's G' is `order`: positions in it, in-degree by stored index
template <typename R>
struct PropView {
  Reach<R>& r;
  const R& hg;
  const PpBufs& pp;
  tlcg_property* out;
  PpCtr* d_ctr;
  PpCtr& h;
  const u32* order;
  u64 n_all;
  const unsigned char* stuck;
  void zero(u64 n, u32* list, int left) { k_pp_zero<<<r.grid(n), LV_BLOCK>>>(pp, n, list, left); }
  void peel(const u32* list, u64 n, u32* next) { k_pp_peel<R><<<r.grid(n), LV_BLOCK>>>(r.B, pp, list, n, next); }
  int path(u64 g, LvTrace* tr, std::string* err) { return pp_path(r.B, pp, hg, g, tr, &out->seed_at, err); }
  // the first seed in the BFS order of the reachable states, then stuttering
  int stutter(LvTrace* tr, std::string* err) {
    if (const int rc = path_to(r.B, hg, h.first_seed, tr, err)) return rc;
    out->seed_at = (int)tr->states.size() - 1;
    return 0;
  }
};

// dg / hg: the graph as the kernels / the host read it, cl: the classifier
// (device memory behind it).  -7: P or Q failed to evaluate on stored state
// out->error_state, *tr the BFS path to it.
template <typename G, typename C>
int run_property(const G& dg0, const G& hg0, const C& cl, const tlcg_opts* o, int fair, int form, tlcg_property* out,
                 LvTrace* tr, std::string* err) {
  using R = ReachAll<G>;
  const R dg{dg0}, hg{hg0};
  tlcg_liveness* lv = &out->lv;
  // 1. reach (the peel lists and G' arrays are sized by the capacity, so that
  // what does not fit is known before the BFS, not after it)
  Reach<R> r;
  PpBufs pp{};
  u32 *la = nullptr, *lb = nullptr;
  auto extra = [&](DevMem& mem, u64 cap) {
    return mem.alloc(&pp.cls, cap) && mem.alloc(&pp.member, cap / 32 + 1) && mem.alloc(&pp.order, cap) &&
           mem.alloc(&pp.gparent, cap) && mem.alloc(&la, cap) && mem.alloc(&lb, cap) && mem.alloc(&pp.ctr, 1);
  };
  if (const int rc = r.run(dg, o, fair, NM_PROPERTY, extra, err)) return rc;
  const LvBufs<R>& B = r.B;
  const u64 n_all = r.h.n;
  out->reachable = n_all;
  // 2. classify
  pp.indeg = B.indeg;  // (nslots >= n_all entries; by stored index from here on)
  pp.stuck = B.stuck;
  pp.n_all = n_all;
  PpCtr c{};
  c.first_seed = c.first_err = ~0ull;
  LV_CHECK(hipMemcpy(pp.ctr, &c, sizeof c, hipMemcpyHostToDevice));
  LV_CHECK(hipMemset(pp.indeg, 0, n_all * sizeof(u32)));
  LV_CHECK(hipMemset(pp.stuck, 0, n_all));
  LV_CHECK(hipMemset(pp.member, 0, (n_all / 32 + 1) * sizeof(u32)));
  LV_CHECK(r.tm.start());
  k_pp_classify<R, C><<<r.grid(n_all), LV_BLOCK>>>(B, cl, pp);
  LV_CHECK(hipGetLastError());
  float ms = 0.f;
  LV_CHECK(r.tm.stop(&ms));
  out->classify_ms = ms;
  const float ms_before = r.ms + ms;
  if (read_ctr(&c, pp.ctr, err)) return -4;
  if (c.first_err != ~0ull) {
    out->error_state = (int64_t)c.first_err;
    lv->kernel_ms = ms_before;
    if (const int rc = path_to(B, hg, c.first_err, tr, err)) return rc;
    *err = "property: P or Q failed to evaluate on a reachable state";
    return -7;
  }
  // 3. seed, 4. sub-BFS
  LV_CHECK(r.tm.start());
  const u64 seed_range = form == TLCG_PROP_EVENTUALLY ? r.level_base[1] : n_all;
  k_pp_seed<<<r.grid(seed_range), LV_BLOCK>>>(pp, seed_range, form);
  LV_CHECK(hipGetLastError());
  if (read_ctr(&c, pp.ctr, err)) return -4;
  out->seeds = c.n;
  std::vector<u64> glevel{0, c.n}, level_stuck;
  while (glevel.back() > glevel[glevel.size() - 2]) {
    const u64 a = glevel[glevel.size() - 2], b = glevel.back(), stuck_before = c.stuck;
    k_pp_expand<R><<<r.grid(b - a), LV_BLOCK>>>(B, pp, a, b, fair);
    LV_CHECK(hipGetLastError());
    if (read_ctr(&c, pp.ctr, err)) return -4;
    if (c.flags & (LV_EVAL | LV_LOOKUP)) {
      *err = "property: a successor of a reachable state is missing from the FPSet";
      return -6;
    }
    level_stuck.push_back(c.stuck - stuck_before);
    glevel.push_back(c.n);
  }
  lv->states_notp = c.n;
  lv->init_notp = out->seeds;
  lv->edges_notp = c.edges;
  lv->depth = (int32_t)(glevel.size() - 2);
  // 5. Kahn peeling, 6. verdict and counterexample
  PropView<R> v{r, hg, pp, out, pp.ctr, c, pp.order, n_all, pp.stuck};
  return peel_verdict(v, hg, fair, glevel, level_stuck, la, lb, ms_before, NM_PROPERTY, lv, tr, err);
}

}  // namespace

extern "C" int tlcg_check_termination(const tlcg_model* m, const tlcg_opts* o, int32_t fairness, tlcg_liveness* out,
                                      uint64_t* states, int32_t* actions, int32_t cap, int32_t* len, char* err,
                                      int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (!m || !out) return fail(-1, "null argument");
  if (fairness != TLCG_FAIR_NONE && fairness != TLCG_FAIR_WF_NEXT) return fail(-1, "unknown fairness");
  std::memset(out, 0, sizeof *out);
  out->fairness = fairness;
  if (len) *len = 0;
  HostModel hm;
  std::string e;
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  if (!hm.constraints.empty())
    return fail(-2, "the model has a CONSTRAINT: PROPERTY Termination is not checked under a state constraint");
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  LvTrace tr;
  const int words = state_words(hm.L);
  const int rc = words == 1 ? run_model<u64>(hm, o, fairness, out, &tr, &e)
                            : run_model<u128>(hm, o, fairness, out, &tr, &e);
  out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc) return fail(rc, e);
  lv_copy_out(tr, words, out, states, actions, cap, len);
  return 0;
}

extern "C" int tlcg_liveness_graph_selftest(const uint32_t* row, const uint32_t* col, const uint8_t* is_p, uint32_t n,
                                            uint32_t n_init, int32_t words, const tlcg_opts* o, int32_t fairness,
                                            tlcg_liveness* out, uint64_t* states, int32_t* actions, int32_t cap,
                                            int32_t* len, char* err, int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (!row || !out || (n && !is_p)) return fail(-1, "null argument");
  if (fairness != TLCG_FAIR_NONE && fairness != TLCG_FAIR_WF_NEXT) return fail(-1, "unknown fairness");
  if (words != 1 && words != 2) return fail(-1, "words must be 1 or 2");
  if (row[n] && !col) return fail(-1, "null argument");
  std::memset(out, 0, sizeof *out);
  out->fairness = fairness;
  if (len) *len = 0;
  std::string e;
  if (!graph_ok(row, col, n, n_init, &e)) return fail(-1, e);
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  LvTrace tr;
  const int rc = words == 1 ? run_explicit<u64>(row, col, is_p, n, n_init, o, fairness, out, &tr, &e)
                            : run_explicit<u128>(row, col, is_p, n, n_init, o, fairness, out, &tr, &e);
  out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc) return fail(rc, e);
  lv_copy_out(tr, words, out, states, actions, cap, len);
  return 0;
}

namespace {

template <typename W>
int run_model_property(const HostModel& hm, const UserProg* d_prog, const tlcg_opts* o, int fair, int form,
                       tlcg_property* out, LvTrace* tr, std::string* err) {
  const ModelGraph<W> g{hm.L, hm.n_init};
  const ProgClass<W> cl{hm.L, d_prog};
  return run_property(g, g, cl, o, fair, form, out, tr, err);
}

template <typename W>
int run_explicit_property(const uint32_t* row, const uint32_t* col, const uint8_t* is_p, const uint8_t* is_q,
                          uint32_t n, uint32_t n_init, const tlcg_opts* o, int fair, int form, tlcg_property* out,
                          LvTrace* tr, std::string* err) {
  DevMem mem;
  ExplicitGraph<W> hg, dg;  // (without a P: ReachAll asks for none)
  if (const int rc = upload_graph(row, col, n, n_init, mem, &hg, &dg, err)) return rc;
  ByteClass<W> cl{nullptr, nullptr};
  if (form == TLCG_PROP_LEADS_TO)
    if (const int rc = upload(mem, is_p, n, &cl.p, err)) return rc;
  if (const int rc = upload(mem, is_q, n, &cl.q, err)) return rc;
  return run_property(dg, hg, cl, o, fair, form, out, tr, err);
}

void pp_reset(tlcg_property* out, int fairness, int form) {
  std::memset(out, 0, sizeof *out);
  out->lv.fairness = fairness;
  out->lv.loop_to = -1;
  out->form = form;
  out->seed_at = -1;
  out->error_state = -1;
}

}  // namespace

extern "C" int tlcg_check_property(const tlcg_model* m, const tlcg_opts* o, int32_t fairness, const char* name,
                                   tlcg_property* out, uint64_t* states, int32_t* actions, int32_t cap, int32_t* len,
                                   char* err, int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (!m || !out || !name) return fail(-1, "null argument");
  if (fairness != TLCG_FAIR_NONE && fairness != TLCG_FAIR_WF_NEXT) return fail(-1, "unknown fairness");
  pp_reset(out, fairness, 0);
  if (len) *len = 0;
  HostModel hm;
  std::string e;
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  if (!hm.constraints.empty())
    return fail(-2, "the model has a CONSTRAINT: a temporal PROPERTY is not checked under a state constraint");
  const std::unique_ptr<UserProg> prog(new UserProg);
  int form = 0;
  if (compile_property(*m, hm, name, &form, prog.get(), &e) != 0) return fail(-2, e);
  out->form = form;
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  DevMem mem;
  UserProg* d_prog = nullptr;
  if (!mem.alloc(&d_prog, 1) ||
      hipMemcpy(d_prog, prog.get(), sizeof(UserProg), hipMemcpyHostToDevice) != hipSuccess)
    return fail(-5, "property: device allocation failed (the predicates' program)");
  LvTrace tr;
  const int words = state_words(hm.L);
  const int rc = words == 1 ? run_model_property<u64>(hm, d_prog, o, fairness, form, out, &tr, &e)
                            : run_model_property<u128>(hm, d_prog, o, fairness, form, out, &tr, &e);
  out->lv.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc == -7 && !tr.states.empty()) {
    // which predicate: the host interpreter on the same state
    const u128 s = tr.states.back();
    const bool p_err = eval_user<u128>(hm.L, *prog, 0, s) == EV_ERROR;
    e = std::string("evaluating ") + (p_err ? "P (the left operand)" : "Q") + " of property " + name +
        " failed on a reachable state (the last state of the trace)";
    lv_copy_out(tr, words, &out->lv, states, actions, cap, len);
    return fail(rc, e);
  }
  if (rc) return fail(rc, e);
  lv_copy_out(tr, words, &out->lv, states, actions, cap, len);
  return 0;
}

extern "C" int tlcg_property_graph_selftest(const uint32_t* row, const uint32_t* col, const uint8_t* is_p,
                                            const uint8_t* is_q, uint32_t n, uint32_t n_init, int32_t words,
                                            const tlcg_opts* o, int32_t fairness, int32_t form, tlcg_property* out,
                                            uint64_t* states, int32_t* actions, int32_t cap, int32_t* len, char* err,
                                            int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (form != TLCG_PROP_EVENTUALLY && form != TLCG_PROP_INFINITELY_OFTEN && form != TLCG_PROP_LEADS_TO)
    return fail(-1, "unknown form");
  if (!row || !out || (n && (!is_q || (form == TLCG_PROP_LEADS_TO && !is_p)))) return fail(-1, "null argument");
  if (fairness != TLCG_FAIR_NONE && fairness != TLCG_FAIR_WF_NEXT) return fail(-1, "unknown fairness");
  if (words != 1 && words != 2) return fail(-1, "words must be 1 or 2");
  if (row[n] && !col) return fail(-1, "null argument");
  pp_reset(out, fairness, form);
  if (len) *len = 0;
  std::string e;
  if (!graph_ok(row, col, n, n_init, &e)) return fail(-1, e);
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  LvTrace tr;
  const int rc = words == 1
                     ? run_explicit_property<u64>(row, col, is_p, is_q, n, n_init, o, fairness, form, out, &tr, &e)
                     : run_explicit_property<u128>(row, col, is_p, is_q, n, n_init, o, fairness, form, out, &tr, &e);
  out->lv.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc) return fail(rc, e);
  lv_copy_out(tr, words, &out->lv, states, actions, cap, len);
  return 0;
}

// ---------------------------------------------------------------- action properties
// [][A]_v over a compiled two-state program (tlcgpu.h
// tlcg_check_action_property): a safety property over steps, so there is no
// G', no seed and no cycle -- every step of the reachable graph is looked at
// once.
//   1. reach: the BFS above over the whole graph (ReachAll), which leaves the
//      level-contiguous store and the parent log;
//   2. check (k_ap_check): one lane per stored state; every move that changes
//      the state is a step (the graph policy's definition; [TLC-ext] TLC would
//      evaluate A on a stuttering successor as well) and is evaluated on
//      (s, t) -- the successor is recomputed, never looked up.  Steps,
//      violating and erroring steps are counted in registers and added once
//      per wave; a flag byte per state says whether it has a violating (bit
//      0) or an erroring (bit 1) step;
//   3. the reported step, independent of the order the races of phase 1 left
//      in the store: the least flagged stored index names the shallowest level
//      with a flagged state (the store is level-contiguous), k_lv_pick takes
//      the least packed flagged state of that level, and the host takes that
//      state's lowest-numbered flagged move.
// Beside the reach pass's buffers: nothing per state -- the flag byte is the
// reach pass's stuck byte, which this pass has no other use for.
namespace {

enum ApFlag { AP_VIOLATES = 1, AP_ERRS = 2 };

struct ApCtr {
  unsigned long long steps, violating, erroring;
  unsigned long long first;  // least stored index of a flagged state
};

// the verdict of a step (0 holds, 1 violates, 2 errs): by the compiled program ...
template <typename W>
struct ProgStep {
  Layout L;
  const UserProg* prog;  // device memory in the kernels' instance, host memory in the host's
  TLCG_HDM int verdict(W s, int, W t) const { return eval_user2<W>(L, *prog, 0, s, t); }
};
// ... or, for an explicit graph, by the caller's byte per edge
template <typename W>
struct ByteStep {
  const uint32_t* row;
  const unsigned char* v;
  TLCG_HDM int verdict(W s, int k, W) const { return v[row[ExplicitGraph<W>::node_of(s)] + (uint32_t)k]; }
};

template <typename R, typename E>
__global__ __launch_bounds__(LV_BLOCK) void k_ap_check(LvBufs<R> B, E ev, u64 n, ApCtr* ctr) {
  using W = typename R::word;
  const R& gr = B.g;
  const int kmax = gr.moves_bound();
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  u64 steps = 0, viol = 0, errs = 0;
  bool seen = false;  // (wave-uniform: later chunks hold larger indices)
  for (u64 base = (u64)blockIdx.x * LV_BLOCK; base < n; base += stride) {
    const u64 g = base + threadIdx.x;
    unsigned f = 0;
    if (g < n) {
      const W s = B.store[g];
      for (int k = 0; k < kmax; ++k) {
        W t = 0;
        int ord = 0;
        if (gr.move(s, k, &t, &ord) != 1) continue;  // (2: the reach pass has reported it)
        ++steps;
        const int v = ev.verdict(s, k, t);
        if (v == 1) {
          ++viol;
          f |= AP_VIOLATES;
        } else if (v != 0) {
          ++errs;
          f |= AP_ERRS;
        }
      }
      B.stuck[g] = (unsigned char)f;
    }
    if (!seen && __ballot(f != 0)) {
      wave_first(f != 0, g, &ctr->first);
      seen = true;
    }
  }
  const u64 st = wave_sum_u64(steps), vi = wave_sum_u64(viol), er = wave_sum_u64(errs);
  if (__lane_id() == 0) {
    if (st) atomicAdd(&ctr->steps, (unsigned long long)st);
    if (vi) atomicAdd(&ctr->violating, (unsigned long long)vi);
    if (er) atomicAdd(&ctr->erroring, (unsigned long long)er);
  }
}

// dg / hg: the graph as the kernels / the host read it; dev / host: the step
// evaluator likewise.  -7: the reported step errs (out->error_state, *tr filled).
template <typename G, typename E>
int run_action(const G& dg0, const G& hg0, const E& dev, const E& host, const tlcg_opts* o, tlcg_action_property* out,
               LvTrace* tr, std::string* err) {
  using R = ReachAll<G>;
  using W = typename G::word;
  const R dg{dg0}, hg{hg0};
  // 1. reach
  Reach<R> r;
  ApCtr* d_ctr = nullptr;
  if (const int rc = r.run(dg, o, TLCG_FAIR_WF_NEXT, NM_ACTION,
                           [&](DevMem& mem, u64) { return mem.alloc(&d_ctr, 1); }, err))
    return rc;
  const LvBufs<R>& B = r.B;
  const u64 n = r.h.n;
  out->reachable = n;
  out->depth = (int32_t)(r.level_base.size() - 2);
  // 2. check
  ApCtr c{};
  c.first = ~0ull;
  LV_CHECK(hipMemcpy(d_ctr, &c, sizeof c, hipMemcpyHostToDevice));
  LV_CHECK(r.tm.start());
  k_ap_check<R, E><<<r.grid(n), LV_BLOCK>>>(B, dev, n, d_ctr);
  LV_CHECK(hipGetLastError());
  float ms = 0.f;
  LV_CHECK(r.tm.stop(&ms));
  LV_CHECK(hipMemcpy(&c, d_ctr, sizeof c, hipMemcpyDeviceToHost));
  out->check_ms = ms;
  out->kernel_ms = (double)r.ms + ms;
  out->steps = c.steps;
  out->violating = c.violating;
  out->erroring = c.erroring;
  if (c.first == ~0ull) {
    out->holds = 1;
    return 0;
  }
  // 3. the reported step
  out->holds = 0;
  if (c.first >= n) {
    *err = "action property: the first flagged state lies outside the store";
    return -6;
  }
  size_t lv = 0;
  while (r.level_base[lv + 1] <= c.first) ++lv;
  const u64 a = r.level_base[lv], b = r.level_base[lv + 1];
  if (const int rc = pick_least(B.store, (const u32*)nullptr, B.stuck, B.ctr, &r.h, a, b, r.grid(b - a), err))
    return rc;
  const u64 pick = r.h.pick;
  if (pick < a || pick >= b) {
    *err = "action property: no flagged state found in its level";
    return -6;
  }
  W s;
  LV_CHECK(hipMemcpy(&s, B.store + pick, sizeof(W), hipMemcpyDeviceToHost));
  const int kmax = hg.moves_bound();
  for (int k = 0; k < kmax; ++k) {
    W t = 0;
    int ord = 0;
    if (hg.move(s, k, &t, &ord) != 1) continue;
    const int v = host.verdict(s, k, t);
    if (v == 0) continue;
    out->step_depth = (int32_t)lv + 1;  // (levels count from 1, as depth does: Init is level 1)
    out->step_action = hg.action_of(ord);
    if (const int rc = path_to(B, hg, pick, tr, err)) return rc;
    tr->states.push_back((u128)t);
    tr->actions.push_back(out->step_action);
    if (v != 1) {
      out->error_state = (int64_t)pick;
      return -7;
    }
    return 0;
  }
  *err = "action property: the host finds no violating step of the state the device flagged";
  return -6;
}

void ap_reset(tlcg_action_property* out) {
  std::memset(out, 0, sizeof *out);
  out->step_action = -1;
  out->error_state = -1;
}

template <typename W>
int run_model_action(const HostModel& hm, const UserProg* h_prog, const UserProg* d_prog, const tlcg_opts* o,
                     tlcg_action_property* out, LvTrace* tr, std::string* err) {
  const ModelGraph<W> g{hm.L, hm.n_init};
  return run_action(g, g, ProgStep<W>{hm.L, d_prog}, ProgStep<W>{hm.L, h_prog}, o, out, tr, err);
}

template <typename W>
int run_explicit_action(const uint32_t* row, const uint32_t* col, const uint8_t* verdict, uint32_t n, uint32_t n_init,
                        const tlcg_opts* o, tlcg_action_property* out, LvTrace* tr, std::string* err) {
  DevMem mem;
  ExplicitGraph<W> hg, dg;  // (without a P: ReachAll asks for none)
  if (const int rc = upload_graph(row, col, n, n_init, mem, &hg, &dg, err)) return rc;
  ByteStep<W> dev{dg.row, nullptr};
  if (const int rc = upload(mem, verdict, row[n], &dev.v, err)) return rc;
  return run_action(dg, hg, dev, ByteStep<W>{row, verdict}, o, out, tr, err);
}

// tlcg_action_eval_selftest: the program on pair i, one lane each
template <typename W>
__global__ __launch_bounds__(LV_BLOCK) void k_ap_eval(Layout L, const UserProg* prog, const u64* pairs, u64 n,
                                                      unsigned char* out) {
  constexpr int w = sizeof(W) / 8;
  const u64 stride = (u64)gridDim.x * LV_BLOCK;
  for (u64 i = (u64)blockIdx.x * LV_BLOCK + threadIdx.x; i < n; i += stride) {
    W s = (W)pairs[2 * i * w], t = (W)pairs[(2 * i + 1) * w];
    if constexpr (w == 2) {
      s |= (W)pairs[2 * i * w + 1] << 64;
      t |= (W)pairs[(2 * i + 1) * w + 1] << 64;
    }
    out[i] = (unsigned char)eval_user2<W>(L, *prog, 0, s, t);
  }
}

}  // namespace

extern "C" int tlcg_check_action_property(const tlcg_model* m, const tlcg_opts* o, const char* name,
                                          tlcg_action_property* out, uint64_t* states, int32_t* actions, int32_t cap,
                                          int32_t* len, char* err, int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (!m || !out || !name) return fail(-1, "null argument");
  ap_reset(out);
  if (len) *len = 0;
  HostModel hm;
  std::string e;
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  if (!hm.constraints.empty())
    return fail(-2, "the model has a CONSTRAINT: an action PROPERTY is not checked under a state constraint");
  const std::unique_ptr<UserProg> prog(new UserProg);
  if (compile_action_property(*m, hm, name, nullptr, prog.get(), &e) != 0) return fail(-2, e);
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  DevMem mem;
  UserProg* d_prog = nullptr;
  if (!mem.alloc(&d_prog, 1) ||
      hipMemcpy(d_prog, prog.get(), sizeof(UserProg), hipMemcpyHostToDevice) != hipSuccess)
    return fail(-5, "action property: device allocation failed (the program)");
  LvTrace tr;
  const int words = state_words(hm.L);
  const int rc = words == 1 ? run_model_action<u64>(hm, prog.get(), d_prog, o, out, &tr, &e)
                            : run_model_action<u128>(hm, prog.get(), d_prog, o, out, &tr, &e);
  out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc == -7)
    e = std::string("evaluating the action of property ") + name +
        " failed on a step of a reachable state (the last two states of the trace)";
  else if (rc)
    return fail(rc, e);
  out->trace_len = trace_copy_out(tr, words, states, actions, cap, len);
  return rc ? fail(rc, e) : 0;
}

extern "C" int tlcg_action_property_graph_selftest(const uint32_t* row, const uint32_t* col, const uint8_t* verdict,
                                                   uint32_t n, uint32_t n_init, int32_t words, const tlcg_opts* o,
                                                   tlcg_action_property* out, uint64_t* states, int32_t* actions,
                                                   int32_t cap, int32_t* len, char* err, int32_t err_cap) {
  const Fail fail{err, err_cap};
  if (!row || !out) return fail(-1, "null argument");
  if (words != 1 && words != 2) return fail(-1, "words must be 1 or 2");
  if (row[n] && (!col || !verdict)) return fail(-1, "null argument");
  ap_reset(out);
  if (len) *len = 0;
  std::string e;
  if (!graph_ok(row, col, n, n_init, &e)) return fail(-1, e);
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const auto t0 = std::chrono::steady_clock::now();
  LvTrace tr;
  int rc = words == 1 ? run_explicit_action<u64>(row, col, verdict, n, n_init, o, out, &tr, &e)
                      : run_explicit_action<u128>(row, col, verdict, n, n_init, o, out, &tr, &e);
  out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc == -7) rc = 0;  // (error_state says so)
  if (rc) return fail(rc, e);
  out->trace_len = trace_copy_out(tr, words, states, actions, cap, len);
  return 0;
}

extern "C" int tlcg_action_eval_selftest(const tlcg_model* m, const tlcg_opts* o, const char* name,
                                         const uint64_t* pairs, uint64_t n, uint8_t* out, char* err, int32_t cap) {
  const Fail fail{err, cap};
  if (!m || !name || (n && (!pairs || !out))) return fail(-1, "null argument");
  HostModel hm;
  std::string e;
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  const std::unique_ptr<UserProg> prog(new UserProg);
  if (compile_action_property(*m, hm, name, nullptr, prog.get(), &e) != 0) return fail(-2, e);
  if (n == 0) return 0;
  if (hipSetDevice(o ? o->device : 0) != hipSuccess) return fail(-4, "hipSetDevice failed");
  const int words = state_words(hm.L);
  DevMem mem;
  UserProg* d_prog = nullptr;
  u64* d_pairs = nullptr;
  unsigned char* d_out = nullptr;
  const u64 nw = 2 * n * (u64)words;
  if (!mem.alloc(&d_prog, 1) || !mem.alloc(&d_pairs, nw) || !mem.alloc(&d_out, n))
    return fail(-5, "action eval: device allocation failed");
  auto run = [&](std::string* err) -> int {
    LV_CHECK(hipMemcpy(d_prog, prog.get(), sizeof(UserProg), hipMemcpyHostToDevice));
    LV_CHECK(hipMemcpy(d_pairs, pairs, nw * sizeof(u64), hipMemcpyHostToDevice));
    const unsigned grid = lv_grid(n, lv_grid_cap());
    if (words == 1) k_ap_eval<u64><<<grid, LV_BLOCK>>>(hm.L, d_prog, d_pairs, n, d_out);
    else k_ap_eval<u128><<<grid, LV_BLOCK>>>(hm.L, d_prog, d_pairs, n, d_out);
    LV_CHECK(hipGetLastError());
    LV_CHECK(hipMemcpy(out, d_out, n, hipMemcpyDeviceToHost));
    return 0;
  };
  const int rc = run(&e);
  return rc ? fail(rc, e) : 0;
}
