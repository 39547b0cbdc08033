// pulsar-tlaplus_amd/csrc/component_lane.h -- the component engine's per-lane
// code pass with a bitmap FPSet and wave-uniform control (round 6).
//
// Like component_body.h, every lane runs TLC's FIFO BFS on its own component
// (compaction.tla:216-231): it expands each of its states (the compactor
// disjunct, BrokerCrash, the stutters), probes and inserts each successor in
// its own FPSet, evaluates every invariant of the cfg on each new state
// (:236-294) and stores each new state's 32-bit record (comp_record).  What
// changes is how a lane's FPSet and FIFO are laid out:
//
//   - FPSet: without a Producer every component walks the same code graph
//     (component_code.h), so the host finds a multiply-shift slot hash that is
//     injective on component 0's code set S (build_lane_phash, host_model.h:
//     T = 256 slots, the top 8 bits of code x a 24-bit multiplier), and a
//     workgroup-shared table owner[slot] = the code of S in that slot + 1.
//     A lane's FPSet is then one bit per slot (T / 32 LDS dwords in lane
//     columns: the lane's own bank, no conflicts), and FPSet.put of code c is
//     exact for any c: c is in the set iff owner[slot(c)] = c + 1 and the
//     lane's bit is set; a successor outside S (owner[slot(c)] != c + 1) means
//     this component's code graph is not S, and the component goes on to the
//     32-bit cascade pass, as one past the pass's capacity does.  A probe is
//     two independent LDS reads (the shared owner word, the lane's bit word)
//     instead of a slot read and then its queue entry, and an insert is two
//     LDS writes.
//   - invariants (round 7): code + 1 takes the low 16 bits of an owner word,
//     and the host writes the code's invariant features into the top 16
//     (component_code.h lane_inv_feat: the half of "does a built-in invariant
//     fail" that reads only the code).  The half that reads only the
//     component is a mask in one register (lane_inv_mask, once per
//     component), so an inserted successor's invariants are the probe's own
//     owner word >> 16, and-ed with the mask: non-zero exactly when one fails
//     (checked on every code and class of component,
//     tlcg_host_lane_inv_selfcheck).  Such a state goes to the rare branch,
//     where check_invariants_direct names the first failing invariant in cfg
//     order and its kind.  Every state still has its own invariants decided:
//     its own code's features against its own component's mask.
//   - stutters (round 7): the code's half of "Terminating is enabled" is a
//     flag of the compactor step's table entry (compactor_step_entry
//     STEP_TERM), the component's half one register.
//   - FIFO: the FPSet no longer points into the queue, so a lane keeps only
//     its unexpanded states, in a ring of LANE_R codes (lane columns); queue
//     positions are counters (the records' numbering is component_body.h's).
//   - control: the BFS loop runs while any lane of the wave is alive, with
//     every lane in it (a finished lane's updates are masked by selects, its
//     record stores go out of the buffer's range), so the per-level counts of
//     the lanes that close a level at one level were one DPP sum and one LDS
//     add instead of 64 same-address LDS adds (round 8 went back to an add
//     per lane, TLCG_LANE_LEVEL_LDS: the sum's own instructions cost more),
//     and the loop pays no exec-mask bookkeeping per branch.
//   - round 8: an owner entry is two words (component_code.h lane_owner_word:
//     code + 1 | features << 16 | the code's step-table index << 25, and the
//     code's dense index in S).  The ring queues the first word instead of
//     the bare code, so a dequeued state brings its step index with it, and
//     the lane's FPSet is one 64-bit register indexed by the dense index (S
//     has at most 62 codes) instead of T bits in LDS: a probe is one 64-bit
//     LDS read, an insert none.  FPSet.put stays exact: c is in the set iff
//     the low half of owner[slot(c)] is c + 1 and the lane's bit of that
//     entry's dense index is set.
//   - round 9: without a Producer the code transitions read nothing of
//     `messages` but its length, so the components of a cfg run in lockstep:
//     in a given iteration BrokerCrash (crashTimes < MaxCrashTimes) is enabled
//     in every live lane of a wave or in none, on G9 in 20 of a component's
//     62 expansions.  Each lane still evaluates the guard on its own state;
//     one ballot then picks one of two straight-line forms of the expansion
//     (`expand`, TLCG_LANE_CRASH_SKIP): with the second successor, which is
//     the kernel as it was and serves a lane without one as before, or
//     without it (no crash_step_c, no second probe, insert, ring write or
//     record).  The forms leave a few masks for the rare branch, which stays
//     one copy after they join (a copy in each form spilled), and the first
//     event of a batch goes to the result at the batch's end instead of
//     riding in two registers across every batch.
//   - round 10 (TLCG_LANE_PREFIX): the second word of an owner entry, the
//     code's dense index, is its position in S's own FIFO BFS walked in this
//     kernel's order (compactor successor, then BrokerCrash's, each appended
//     when new).  A component that walks S in that order inserts the code
//     with dense index `tail` at queue position `tail`, every time, so the
//     64-bit set and the ring re-derive what one comparison against `tail`
//     decides.  The lane keeps neither: FPSet.put of a successor t is its
//     probe as before (the lane's own t, lane_slot, owner[p], low half against
//     t + 1), then with d the entry's dense index: d < tail: in the set;
//     d == tail: new, at position tail; any other d: this component does not
//     walk S in S's order, and it goes to the cascade as one with a successor
//     outside S does (`out`: the expansion's inserts masked, the levels
//     counted so far kept).  The state to expand is byidx[head], a shared
//     table of S's owner words by dense index filled from owner[] at start.
//     This is exact for any component, by induction over the inserts on
//       I(tail): the lane's set is {codes of S with dense index < tail}, and
//                queue position i holds the code with dense index i, i < tail.
//     The root is checked to be S's code of dense index 0, so I(1) holds (or
//     the lane leaves before it expands anything).  Given I(tail) and a
//     successor t: the slot hash is injective on S, so the low half of
//     owner[slot(t)] is t + 1 exactly when t is in S, and then d is t's dense
//     index.  t outside S is not in a set of codes of S: the lane leaves, as
//     before this round.  d < tail: t is in the set by I(tail), nothing
//     changes.  d == tail: t is not in the set by I(tail) (dense indices are a
//     bijection), it is appended at position tail, and I(tail + 1) holds.
//     d > tail: t is new, but appending it would break I, so the lane leaves
//     with nothing of this expansion inserted.  The second successor of an
//     expansion is judged against the prefix after the first's insert
//     (tail + new1); when both are the same code the second finds d < tail +
//     1.  A lane that stays therefore computed, at every insert, exactly
//     what a private set and queue would have; nothing is assumed of the
//     component, and no successor is read from a table: each lane still
//     steps, hashes and probes its own state's successors.
// LDS per 64-lane workgroup (TLCG_LANE_PREFIX: byidx 0.25 KB instead of the
// ring, 3072 B; below, the figures without it): the ring R x 256 B (the host picks R per layout,
// jit.cpp / host_model.cpp lane_ring_entries: 8 entries, 2 KB, on G9; a wider
// frontier sends the component to the cascade), owner 2 KB, the step table
// 0.5 KB, the level sums 0.25 KB: 4864 B as before round 8 (then the ring 1
// KB, the bits 2 KB, owner 1 KB), 32 workgroups of the CU's 160 KB (vs 13.3
// KB for component_body.h), so registers, not LDS, set the occupancy.  (With
// TLCG_LANE_FP_REG=0 and the 32-bit ring it is 5888 B: 27 workgroups.)
#pragma once
#if !defined(__HIPCC_RTC__)
#include "component_body.h"
#endif

namespace tlcg {

#ifndef TLCG_LANE_R
#define TLCG_LANE_R 16
#endif
constexpr int LANE_R = TLCG_LANE_R;  // FIFO ring entries per lane (a power of 2; the hipRTC module defines it)
// the compactor disjunct through its update masks (component_code.h
// compactor_step_tab: one LDS read and a few bit operations instead of the six
// candidate successors of compactor_step_cb); 0: compactor_step_cb (A/B)
#ifndef TLCG_LANE_STEP_TAB
#define TLCG_LANE_STEP_TAB 1
#endif
// an inserted successor's built-in invariants from the feature word the owner
// table carries beside its code (component_code.h lane_inv_feat) and the
// component's mask; 0: check_invariants_cbt on each (A/B).  The user
// invariants' outcome tables are not folded in: a module with them keeps
// check_invariants_cbt.
#ifndef TLCG_LANE_INV_FEAT
#define TLCG_LANE_INV_FEAT 1
#endif
#if defined(TLCG_USER_INV) || defined(TLCG_LANE_INV_UNCOND)
#undef TLCG_LANE_INV_FEAT
#define TLCG_LANE_INV_FEAT 0
#endif
// round 8, each on by default and 0 for A/B:
// the ring queues a state's 32-bit owner word instead of its bare code, so a
// dequeued state brings its step-table index with it (bits 25..30,
// component_code.h lane_owner_word) and the ffbh / phase / r index chain goes
#ifndef TLCG_LANE_OWNER_RING
#define TLCG_LANE_OWNER_RING 1
#endif
#if !TLCG_LANE_STEP_TAB  // (the index is the step table's)
#undef TLCG_LANE_OWNER_RING
#define TLCG_LANE_OWNER_RING 0
#endif
// the lane's FPSet as one 64-bit register, indexed by the code's dense index
// in S (the owner entry's second word) instead of T bits in LDS lane columns
#ifndef TLCG_LANE_FP_REG
#define TLCG_LANE_FP_REG 1
#endif
// a level's counts as one LDS add per adding lane: no ballots, DPP sum or
// lane reads at a level end (0: round 6's wave sum and one add, A/B)
#ifndef TLCG_LANE_LEVEL_LDS
#define TLCG_LANE_LEVEL_LDS 1
#endif
// round 9: the BrokerCrash successor's code (crash_step_c, its probe, insert,
// ring write and record) only in the iterations where some live lane of the
// wave has BrokerCrash enabled; 0: in every iteration (A/B)
#ifndef TLCG_LANE_CRASH_SKIP
#define TLCG_LANE_CRASH_SKIP 1
#endif
// round 10: the lane's FPSet and FIFO as a prefix of S's dense order, verified
// at every insert (the header comment): membership is `dense index < tail`,
// the state to expand is byidx[head]; no fp register, no ring.  0: round 9's
// kernel (A/B).  It needs the two-word owner entry and the owner word.
#ifndef TLCG_LANE_PREFIX
#define TLCG_LANE_PREFIX 1
#endif
#if !TLCG_LANE_FP_REG || !TLCG_LANE_OWNER_RING
#undef TLCG_LANE_PREFIX
#define TLCG_LANE_PREFIX 0
#endif
// test only, TLCG_LANE_PREFIX_BREAK=p: the insert at queue position p counts
// as one out of order, so every lane leaves for the cascade there, mid-wave,
// with the levels it has counted (no cfg of the spec is known to take that
// path by itself)

// which form of the expansion component_lane_body's `expand` compiles
template <bool B>
struct lane_with2 {
  static constexpr bool value = B;
};

// the sum over the wave of x (every lane active), in a scalar
__device__ __forceinline__ uint32_t lane_wave_sum(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);  // row_shr:8
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
         (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

template <int K, bool OD = false>
__device__ __forceinline__ void component_lane_body(const CompArgs& a, const Layout& L) {
  static_assert(K <= 64, "records and the 16-bit level sums take K <= 64");
  // level_add's wave sum keeps distinct and generated in 16-bit halves: a
  // lane expands at most K - 2 states (`full`), each generates at most 4
  // (the compactor's, BrokerCrash's, two stutters), 64 lanes are summed
  static_assert(64 * (K - 2) * 4 < 65536, "level_add's 16-bit halves");
  constexpr int T = LANE_T, NW = T / 32, R = LANE_R;
  constexpr int LV = TLCG_CODE_MAXLV < COMP_MAXLV ? TLCG_CODE_MAXLV : COMP_MAXLV;  // levels tracked
#if TLCG_LANE_OWNER_RING
  typedef uint32_t ring_t;                     // (owner words)
#else
  typedef uint16_t ring_t;                     // (codes)
#endif
#if TLCG_LANE_PREFIX
  // S in dense order: byidx[d] = the owner word of the code with dense index d
  // (0 past |S|), shared: a lane's queue position i holds byidx[i]
  __shared__ uint32_t byidx[64];
  (void)R;
#else
  __shared__ ring_t ring[R][64];               // the lanes' FIFOs (unexpanded states)
#endif
#if TLCG_LANE_FP_REG
  __shared__ u64 owner[T];                     // slot s: its owner word (0: none) | dense index << 32, shared
#else
  __shared__ uint32_t bits[NW][64];            // the lanes' FPSets: bit s of lane l = bit s % 32 of bits[s / 32][l]
  __shared__ uint32_t owner[T];                // slot s: its owner word (code + 1 in the low half; 0: none), shared
#endif
  // per level: distinct (low 32) + generated (high 32); OD: then the expansions
  // that discovered 0, 1 and 2 new states (kept here, not in registers of the
  // loop: the kernel stays within the 64 VGPRs of 8 waves per SIMD)
  constexpr int LVS = LV + (OD ? 3 : 0);
  static_assert(LVS <= 64 && (K - 2) * 4 + 1 < 256, "one lane per level sum; OD packs three counts above lgen's 8 bits");
  __shared__ unsigned long long lvl_sh[LVS];
#if TLCG_LANE_STEP_TAB
  __shared__ u64 steps[STEP_TAB];              // the compactor disjunct's update masks (compactor_step_entry)
#endif
  const int lane = threadIdx.x;
  const int mb = L.msg_sh + L.N * L.mw;
  const uint32_t mult = a.lane_mult;
#if TLCG_LANE_FP_REG
  for (int i = lane; i < T; i += 64) owner[i] = (u64)a.lane_owner[2 * i] | ((u64)a.lane_owner[2 * i + 1] << 32);
#else
  for (int i = lane; i < T; i += 64) owner[i] = a.lane_owner[2 * i];
#endif
#if TLCG_LANE_STEP_TAB
  for (int i = lane; i < STEP_TAB; i += 64) steps[i] = compactor_step_entry(L, i);
#endif
  if (lane < LVS) lvl_sh[lane] = 0;
  uint32_t gen = 0, dist = 0, nexp = 0;  // (nexp: states expanded by the components that finish here)
#if TLCG_LANE_PREFIX
  byidx[lane] = 0u;
  __syncthreads();
  for (int i = lane; i < T; i += 64) {
    const uint32_t w = a.lane_owner[2 * i], d = a.lane_owner[2 * i + 1];
    if (w && d < 64u) byidx[d] = w;  // (the dense indices are a bijection onto 0..|S| - 1: one writer each)
  }
#endif
  __syncthreads();
  // a level's per-lane counts (x: distinct | generated << 16) into lvl_sh: one
  // LDS add per adding lane (round 8: at 20 level ends per 62 iterations the
  // same-address adds cost less than the ballots, the DPP sum and the lane
  // reads that saved them); TLCG_LANE_LEVEL_LDS=0: one DPP sum when every
  // lane that adds adds at one level, else per lane
  auto level_add = [&](bool add, int lvc, uint32_t x) {
#if TLCG_LANE_LEVEL_LDS
    if (add) atomicAdd(&lvl_sh[lvc], (unsigned long long)(x & 0xFFFFu) | ((unsigned long long)(x >> 16) << 32));
#else
    const unsigned long long m = __ballot(add);
    if (!m) return;
    const int l0 = __builtin_amdgcn_readlane(lvc, __ffsll((long long)m) - 1);
    if (!__ballot(add && lvc != l0)) {
      const uint32_t s = lane_wave_sum(add ? x : 0u);
      if (lane == 0) atomicAdd(&lvl_sh[l0], (unsigned long long)(s & 0xFFFFu) | ((unsigned long long)(s >> 16) << 32));
    } else if (add) {
      atomicAdd(&lvl_sh[lvc], (unsigned long long)(x & 0xFFFFu) | ((unsigned long long)(x >> 16) << 32));
    }
#endif
  };
  for (u64 b = blockIdx.x; b * 64 < a.n_comp; b += gridDim.x) {
    const u64 ci = b * 64 + (u64)lane;
    const bool act = ci < a.n_comp;
    // cascade entries carry the levels an earlier pass already counted (bits 40..)
    const u64 entry = act ? (a.list ? a.list[ci] : a.comp0 + ci) : 0;
    const u64 idx0 = entry & ((1ull << 40) - 1);
    const int counted = (int)(entry >> 40);
#if TLCG_LANE_PREFIX
    // (the lane's FPSet is the codes of S with dense index < tail)
#elif TLCG_LANE_FP_REG
    u64 fp = 0;  // the lane's FPSet: bit d = the code of S with dense index d
#else
#pragma unroll
    for (int i = 0; i < NW; ++i) bits[i][lane] = 0u;  // (the lane's own columns)
#endif
    const u64 s0 = init_state(L, idx0);
    CodeConsts ccon = code_consts(L, comp_msgs_init(L, s0));
#ifdef TLCG_USER_INV
    code_consts_user(L, ccon);  // the user invariants' outcome tables of this component
#endif
#if TLCG_LANE_INV_FEAT
    const uint32_t cmask = lane_inv_mask(L, ccon);  // the features that are failures in this component
#endif
#if TLCG_LANE_STEP_TAB
    const int term_c = lane_term_consts(L, ccon);
#endif
    // the records of this batch: [K][64] 32-bit words, position p of lane l at
    // (p x 64 + l) x 4; a store at an offset past the range is dropped
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<uint32_t*>(a.store) + b * (u64)K * 64, (short)0, K * 64 * 4, 0x00020000);
    constexpr int OOB = 0x7fffffff;
    const unsigned loff = (unsigned)lane * 4u;
    int head = 0, tail = 0, level = 0, lvl_start = 0, lvl_end = 0;
    // alive: the BFS goes on; stop: an error was found, so the lane finishes
    // the current level and stops at its end (end-of-level counts, as every
    // engine reports them); ovf: the component goes on to the cascade
    bool alive = act, ovf = false, stop = false;
    uint32_t lgen = 0, lvgen = 0;  // (OD: bits 8.., expansions by new states discovered)
    u64 lev = NO_EVENT;
    const lkey k0 = act ? (lkey)(s0 >> mb) : 0;
    const ckey c0 = code_encode(L, k0);
    const unsigned p0 = lane_slot(c0, mult);
    const uint32_t ow0 = (uint32_t)owner[p0];
#if TLCG_LANE_PREFIX
    // (the prefix starts at the root: S's code of dense index 0)
    const bool root_ok = (ow0 & 0xFFFFu) == c0 + 1u && (uint32_t)(owner[p0] >> 32) == 0u;
#else
    const bool root_ok = (ow0 & 0xFFFFu) == c0 + 1u;
#endif
    if (act && (code_decode(L, ccon, c0) != k0 || !root_ok)) {
      // no code, or not the code graph the slots were built for: the cascade
      ovf = true;
      alive = false;
    }
    if (alive) {
#if TLCG_LANE_PREFIX
      // (position 0 is byidx[0], the set is [0, tail))
#elif TLCG_LANE_FP_REG
      fp = 1ull << (uint32_t)(owner[p0] >> 32);
#else
      bits[p0 >> 5][lane] = 1u << (p0 & 31);
#endif
#if TLCG_LANE_PREFIX
#elif TLCG_LANE_OWNER_RING
      ring[0][lane] = ow0;
#else
      ring[0][lane] = (uint16_t)c0;
#endif
      tail = 1;
      __builtin_amdgcn_raw_buffer_store_b32(comp_record(c0, 0, 0), rsrc, (int)loff, 0, 0);  // (position 0: the root)
      lgen = 1;
      const int c = check_invariants_direct(L, ccon, c0);
      if (c >= 0) {  // an initial state violates: level 0 is complete, nothing is expanded
        lev = make_comp_event(0, idx0, 0, 0, (c & 1) ? EVK_INV_ERROR : EVK_VIOLATION, c >> 1);
        alive = false;
        stop = true;
      }
    }
    lvl_end = tail;
#if TLCG_LANE_OWNER_RING
    uint32_t cur = ow0;  // the state to expand: its owner word
#else
    ckey cur = c0;
#endif
    while (__ballot(alive)) {
      const int tail0 = tail;
#if TLCG_LANE_OWNER_RING
      // (a finished lane goes on with whatever its ring holds: the index is
      // kept inside the table, every slot is below T)
      const ckey s = (cur & 0xFFFFu) - 1u;
#if TLCG_LANE_PREFIX
      uint32_t nxt = 0;
#else
      uint32_t nxt = 0, first_new = 0;
#endif
#else
      const ckey s = cur;
      ckey nxt = 0, first_new = 0;
#endif
      // what the rare branch reads of an expansion: a deadlock, each inserted
      // successor's invariants not known to hold (u1, u2) and how far they are
      // decided (q1, q2: first failing + 1, or INV_UNKNOWN + 1)
      bool out = false, rare = false, dl = false, u1 = false, u2 = false;
      int q1 = INV_UNKNOWN + 1, q2 = INV_UNKNOWN + 1;
      ckey t = 0;
      int action = 0;
#if TLCG_LANE_OWNER_RING
#if TLCG_LANE_PREFIX
      // the next state to expand: position head + 1 holds S's code of that
      // dense index whatever this expansion inserts, so the read goes out
      // with the step entry's (the lanes of a wave read one address: a
      // broadcast; a finished lane's index stays inside the table)
      nxt = byidx[(head + 1) & 63];
#else
      nxt = ring[(head + 1) & (R - 1)][lane];
#endif
      const uint32_t six = (cur >> LANE_OWNER_STEP_SH) & (uint32_t)(STEP_TAB - 1);
      uint32_t term = 0;
      const int r = compactor_step_ent(L, ccon, steps[six], six & 7u, s, &t, &action, &term);  // compaction.tla:221-226
#else
      nxt = ring[(head + 1) & (R - 1)][lane];
#if TLCG_LANE_STEP_TAB
      uint32_t term = 0;
      const int r = compactor_step_tab(L, ccon, steps, s, &t, &action, &term);  // compaction.tla:221-226
#else
      const int r = compactor_step_cb(L, ccon, s, &t, &action);
#endif
#endif
      // one expansion, straight-line.  W2: with the BrokerCrash successor;
      // without it nothing of the second probe is left (no t2, no owner[p2]
      // read, no second insert, ring write or record store)
      auto expand = [&](auto with2) __attribute__((always_inline)) {
        constexpr bool W2 = decltype(with2)::value;
        ckey t2 = 0;
        bool crash = false;
        if constexpr (W2) crash = crash_step_c(L, s, &t2) != 0;     // :227
        // FPSet.put of both successors: slot, the shared owner, the lane's bits
        const unsigned p1 = lane_slot(t, mult), p2 = W2 ? lane_slot(t2, mult) : 0u;
#if TLCG_LANE_FP_REG
        const u64 oe1 = owner[p1], oe2 = W2 ? owner[p2] : 0ull;
        const uint32_t o1 = (uint32_t)oe1, o2 = (uint32_t)oe2;
#else
        const uint32_t o1 = owner[p1], o2 = W2 ? owner[p2] : 0u;
        const uint32_t w1 = bits[p1 >> 5][lane];
        uint32_t w2 = W2 ? bits[p2 >> 5][lane] : 0u;
#endif
#ifndef TLCG_LANE_NO_SCHED_BARRIER
        // (the reads issued together, before anything that consumes them or
        // writes LDS: one round trip per expansion, not two)
        __builtin_amdgcn_sched_barrier(0);
#endif
        const bool e1 = alive && r == 1, e2 = W2 && alive && crash;
        // (the low half of an owner word: the code + 1; above it its features)
        const bool in1 = (o1 & 0xFFFFu) == t + 1u, in2 = W2 && (o2 & 0xFFFFu) == t2 + 1u;
        // a successor outside the code set: this component is not S's, the cascade
        out = (e1 && !in1) || (e2 && !in2);
        bool new2 = false;
#if TLCG_LANE_PREFIX
        // FPSet.put against the prefix [0, tail): a code of S with dense index
        // d is in the set iff d < tail; one not in it must be the next of S's
        // order (d == tail, for the second successor after the first's
        // insert), or this component does not walk S in S's order: the
        // cascade, as for a successor outside S
        const uint32_t d1 = (uint32_t)(oe1 >> 32), ut = (uint32_t)tail;
        const bool n1 = e1 && in1 && d1 >= ut;
        bool bad = n1 && d1 != ut;
#ifdef TLCG_LANE_PREFIX_BREAK
        bad = bad || (n1 && tail == (TLCG_LANE_PREFIX_BREAK));
#endif
        bool n2 = false;
        if constexpr (W2) {
          const uint32_t d2 = (uint32_t)(oe2 >> 32), ut2 = ut + (n1 ? 1u : 0u);
          n2 = e2 && in2 && d2 >= ut2;
          bad = bad || (n2 && d2 != ut2);
#ifdef TLCG_LANE_PREFIX_BREAK
          bad = bad || (n2 && (int)ut2 == (TLCG_LANE_PREFIX_BREAK));
#endif
        }
        out = out || bad;
        const bool new1 = n1 && !out;
        new2 = n2 && !out;
#elif TLCG_LANE_FP_REG
        // (a dense index is below 62: build_lane_phash)
        const u64 b1 = 1ull << (uint32_t)(oe1 >> 32);
        const bool new1 = e1 && in1 && !(fp & b1) && !out;
        fp |= new1 ? b1 : 0ull;  // (the second sees the first's insert)
        if constexpr (W2) {
          const u64 b2 = 1ull << (uint32_t)(oe2 >> 32);
          new2 = e2 && in2 && !(fp & b2) && !out;
          fp |= new2 ? b2 : 0ull;
        }
#else
        const uint32_t b1 = 1u << (p1 & 31);
        const bool new1 = e1 && in1 && !(w1 & b1) && !out;
        bits[p1 >> 5][lane] = new1 ? w1 | b1 : w1;
        if constexpr (W2) {
          const uint32_t b2 = 1u << (p2 & 31);
          if ((p2 >> 5) == (p1 >> 5) && new1) w2 |= b1;  // (the second sees the first's insert)
          new2 = e2 && in2 && !(w2 & b2) && !out;
          bits[p2 >> 5][lane] = new2 ? w2 | b2 : w2;
        }
#endif
        // the queue (the ring: a successor not inserted is overwritten or never
        // read) and each new state's record at its position
#if TLCG_LANE_PREFIX
        // (no queue to write: position tail holds byidx[tail], just verified)
#elif TLCG_LANE_OWNER_RING
        ring[tail & (R - 1)][lane] = o1;
        if constexpr (W2) ring[(tail + (new1 ? 1 : 0)) & (R - 1)][lane] = o2;
#else
        ring[tail & (R - 1)][lane] = (uint16_t)t;
        if constexpr (W2) ring[(tail + (new1 ? 1 : 0)) & (R - 1)][lane] = (uint16_t)t2;
#endif
#ifndef TLCG_NO_STORE  // (experiment only: measures what the records cost)
        __builtin_amdgcn_raw_buffer_store_b32(comp_record(t, head, action), rsrc,
                                              new1 ? (int)((unsigned)tail * 256u + loff) : OOB, 0, 0);
        if constexpr (W2)
          __builtin_amdgcn_raw_buffer_store_b32(comp_record(t2, head, ACT_CRASH), rsrc,
                                                new2 ? (int)((unsigned)(tail + (new1 ? 1 : 0)) * 256u + loff) : OOB,
                                                0, 0);
#endif
#if TLCG_LANE_PREFIX
#elif TLCG_LANE_OWNER_RING
        first_new = W2 ? (new1 ? o1 : o2) : o1;
#else
        first_new = W2 ? (new1 ? t : t2) : t;
#endif
        tail += (new1 ? 1 : 0) + (new2 ? 1 : 0);
#if TLCG_LANE_STEP_TAB
        const int nsucc = (e1 ? 1 : 0) + (e2 ? 1 : 0) + (alive ? selfloop_count_tab(L, term_c, term) : 0);  // + stutters
#else
        const int nsucc = (e1 ? 1 : 0) + (e2 ? 1 : 0) + (alive ? selfloop_count_c(L, ccon, s) : 0);  // + stutters
#endif
        lvgen += (unsigned)nsucc;
        if constexpr (OD) lgen += alive ? 256u << (8 * (tail - tail0)) : 0u;  // new states this expansion discovered
        // the inserted successors' invariants (first failing + 1; INV_UNKNOWN
        // + 1: the rare branch settles it -- a failing feature, or an outcome
        // table that left it to the programs)
#if TLCG_LANE_INV_FEAT && !defined(TLCG_NO_INV)
        // (a feature of the code that is a failure in this component: which
        // invariant and how, the rare branch says)
        u1 = new1 && ((o1 >> 16) & cmask);
        if constexpr (W2) u2 = new2 && ((o2 >> 16) & cmask);
#elif !defined(TLCG_NO_INV)  // (TLCG_NO_INV: experiment only, measures what the invariants cost)
#ifdef TLCG_LANE_INV_UNCOND  // (A/B: both evaluated, no branch)
        q1 = check_invariants_cbt(L, ccon, t) + 1;
        if constexpr (W2) q2 = check_invariants_cbt(L, ccon, t2) + 1;
#else
        q1 = new1 ? check_invariants_cbt(L, ccon, t) + 1 : 0;
        if constexpr (W2) q2 = new2 ? check_invariants_cbt(L, ccon, t2) + 1 : 0;
#endif
        u1 = new1 && q1 != 0;
        if constexpr (W2) u2 = new2 && q2 != 0;
#endif
        // an action error (no successor from the failing action; the others
        // still count, as k_expand), a deadlock and the successors' invariant
        // events in one rare branch, after the two forms join
        dl = nsucc == 0 && L.check_deadlock;
        rare = alive && ((r == 2) | dl | u1 | u2);
      };
#if TLCG_LANE_CRASH_SKIP
      // BrokerCrash's guard on this lane's state; the second successor's code
      // runs only when some live lane of the wave has one (one uniform branch)
      if (__ballot(alive && crash_enabled_c(L, s))) expand(lane_with2<true>{});
      else expand(lane_with2<false>{});
#else
      expand(lane_with2<true>{});
#endif
      if (__ballot(rare)) {
        if (rare) {
          int ev1 = u1 ? q1 : 0, ev2 = u2 ? q2 : 0;
          ckey t2 = 0;
          if (u2) crash_step_c(L, s, &t2);  // (u2: the form with BrokerCrash ran, and this lane's is enabled)
#pragma nounroll
          for (int i = 0; i < 2; ++i) {
            if ((i ? ev2 : ev1) == INV_UNKNOWN + 1) {
              const int e = check_invariants_direct(L, ccon, i ? t2 : t) + 1;
              if (i) ev2 = e;
              else ev1 = e;
            }
          }
          u64 k = r == 2 ? make_comp_event(level + 1, idx0, head, action, EVK_ACTION_ERROR, action)
                  : dl ? make_comp_event(level + 1, idx0, head, 15, EVK_DEADLOCK, 0)
                                                   : NO_EVENT;
          if (ev1) k = min(k, make_comp_event(level + 1, idx0, head, action, ((ev1 - 1) & 1) ? EVK_INV_ERROR : EVK_VIOLATION, (ev1 - 1) >> 1));
          if (ev2) k = min(k, make_comp_event(level + 1, idx0, head, ACT_CRASH, ((ev2 - 1) & 1) ? EVK_INV_ERROR : EVK_VIOLATION, (ev2 - 1) >> 1));
          lev = min(lev, k);
          stop = stop || k != NO_EVENT;  // (no event: every unknown outcome held)
        }
      }
      if (alive) ++head;
#if TLCG_LANE_PREFIX
      // (a live lane's head went up by one; a finished lane expands nothing,
      // whatever it holds)
      cur = nxt;
#else
      cur = head < tail0 ? nxt : first_new;  // position head was filled by this expansion
#endif
      bool brk = alive && head >= tail;      // the component ran out
      // level `level` = [lvl_start, lvl_end) complete and expanded
      const bool ended = alive && head == lvl_end;
      if (__ballot(ended)) {
        const int lvc = level < LV ? level : LV - 1;
        level_add(ended && level >= counted, lvc, (uint32_t)(lvl_end - lvl_start) | (lvgen << 16));
        if (ended) {
          lgen += lvgen;
          lvgen = 0;
          ++level;
          lvl_start = head;  // the new level is [head, tail)
          lvl_end = tail;
          const bool deep = level >= LV;  // more levels than tracked on chip: cascade
          ovf = ovf || deep;
          brk = brk || deep || stop;  // stop: an error in the level just expanded, the new level is not expanded
        }
      }
      // room for both successors of the next expansion, in the records and
      // in the ring (checked once per expansion; a component of K - 1 or K
      // states goes on to the cascade too)
#if TLCG_LANE_PREFIX
      // (no ring to fill; every insert had dense index tail, and a dense index
      // is below 62 (build_lane_phash, and byidx holds 64), so tail <= 62 =
      // K - 2 at K = 64: the test is left to a smaller K)
      const bool full = K < 64 && alive && !brk && tail > K - 2;
#else
      const bool full = alive && !brk && (tail > K - 2 || tail - head > R - 2);
#endif
      ovf = ovf || full || out;
      alive = alive && !(brk || full || out);
    }
    if (act && ovf) {
      // the next pass redoes the component and counts only levels >= `level`
      // (the complete ones were counted here, at their transitions)
      const unsigned long long k = atomicAdd(a.ovf_n, 1ull);
      a.ovf_list[k] = idx0 | ((u64)(level > counted ? level : counted) << 40);
    }
    // the last level [lvl_start, tail) was discovered, not expanded (empty
    // when the component ran out)
    const bool fin = act && !ovf;
    const int lvc = level < LV ? level : LV - 1;
    level_add(fin && tail > lvl_start && level >= counted, lvc, (uint32_t)(tail - lvl_start));
    if constexpr (OD) {  // (every lane here: one wave sum and one LDS add per count, as level_add)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const u64 w = wave_sum_u64(fin ? (lgen >> (8 + 8 * i)) & 0xFFu : 0u);
        if (lane == 0 && w) atomicAdd(&lvl_sh[LV + i], (unsigned long long)w);
      }
    }
    if (fin) {
      gen += OD ? lgen & 0xFFu : lgen;
      dist += (uint32_t)tail;
      nexp += (uint32_t)head;
    }
    // the batch's first event, once per wave (rare: not kept in a register
    // across the batches, where it cost the BFS loop two VGPRs)
    if (__ballot(fin && lev != NO_EVENT)) {
      unsigned long long ev = fin ? (unsigned long long)lev : NO_EVENT;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) ev = min(ev, (unsigned long long)__shfl_xor(ev, off));
      if (lane == 0) atomicMin(a.event, ev);
    }
  }
  const u64 g64 = wave_sum_u64(gen), d64 = wave_sum_u64(dist), x64 = wave_sum_u64(nexp);
  __syncthreads();
  const u64 so = a.nstripe > 1 ? (u64)(blockIdx.x % (unsigned)a.nstripe) * a.stripe : 0;  // this workgroup's copy
  if (lane == 0) {
    if (x64 && a.expansions) atomicAdd(&a.expansions[so], (unsigned long long)x64);
    if (g64) atomicAdd(&a.totals[so + 0], (unsigned long long)g64);
    if (d64) atomicAdd(&a.totals[so + 1], (unsigned long long)d64);
  }
  if constexpr (OD)
    if (lane < 3 && lvl_sh[LV + lane]) atomicAdd(&a.outdeg[so + lane], lvl_sh[LV + lane]);
  if (lane < LV && lvl_sh[lane]) {
    atomicAdd(&a.lvl[so + lane], lvl_sh[lane] & 0xffffffffull);
    if (lvl_sh[lane] >> 32) atomicAdd(&a.lvl_gen[so + lane], lvl_sh[lane] >> 32);
  }
}

}  // namespace tlcg
