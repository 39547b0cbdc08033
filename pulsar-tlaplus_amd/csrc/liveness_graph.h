// pulsar-tlaplus_amd/csrc/liveness_graph.h -- the graphs the liveness pass
// (liveness.hip) walks, and its host-side lasso extraction.
//
// The pass is written over a graph policy G, host and device:
//   word           the packed state (u64, or u128 for two-word states)
//   n_init()       initial states, init(i) the i-th
//   is_p(s)        P, the property's predicate: a P state ends every path
//   moves_bound()  moves of a state are numbered 0 .. moves_bound() - 1
//   move(s, k, &t, &ord)  1 with *t / *ord (the ordinal kept in the parent
//                  reference) when move k exists and changes the state, 0
//                  otherwise (a self-loop is never a move), 2 on an
//                  evaluation error
//   ord_bits()     bits of an ordinal, action_of(ord) what a trace reports
// ModelGraph is the spec's graph over a Layout; ExplicitGraph is a CSR graph
// the caller supplies (tlcg_liveness_graph_selftest), which reaches what the
// spec cannot: G' of the spec is acyclic for every cfg.
//
// Plain C++ compiles this header too (tests/fuzz/lasso_fuzz.cpp runs
// lasso_walk under sanitizers).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "model.h"

namespace tlcg {

template <typename W>
TLCG_HD bool lv_p(const Layout& L, W s) {
  return terminating_enabled(L, s);
}

// Move k of s (k < moves_bound(L)): Producer's nkv successors (key outer,
// value inner), then the compactor disjunct, then BrokerCrash.  Returns 1 with
// *t / *ord set when that move exists and changes the state, 0 otherwise, 2 on
// an evaluation error.  Stutters (Consumer, Terminating) are never moves.
template <typename W>
TLCG_HD int lv_move(const Layout& L, W s, int k, W* t, int* ord) {
  const int np = L.producer ? L.nkv : 0;
  if (k < np) {
    const int len = st_len(L, s);
    if (len >= L.N) return 0;
    *t = producer_succ(L, s, len, k);
    *ord = ordinal_of(L, ACT_PRODUCER, k);
    return *t != s;
  }
  int act = 0;
  if (k == np) {
    const int r = compactor_step(L, s, t, &act);
    if (r == 2) return 2;
    *ord = ordinal_of(L, act, 0);
    return r == 1 && *t != s;
  }
  if (!crash_step(L, s, t)) return 0;
  *ord = ordinal_of(L, ACT_CRASH, 0);
  return *t != s;
}
TLCG_HD int moves_bound(const Layout& L) { return (L.producer ? L.nkv : 0) + 2; }

// the spec's state graph
template <typename W>
struct ModelGraph {
  using word = W;
  Layout L;
  u64 n_init_;
  TLCG_HDM u64 n_init() const { return n_init_; }
  TLCG_HDM W init(u64 i) const { return init_state<W>(L, i); }
  TLCG_HDM bool is_p(W s) const { return lv_p(L, s); }
  TLCG_HDM int moves_bound() const { return tlcg::moves_bound(L); }
  TLCG_HDM int move(W s, int k, W* t, int* ord) const { return lv_move(L, s, k, t, ord); }
  TLCG_HDM int ord_bits() const { return L.ord_bits; }
  TLCG_HDM int action_of(int ord) const { return action_of_ordinal(L, ord); }
};

// A CSR graph with a P byte per node: nodes 0 .. n_init_ - 1 are initial, move
// k of node v is edge row[v] + k (ordinal k, also the action a trace reports).
// Node v's word is v; as a two-word state its high half is v >> 3, so eight
// nodes share a high half of the wide FPSet's slot.  The arrays are device
// memory in the instance the kernels get, host memory in the host's.
template <typename W>
struct ExplicitGraph {
  using word = W;
  const uint32_t* row;  // n + 1 offsets into col
  const uint32_t* col;
  const unsigned char* p;
  uint32_t n, n_init_;
  int max_deg, ord_bits_;
  TLCG_HDM static W word_of(uint32_t v) {
    if constexpr (sizeof(W) == 8) return (W)v;
    else return (W)v | ((W)(v >> 3) << 64);
  }
  TLCG_HDM static uint32_t node_of(W s) { return (uint32_t)(u64)s; }
  TLCG_HDM u64 n_init() const { return n_init_; }
  TLCG_HDM W init(u64 i) const { return word_of((uint32_t)i); }
  TLCG_HDM bool is_p(W s) const { return p[node_of(s)] != 0; }
  TLCG_HDM int moves_bound() const { return max_deg; }
  TLCG_HDM int move(W s, int k, W* t, int* ord) const {
    const uint32_t v = node_of(s), e = row[v] + (uint32_t)k;
    if (e >= row[v + 1]) return 0;
    *t = word_of(col[e]);
    *ord = k;
    return *t != s;
  }
  TLCG_HDM int ord_bits() const { return ord_bits_; }
  TLCG_HDM int action_of(int ord) const { return ord; }
};

// Checks a caller's CSR arrays (every index the kernels form stays inside
// them) and fills the graph but for its pointers; false with a message.
template <typename W>
inline bool explicit_graph_shape(const uint32_t* row, const uint32_t* col, uint32_t n, uint32_t n_init,
                                 ExplicitGraph<W>* g, std::string* err) {
  if (n_init > n || n >= (1u << 31)) {
    *err = "graph: n_init <= n < 2^31 expected";
    return false;
  }
  if (row[0] != 0) {
    *err = "graph: row[0] must be 0";
    return false;
  }
  uint32_t deg = 0;
  for (uint32_t v = 0; v < n; ++v) {
    if (row[v + 1] < row[v]) {
      *err = "graph: row must not decrease";
      return false;
    }
    deg = std::max(deg, row[v + 1] - row[v]);
  }
  if (deg > (1u << 20)) {
    *err = "graph: out-degree above 2^20";
    return false;
  }
  for (uint32_t e = 0; e < row[n]; ++e)
    if (col[e] >= n) {
      *err = "graph: an edge leaves the node range";
      return false;
    }
  g->n = n;
  g->n_init_ = n_init;
  g->max_deg = (int)deg;
  g->ord_bits_ = std::max(1, bits_for(deg ? deg - 1 : 0));
  return true;
}

// Host: the states left after peeling (st, with their BFS indices idx,
// ascending) lie on cycles or after them.  Peel them from the other side
// (drop states none of whose successors is left) so that every remaining state
// has a successor among them, then walk from the shallowest remaining state,
// taking the first remaining successor in move order, until a state repeats.
// The lasso: *g_entry (the repeated state's BFS index), the cycle's other
// states with the actions into them, and the action back to the entry.
template <typename G>
int lasso_walk(const G& g, const std::vector<typename G::word>& st, const std::vector<uint32_t>& idx, u64* g_entry,
               std::vector<u128>* cyc, std::vector<int>* cyc_act, int* back_action, std::string* err) {
  using W = typename G::word;
  using u32 = uint32_t;
  const size_t n = st.size();
  std::vector<std::pair<W, u32>> by_state(n);
  for (size_t i = 0; i < n; ++i) by_state[i] = {st[i], (u32)i};
  std::sort(by_state.begin(), by_state.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  auto find = [&](W t) -> long {
    auto it = std::lower_bound(by_state.begin(), by_state.end(), t,
                               [](const std::pair<W, u32>& a, W v) { return a.first < v; });
    return it != by_state.end() && it->first == t ? (long)it->second : -1;
  };
  const int kmax = g.moves_bound();
  std::vector<std::vector<std::pair<u32, int>>> succ(n);  // (state, ordinal) in move order
  std::vector<std::vector<u32>> pred(n);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < kmax; ++k) {
      W t;
      int ord = 0;
      if (g.move(st[i], k, &t, &ord) != 1 || g.is_p(t)) continue;
      const long j = find(t);
      if (j < 0) continue;
      succ[i].push_back({(u32)j, ord});
      pred[j].push_back((u32)i);
    }
  std::vector<size_t> outc(n);
  std::vector<char> alive(n, 1);
  std::vector<u32> q;
  for (size_t i = 0; i < n; ++i)
    if ((outc[i] = succ[i].size()) == 0) q.push_back((u32)i);
  while (!q.empty()) {
    const u32 v = q.back();
    q.pop_back();
    alive[v] = 0;
    for (u32 p : pred[v])
      if (alive[p] && --outc[p] == 0) q.push_back(p);
  }
  size_t start = 0;
  while (start < n && !alive[start]) ++start;
  if (start == n) {
    *err = "liveness: peeling left states but no cycle among them";
    return -1;
  }
  std::vector<long> seen(n, -1);
  std::vector<u32> walk;
  std::vector<int> ords;
  u32 v = (u32)start;
  while (seen[v] < 0) {
    seen[v] = (long)walk.size();
    walk.push_back(v);
    const auto* nx = &succ[v][0];
    while (!alive[nx->first]) ++nx;  // one exists: v kept a live successor
    ords.push_back(nx->second);
    v = nx->first;
  }
  const size_t c0 = (size_t)seen[v];
  *g_entry = idx[walk[c0]];
  for (size_t i = c0 + 1; i < walk.size(); ++i) {
    cyc->push_back((u128)st[walk[i]]);
    cyc_act->push_back(g.action_of(ords[i - 1]));
  }
  *back_action = g.action_of(ords.back());
  return 0;
}

}  // namespace tlcg
