// tests/fuzz/lasso_fuzz.cpp -- the liveness pass's host-side lasso extraction
// (csrc/liveness_graph.h lasso_walk) on seeded explicit graphs, built with
// g++ -fsanitize=address,undefined (tests/test_lasso_fuzz.py).  No GPU: this
// program does the BFS of G' and the Kahn peeling itself, hands lasso_walk the
// states left (through ExplicitGraph's host side, one- and two-word states),
// and verifies the lasso: its entry is among the states left, every step is
// the edge its ordinal names between live not-P states, the states are
// distinct, the walk closes -- and it is the documented one (from the
// shallowest state that still reaches a cycle, the first such successor in
// move order each time).
//
//   lasso_fuzz <graphs> <seed>   ->  one JSON line of counts, exit 0; a
//                                    mismatch prints the graph and exits 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "liveness_graph.h"

using namespace tlcg;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
  bool chance(uint32_t percent) { return below(100) < percent; }
};

struct Csr {
  std::vector<uint32_t> row, col;
  std::vector<unsigned char> p;
  uint32_t n = 0, n_init = 0;
};

Csr draw(Rng& r) {
  Csr g;
  g.n = 1 + r.below(40);
  g.n_init = 1 + r.below(g.n < 3 ? g.n : 3);
  const uint32_t max_deg = 1 + r.below(6), p_pct = r.below(30), back_pct = r.below(101);
  g.row.push_back(0);
  for (uint32_t v = 0; v < g.n; ++v) {
    g.p.push_back(v >= g.n_init && r.chance(p_pct));
    const uint32_t deg = r.below(max_deg + 1);
    for (uint32_t k = 0; k < deg; ++k) {
      uint32_t t = r.below(g.n);
      if (t < v && !r.chance(back_pct)) t = v + r.below(g.n - v);  // fewer back edges: longer tails
      if (k && r.chance(15)) t = g.col.back();                    // a repeated edge
      g.col.push_back(t);
    }
    g.row.push_back((uint32_t)g.col.size());
  }
  return g;
}

struct Counts {
  long graphs = 0, cyclic = 0, acyclic = 0, left_states = 0, dead_states = 0, dead_skipped = 0, steps = 0;
};

[[noreturn]] void fail(const Csr& g, const char* what) {
  std::fprintf(stderr, "lasso_fuzz: %s\n n=%u n_init=%u\n", what, g.n, g.n_init);
  for (uint32_t v = 0; v < g.n; ++v) {
    std::fprintf(stderr, " %u%s:", v, g.p[v] ? "(P)" : "");
    for (uint32_t e = g.row[v]; e < g.row[v + 1]; ++e) std::fprintf(stderr, " %u", g.col[e]);
    std::fprintf(stderr, "\n");
  }
  std::exit(1);
}

template <typename W>
void check(const Csr& c, Counts* cnt) {
  using G = ExplicitGraph<W>;
  G g{};
  std::string err;
  if (!explicit_graph_shape(c.row.data(), c.col.data(), c.n, c.n_init, &g, &err)) fail(c, err.c_str());
  g.row = c.row.data();
  g.col = c.col.data();
  g.p = c.p.data();
  // BFS of G' in store order, then Kahn peeling: the states left
  std::vector<uint32_t> order;
  std::vector<long> index(c.n, -1);
  for (uint32_t v = 0; v < c.n_init; ++v)
    if (!c.p[v]) {
      index[v] = (long)order.size();
      order.push_back(v);
    }
  auto each_move = [&](uint32_t v, auto&& f) {  // (ordinal, successor) of the moves into G'
    for (uint32_t e = c.row[v]; e < c.row[v + 1]; ++e)
      if (c.col[e] != v && !c.p[c.col[e]]) f((int)(e - c.row[v]), c.col[e]);
  };
  for (size_t i = 0; i < order.size(); ++i)
    each_move(order[i], [&](int, uint32_t t) {
      if (index[t] < 0) {
        index[t] = (long)order.size();
        order.push_back(t);
      }
    });
  std::vector<uint32_t> indeg(c.n, 0), q;
  for (uint32_t v : order) each_move(v, [&](int, uint32_t t) { ++indeg[t]; });
  for (uint32_t v : order)
    if (!indeg[v]) q.push_back(v);
  while (!q.empty()) {
    const uint32_t v = q.back();
    q.pop_back();
    each_move(v, [&](int, uint32_t t) {
      if (--indeg[t] == 0) q.push_back(t);
    });
  }
  std::vector<W> st;
  std::vector<uint32_t> idx;
  std::set<uint32_t> live;
  for (size_t i = 0; i < order.size(); ++i)
    if (indeg[order[i]]) {
      st.push_back(G::word_of(order[i]));
      idx.push_back((uint32_t)i);
      live.insert(order[i]);
    }
  if (st.empty()) {
    ++cnt->acyclic;
    return;
  }
  ++cnt->cyclic;
  cnt->left_states += (long)st.size();
  // the states that still reach a cycle: drop, until none is left to drop,
  // every state without a successor in the set
  for (bool again = true; again;) {
    again = false;
    for (auto it = live.begin(); it != live.end();) {
      bool has = false;
      each_move(*it, [&](int, uint32_t t) { has = has || live.count(t); });
      if (has) {
        ++it;
      } else {
        it = live.erase(it);
        again = true;
        ++cnt->dead_states;
      }
    }
  }
  if (live.empty()) fail(c, "states left after peeling but none on a cycle");
  // the documented walk
  uint32_t v = c.n;
  for (size_t i = 0; i < order.size() && v == c.n; ++i)
    if (live.count(order[i])) v = order[i];
  std::vector<uint32_t> walk;
  std::vector<int> ords;
  std::vector<long> seen(c.n, -1);
  while (seen[v] < 0) {
    seen[v] = (long)walk.size();
    walk.push_back(v);
    int ord = -1;
    uint32_t nx = 0;
    each_move(v, [&](int k, uint32_t t) {
      if (ord >= 0) return;
      if (live.count(t)) {
        ord = k;
        nx = t;
      } else if (indeg[t]) {
        ++cnt->dead_skipped;  // left after peeling, but only after the cycles
      }
    });
    ords.push_back(ord);
    v = nx;
  }
  const size_t c0 = (size_t)seen[v];
  u64 g_entry = ~0ull;
  std::vector<u128> cyc;
  std::vector<int> acts;
  int back = -1;
  if (lasso_walk(g, st, idx, &g_entry, &cyc, &acts, &back, &err) != 0) fail(c, err.c_str());
  // the lasso on its own terms
  if (g_entry >= order.size() || !indeg[order[g_entry]]) fail(c, "the entry is not a state left after peeling");
  if (cyc.size() != acts.size()) fail(c, "states and actions differ in number");
  std::vector<uint32_t> loop{order[g_entry]};
  for (u128 w : cyc) {
    const uint32_t t = G::node_of((W)w);
    if (G::word_of(t) != (W)w || t >= c.n) fail(c, "a cycle state is no node's word");
    loop.push_back(t);
  }
  std::set<uint32_t> distinct(loop.begin(), loop.end());
  if (distinct.size() != loop.size()) fail(c, "the cycle repeats a state");
  acts.push_back(back);
  for (size_t i = 0; i < loop.size(); ++i) {
    const uint32_t a = loop[i], b = loop[(i + 1) % loop.size()];
    const int k = acts[i];
    if (c.p[a] || !indeg[a]) fail(c, "a cycle state is in P or was peeled");
    if (k < 0 || c.row[a] + (uint32_t)k >= c.row[a + 1] || c.col[c.row[a] + (uint32_t)k] != b || a == b)
      fail(c, "a step of the cycle is not the edge its ordinal names");
    ++cnt->steps;
  }
  // ... and it is the documented one
  if (order[g_entry] != walk[c0] || loop.size() != walk.size() - c0) fail(c, "not the documented cycle");
  for (size_t i = 0; i < loop.size(); ++i)
    if (loop[i] != walk[c0 + i] || acts[i] != ords[c0 + i]) fail(c, "not the documented cycle");
}

}  // namespace

int main(int argc, char** argv) {
  const long graphs = argc > 1 ? std::atol(argv[1]) : 2000;
  Rng r{argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1};
  Counts cnt;
  for (long i = 0; i < graphs; ++i) {
    const Csr g = draw(r);
    ++cnt.graphs;
    if (i & 1) check<u128>(g, &cnt);
    else check<u64>(g, &cnt);
  }
  std::printf("{\"graphs\": %ld, \"cyclic\": %ld, \"acyclic\": %ld, \"left_states\": %ld, \"dead_states\": %ld, "
              "\"dead_skipped\": %ld, \"steps\": %ld}\n",
              cnt.graphs, cnt.cyclic, cnt.acyclic, cnt.left_states, cnt.dead_states, cnt.dead_skipped, cnt.steps);
  return 0;
}
