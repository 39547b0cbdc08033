// pulsar-tlaplus_amd/csrc/host_model.cpp -- host-only model plumbing and the
// model-level (context-free) C-ABI entry points.
#include "host_model.h"

#include "component_code.h"
#include "component_model.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <unordered_set>

namespace tlcg {

static const char* kPhaseName[6] = {
    "Compactor_In_PhaseOne", "Compactor_In_PhaseTwoWrite", "Compactor_In_PhaseTwoUpdateContext",
    "Compactor_In_PhaseTwoUpdateHorizon", "Compactor_In_PhaseTwoPersistCusror",
    "Compactor_In_PhaseTwoDeleteLedger"};

bool build_model(const tlcg_model& m, HostModel* out, std::string* err) {
  // ASSUME, compaction.tla:25-35 (the booleans are typed by the C struct)
  auto fail = [&](const std::string& s) {
    if (err) *err = s;
    return false;
  };
  if (m.msg_sent_limit < 0) return fail("Assumption MessageSentLimit \\in Nat is false.");
  if (m.compaction_times_limit < 0) return fail("Assumption CompactionTimesLimit \\in Nat is false.");
  if (m.consume_times_limit < 0) return fail("Assumption ConsumeTimesLimit \\in Nat is false.");
  if (m.max_crash_times < 0) return fail("Assumption MaxCrashTimes \\in Nat is false.");
  if (m.n_keys < 0 || m.n_keys > TLCG_MAX_SET || m.n_values < 0 || m.n_values > TLCG_MAX_SET)
    return fail("KeySpace/ValueSpace larger than this build supports (63 elements).");
  std::vector<int64_t> ks(m.keys, m.keys + m.n_keys), vs(m.values, m.values + m.n_values);
  for (int64_t k : ks) {
    if (k < 0) return fail("Assumption KeySpace \\in SUBSET Nat is false.");
    if (k == 0) return fail("Assumption 0 \\notin KeySpace is false.");
  }
  for (int64_t v : vs) {
    if (v < 0) return fail("Assumption ValueSpace \\in SUBSET Nat is false.");
    if (v == 0) return fail("Assumption 0 \\notin ValueSpace is false.");
  }
  if (m.n_invariants < 0 || m.n_invariants > TLCG_MAX_INV) return fail("too many invariants");
  const std::vector<std::string> udefs = user_def_names(m.user_defs);
  for (int q = 0; q < m.n_invariants; ++q) {
    const int kind = m.invariants[q];
    const bool user = kind >= TLCG_INV_USER && kind - TLCG_INV_USER < (int)udefs.size();
    if (!user && (kind < 0 || kind >= N_INVARIANT_KINDS)) return fail("unknown invariant id");
  }
  HostModel hm;
  ks.push_back(0);
  vs.push_back(0);
  std::sort(ks.begin(), ks.end());
  ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
  std::sort(vs.begin(), vs.end());
  vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
  hm.keyset = ks;
  hm.valueset = vs;
  Layout& L = hm.L;
  std::memset(&L, 0, sizeof L);
  L.N = m.msg_sent_limit;
  L.C = m.compaction_times_limit;
  L.K = m.max_crash_times;
  L.ctl = m.consume_times_limit;
  if (L.N > 32) return fail("MessageSentLimit > 32 is not supported by this build.");
  if (L.C > 32) return fail("CompactionTimesLimit > 32 is not supported by this build.");
  L.nk = (int)ks.size();
  L.nv = (int)vs.size();
  L.nkv = L.nk * L.nv;
  L.kb = bits_for((u64)(L.nk - 1));
  L.vb = bits_for((u64)(L.nv - 1));
  L.mw = L.kb + L.vb;
  int sh = 0;
  L.len_sh = sh; L.len_w = bits_for((u64)L.N); sh += L.len_w;
  L.msg_sh = sh; sh += L.N * L.mw;
  L.led_sh = sh; L.led_w = 1 + L.N; sh += L.C * L.led_w;
  L.p1r_sh = sh; L.p1r_w = bits_for((u64)L.N); sh += L.p1r_w;
  L.cur_sh = sh; L.curh_w = bits_for((u64)L.N); L.curc_w = bits_for((u64)L.C); sh += 1 + L.curh_w + L.curc_w;
  L.ph_sh = sh; sh += 3;
  L.hz_sh = sh; L.hz_w = bits_for((u64)L.N); sh += L.hz_w;
  L.ctx_sh = sh; L.ctx_w = bits_for((u64)L.C); sh += L.ctx_w;
  L.cr_sh = sh; L.cr_w = bits_for((u64)L.K); sh += L.cr_w;
  L.bits = sh;
  if (L.bits > 126) {
    char b[160];
    std::snprintf(b, sizeof b, "these constants need a %d-bit state; this build packs states into 126 bits", L.bits);
    return fail(b);
  }
  L.retain = m.retain_null_key ? 1 : 0;
  L.producer = m.model_producer ? 1 : 0;
  L.consumer = m.model_consumer ? 1 : 0;
  // Terminating's last conjunct: ModelConsumer => consumeTimes = ConsumeTimesLimit,
  // with consumeTimes constantly 0.
  L.term_ok = (!L.consumer || L.ctl == 0) ? 1 : 0;
  L.check_deadlock = m.check_deadlock ? 1 : 0;
  L.ord_bits = bits_for((u64)(L.nkv + N_ACTIONS - 1));
  L.n_inv = m.n_invariants;
  for (int q = 0; q < m.n_invariants; ++q) L.inv[q] = m.invariants[q];
  const u128 mm = wmask<u128>(L.msg_sh + L.N * L.mw);
  L.msgs_mask = (u64)mm;
  L.msgs_mask_hi = (u64)(mm >> 64);
  u128 pm = 0;
  for (int j = 1; j <= L.C; ++j) pm |= (u128)1 << led_base(L, j);
  L.led_present_mask = (u64)pm;
  L.led_present_mask_hi = (u64)(pm >> 64);
  // initial states
  if (L.producer) {
    hm.n_init = 1;
  } else {
    long double n = 1;
    for (int i = 0; i < L.N; ++i) n *= (long double)L.nkv;
    if (n > (long double)(1ull << 40)) return fail("more than 2^40 initial states");
    u64 c = 1;
    for (int i = 0; i < L.N; ++i) c *= (u64)L.nkv;
    hm.n_init = c;
  }
  hm.max_new_per_state = (L.producer ? L.nkv : 0) + 2;
  // user invariants (user_inv.h): the distinct definitions the cfg names, in
  // first-use order, become program entries 0, 1, ..; L.inv holds INV_USER + entry
  std::vector<std::string> names;
  for (int q = 0; q < m.n_invariants; ++q) {
    if (m.invariants[q] < TLCG_INV_USER) continue;
    const std::string& nm = udefs[(size_t)(m.invariants[q] - TLCG_INV_USER)];
    size_t k = std::find(names.begin(), names.end(), nm) - names.begin();
    if (k == names.size()) names.push_back(nm);
    L.inv[q] = INV_USER + (int)k;
  }
  hm.constraints = user_constraint_names(m.user_defs);
  if (!names.empty() || !hm.constraints.empty()) {
    auto prog = std::make_shared<UserProg>();
    std::string e;
    if (!compile_user_invariants(m, hm, names, prog.get(), &e, hm.constraints)) return fail(e);
    hm.user = prog;
    hm.user_defs = m.user_defs;
    L.defer_inv = names.empty() ? 0 : 1;
  }
  *out = hm;
  return true;
}

namespace {
// the insert calls of component `comp`'s BFS (the closure of initial state
// comp), in the kernels' order: per depth, chunks of `group` states; per
// chunk the compactor successors, then BrokerCrash's (`pair`: a depth of at
// most group / 2 states in one call, the tree's pair mode); and its codes in
// BFS order.  False when the component does not fit T slots.
bool comp_calls(const HostModel& hm, int T, int group, u64 comp, bool pair, std::vector<std::vector<uint32_t>>* calls,
                std::vector<uint32_t>* codes) {
  const Layout& L = hm.L;
  const u128 s0 = init_state<u128>(L, comp);
  const CompMsgs cm = comp_msgs_init(L, (u64)s0);
  const CodeConsts kc = code_consts(L, cm);
  *calls = {{code_encode_w<u128>(L, s0)}};
  *codes = {(*calls)[0][0]};
  std::unordered_set<uint32_t> seen{(*calls)[0][0]};
  std::vector<uint32_t> level{(*calls)[0][0]};
  while (!level.empty() && seen.size() < (size_t)T) {
    std::vector<uint32_t> next;
    for (size_t b = 0; b < level.size(); b += (size_t)group) {
      std::vector<uint32_t> c1, c2;
      for (size_t i = b; i < b + (size_t)group && i < level.size(); ++i) {
        ckey t = 0, t2 = 0;
        int act = 0;
        if (compactor_step_cb(L, kc, level[i], &t, &act) == 1) c1.push_back(t);
        if (crash_step_c(L, level[i], &t2)) c2.push_back(t2);
      }
      if (pair && level.size() <= (size_t)group / 2) {
        c1.insert(c1.end(), c2.begin(), c2.end());
        c2.clear();
      }
      for (auto* c : {&c1, &c2}) {
        if (c->empty()) continue;
        calls->push_back(*c);
        for (uint32_t k : *c)
          if (seen.insert(k).second) {
            next.push_back(k);
            codes->push_back(k);
          }
      }
    }
    level.swap(next);
  }
  return seen.size() < (size_t)T;
}
bool comp0_calls(const HostModel& hm, int T, int group, std::vector<std::vector<uint32_t>>* calls,
                 std::vector<uint32_t>* codes) {
  return comp_calls(hm, T, group, 0, false, calls, codes);
}
// the probe trips of a group's longest lane, summed over the insert calls, on
// a T-slot table probed linearly from the multiply-shift slot of `mult` plus
// disp[(code * dmult) >> 24] (the tree kernel's insert, tree_body.h)
long sim_trips(const std::vector<std::vector<uint32_t>>& calls, int T, uint32_t mult, uint32_t dmult,
               const uint16_t* disp) {
  std::vector<uint32_t> h((size_t)T, 0);
  long total = 0;
  for (const auto& c : calls) {
    int longest = 0;
    for (uint32_t key : c) {
      unsigned sl = (unsigned)(((unsigned long long)(key * mult) * (unsigned)T) >> 32);
      if (disp) {
        sl += disp[(key * dmult) >> 24];
        sl = sl >= (unsigned)T ? sl - (unsigned)T : sl;
      }
      int p = 1;
      for (; p <= T; ++p) {
        if (h[sl] == 0) {
          h[sl] = key + 1;
          break;
        }
        if (h[sl] == key + 1) break;
        sl = sl + 1 == (unsigned)T ? 0 : sl + 1;
      }
      longest = std::max(longest, p);
    }
    total += longest;
  }
  return total;
}
}  // namespace

uint32_t tune_slot_mult(const HostModel& hm, int T, int group, int candidates) {
  const Layout& L = hm.L;
  const uint32_t def = 0x9E3779B1u;
  if (L.producer || T <= 0 || group <= 0) return def;
  std::vector<std::vector<uint32_t>> calls;
  std::vector<uint32_t> codes;
  if (!comp0_calls(hm, T, group, &calls, &codes)) return def;  // does not fit the table: nothing to tune
  auto trips = [&](uint32_t mult) {
    std::vector<uint32_t> h((size_t)T, 0);
    long total = 0;
    for (const auto& c : calls) {
      int longest = 0;
      for (uint32_t key : c) {
        unsigned sl = (unsigned)(((unsigned long long)(key * mult) * (unsigned)T) >> 32);
        int p = 1;
        for (; p <= T; ++p) {
          if (h[sl] == 0) {
            h[sl] = key + 1;
            break;
          }
          if (h[sl] == key + 1) break;
          sl = sl + 1 == (unsigned)T ? 0 : sl + 1;
        }
        longest = std::max(longest, p);
      }
      total += longest;
    }
    return total;
  };
  uint32_t best = def;
  long best_t = trips(def);
  uint64_t x = 0x2545F4914F6CDD1Dull;  // a fixed sequence: the choice is deterministic
  for (int i = 0; i < candidates; ++i) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    const uint32_t m = (uint32_t)(x >> 16) | 1u;
    const long t = trips(m);
    if (t < best_t) {
      best_t = t;
      best = m;
    }
  }
  return best;
}

bool build_slot_disp(const HostModel& hm, int T, uint32_t mult, uint32_t* dmult, uint16_t* disp) {
  constexpr int NB = 256;
  std::fill(disp, disp + NB, (uint16_t)0);
  *dmult = 0x85EBCA6Bu;
  if (hm.L.producer || T <= 0 || T > 65535) return false;
  std::vector<std::vector<uint32_t>> calls;
  std::vector<uint32_t> codes;
  if (!comp0_calls(hm, T, 16, &calls, &codes)) return false;
  auto base = [&](uint32_t k) { return (unsigned)(((unsigned long long)(k * mult) * (unsigned)T) >> 32); };
  uint64_t x = 0x2545F4914F6CDD1Dull;  // a fixed sequence: the choice is deterministic
  for (int attempt = 0; attempt < 64; ++attempt) {
    const uint32_t dm = attempt == 0 ? *dmult : (uint32_t)((x ^= x << 13, x ^= x >> 7, x ^= x << 17) >> 16) | 1u;
    std::vector<std::vector<uint32_t>> bucket(NB);
    for (uint32_t k : codes) bucket[(k * dm) >> 24].push_back(k);
    std::vector<int> order(NB);
    for (int b = 0; b < NB; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return bucket[p].size() > bucket[q].size(); });
    std::vector<char> used((size_t)T, 0);
    uint16_t d[NB] = {};
    bool ok = true;
    for (int b : order) {
      if (bucket[b].empty()) break;
      int found = -1;
      for (int dv = 0; dv < T && found < 0; ++dv) {
        bool fits = true;
        for (size_t i = 0; i < bucket[b].size() && fits; ++i) {
          const unsigned s = (base(bucket[b][i]) + (unsigned)dv) % (unsigned)T;
          fits = !used[s];
          for (size_t j = 0; j < i && fits; ++j) fits = (base(bucket[b][j]) + (unsigned)dv) % (unsigned)T != s;
        }
        if (fits) found = dv;
      }
      if (found < 0) {
        ok = false;
        break;
      }
      d[b] = (uint16_t)found;
      for (uint32_t k : bucket[b]) used[(base(k) + (unsigned)found) % (unsigned)T] = 1;
    }
    if (ok) {
      *dmult = dm;
      std::copy(d, d + NB, disp);
      return true;
    }
  }
  return false;
}

bool build_slot_owner(const HostModel& hm, int T, uint32_t mult, uint32_t dmult, const uint16_t* disp,
                      uint32_t* owner) {
  std::fill(owner, owner + T, 0u);
  if (hm.L.producer || T <= 0) return false;
  std::vector<std::vector<uint32_t>> calls;
  std::vector<uint32_t> codes;
  if (!comp0_calls(hm, T, 16, &calls, &codes)) return false;
  for (uint32_t k : codes) {
    unsigned sl = (unsigned)(((unsigned long long)(k * mult) * (unsigned)T) >> 32);  // (tree_body.h's slot)
    sl += disp[(k * dmult) >> 24];
    sl = sl >= (unsigned)T ? sl - (unsigned)T : sl;
    if (owner[sl]) {
      std::fill(owner, owner + T, 0u);
      return false;
    }
    owner[sl] = k + 1u;
  }
  return true;
}

bool build_lane_phash(const HostModel& hm, uint32_t* mult, uint32_t* owner, std::string* why) {
  std::fill(owner, owner + 2 * LANE_T, 0u);
  *mult = 0;
  const Layout& L = hm.L;
  if (L.producer || code_bits(L) > 16) return false;
  std::vector<std::vector<uint32_t>> calls;
  std::vector<uint32_t> codes;
  if (!comp0_calls(hm, 63, 1, &calls, &codes)) return false;  // (>= 63 states: past the pass's K = 64 - 2)
  // an owner entry is two words (component_code.h lane_owner_word): code + 1,
  // the code's invariant features, which the kernel ands with each
  // component's mask, and its step-table index in the first, its dense index
  // in S (the position in `codes`) in the second.  The pass is taken only if
  // every field fits, and the features only if they are
  // check_invariants_cb's answer on every code of S, under the constants of
  // the first components (tlcg_host_lane_inv_selfcheck: every code and class)
  if (codes.size() > 62) return false;  // (a dense index is a bit of a 64-bit register)
  for (uint32_t c : codes) {
    if (lane_owner_word(L, c) == 0u) return false;
    for (u64 idx = 0; idx < 16 && idx < hm.n_init && !hm.user; ++idx) {
      const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)init_state<u128>(L, idx)));
      if (((lane_inv_feat(L, c) & lane_inv_mask(L, kc)) != 0) != (check_invariants_cb(L, kc, c) != -1)) {
        if (why)
          *why = "the per-lane pass is not taken: the invariant features of code " + std::to_string(c) +
                 " disagree with check_invariants_cb on component " + std::to_string(idx);
        return false;
      }
    }
  }
  std::vector<uint32_t> used(2 * LANE_T, 0);
  uint64_t x = 0x2545F4914F6CDD1Dull;  // a fixed sequence: the choice is deterministic
  for (int i = 0; i < (1 << 20); ++i) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    const uint32_t m = ((uint32_t)(x >> 20) & 0xFFFFFFu) | 1u;
    std::fill(used.begin(), used.end(), 0u);
    bool ok = true;
    for (size_t i = 0; i < codes.size(); ++i) {
      const unsigned sl = lane_slot(codes[i], m);
      if (used[2 * sl]) {
        ok = false;
        break;
      }
      used[2 * sl] = lane_owner_word(L, codes[i]);
      used[2 * sl + 1] = (uint32_t)i;
    }
    if (ok) {
      *mult = m;
      std::copy(used.begin(), used.end(), owner);
      return true;
    }
  }
  return false;
}

int lane_ring_entries(const Layout& L) {
  if (L.producer || code_bits(L) > 16 || L.C > 3) return 16;
  // component 0's FIFO BFS in the kernel's order (compactor successor, then
  // BrokerCrash's, each appended when new); the widest queue after an expansion
  const u128 s0 = init_state<u128>(L, 0);
  const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)s0));
  std::vector<uint32_t> q{code_encode_w<u128>(L, s0)};
  std::unordered_set<uint32_t> seen{q[0]};
  size_t width = 0;
  for (size_t head = 0; head < q.size(); ++head) {
    if (q.size() >= 63) return 16;  // (past the pass's capacity: the cascade runs it)
    ckey t = 0, t2 = 0;
    int act = 0;
    if (compactor_step_cb(L, kc, q[head], &t, &act) == 1 && seen.insert(t).second) q.push_back(t);
    if (crash_step_c(L, q[head], &t2) && seen.insert(t2).second) q.push_back(t2);
    width = std::max(width, q.size() - (head + 1));
  }
  return width + 2 <= 8 ? 8 : 16;
}

template <typename W>
std::string format_state(const HostModel& hm, W s) {
  const Layout& L = hm.L;
  std::ostringstream o;
  int len = st_len(L, s);
  auto msg = [&](int p) {
    o << "[id |-> " << p << ", key |-> " << hm.keyset[st_key(L, s, p)] << ", value |-> "
      << hm.valueset[st_val(L, s, p)] << "]";
  };
  o << "/\\ messages = <<";
  for (int p = 1; p <= len; ++p) {
    if (p > 1) o << ", ";
    msg(p);
  }
  o << ">>\n/\\ compactedLedgers = <<";
  for (int j = 1; j <= L.C; ++j) {
    if (j > 1) o << ", ";
    if (!led_present(L, s, j)) {
      o << "Nil";
      continue;
    }
    u64 mk = led_mask(L, s, j);
    o << "<<";
    bool first = true;
    for (int p = 1; p <= L.N; ++p)
      if ((mk >> (p - 1)) & 1) {
        if (!first) o << ", ";
        msg(p);
        first = false;
      }
    o << ">>";
  }
  o << ">>\n/\\ cursor = ";
  if (!cur_present(L, s)) o << "Nil";
  else o << "[compactedTopicContext |-> " << cur_c(L, s) << ", compactionHorizon |-> " << cur_h(L, s) << "]";
  o << "\n/\\ compactorState = " << kPhaseName[st_phase(L, s) < 6 ? st_phase(L, s) : 0];
  o << "\n/\\ phaseOneResult = ";
  int r = st_p1r(L, s);
  if (r == 0) {
    o << "Nil";
  } else {
    // latestForKey == [key \in GetKeys(messages[1..r]) |-> Max(...)] (compaction.tla:97-98)
    std::vector<std::pair<int64_t, int>> f;
    for (int ki = 1; ki < L.nk; ++ki) {
      int mx = 0;
      for (int p = 1; p <= r; ++p)
        if (st_key(L, s, p) == ki) mx = p;
      if (mx) f.push_back({hm.keyset[ki], mx});
    }
    bool tuple = true;
    for (size_t i = 0; i < f.size(); ++i)
      if (f[i].first != (int64_t)(i + 1)) tuple = false;
    o << "[latestForKey |-> ";
    if (tuple) {
      o << "<<";
      for (size_t i = 0; i < f.size(); ++i) o << (i ? ", " : "") << f[i].second;
      o << ">>";
    } else {
      o << "(";
      for (size_t i = 0; i < f.size(); ++i) o << (i ? " @@ " : "") << f[i].first << " :> " << f[i].second;
      o << ")";
    }
    o << ", readPosition |-> " << r << "]";
  }
  o << "\n/\\ compactionHorizon = " << st_hz(L, s);
  o << "\n/\\ compactedTopicContext = " << st_ctx(L, s);
  o << "\n/\\ crashTimes = " << st_crash(L, s);
  o << "\n/\\ consumeTimes = 0";
  return o.str();
}

template <typename W>
int successor_at(const Layout& L, W s, int ord, W* t) {
  int act = action_of_ordinal(L, ord);
  if (act == ACT_PRODUCER) {
    if (!L.producer) return 0;
    int len = st_len(L, s);
    if (len >= L.N) return 0;
    *t = producer_succ(L, s, len, ord);
    return 1;
  }
  if (act == ACT_CRASH) return crash_step(L, s, t);
  if (act == ACT_CONSUMER) {
    if (!L.consumer) return 0;
    *t = s;
    return 1;
  }
  if (act == ACT_TERMINATING) {
    if (!terminating_enabled(L, s)) return 0;
    *t = s;
    return 1;
  }
  int a2 = -1;
  W u = 0;
  int r = compactor_step(L, s, &u, &a2);
  if (r == 0 || a2 != act) return 0;
  if (r == 2) return 2;
  *t = u;
  return 1;
}

template <typename W>
int host_successors(const Layout& L, W s, W* out, int* actions, int cap) {
  int n = 0;
  auto put = [&](W t, int a) {
    if (n < cap) {
      out[n] = t;
      if (actions) actions[n] = a;
    }
    ++n;
  };
  if (L.producer) {
    int len = st_len(L, s);
    if (len < L.N)
      for (int j = 0; j < L.nkv; ++j) put(producer_succ(L, s, len, j), ACT_PRODUCER);
  }
  W t;
  int act;
  int r = compactor_step(L, s, &t, &act);
  if (r == 2) return -1;
  if (r == 1) put(t, act);
  if (crash_step(L, s, &t)) put(t, ACT_CRASH);
  if (L.consumer) put(s, ACT_CONSUMER);
  if (terminating_enabled(L, s)) put(s, ACT_TERMINATING);
  return n;
}

template std::string format_state<u64>(const HostModel&, u64);
template std::string format_state<u128>(const HostModel&, u128);
template int successor_at<u64>(const Layout&, u64, int, u64*);
template int successor_at<u128>(const Layout&, u128, int, u128*);
template int host_successors<u64>(const Layout&, u64, u64*, int*, int);
template int host_successors<u128>(const Layout&, u128, u128*, int*, int);

}  // namespace tlcg

using namespace tlcg;

namespace {

// the user invariants' views of one reachable state: a component code's
// (component_code.h UVCode, the on-chip engines' form) against the word's
// (model.h UVWord): every field the programs read, and each user invariant
template <typename W>
bool user_views_agree(const HostModel& hm, const CodeConsts& kc, W w) {
  const Layout& L = hm.L;
  const ckey cd = code_encode_w<W>(L, w);
  const UVWord<W> a{L, w};
  const UVCode<W> b{L, kc, cd};
  if (b.word() != w) return false;
  bool ok = a.len() == b.len() && a.phase() == b.phase() && a.p1r() == b.p1r() && a.hz() == b.hz() &&
            a.ctx() == b.ctx() && a.crash() == b.crash() && a.curp() == b.curp() && a.curh() == b.curh() &&
            a.curc() == b.curc();
  for (int i = 1; i <= L.N; ++i) ok = ok && a.key(i) == b.key(i) && a.val(i) == b.val(i);
  for (int j = 1; j <= L.C; ++j) ok = ok && a.ledp(j) == b.ledp(j) && a.ledm(j) == b.ledm(j);
  for (int k = 0; k < hm.user->n_user && ok; ++k) ok = eval_user_v(*hm.user, k, a) == eval_user_v(*hm.user, k, b);
  return ok;
}

// user invariants: the views on every reachable state of components
// [first, first + n) (no Producer).  Returns the states checked, or
// -(1 + checked) at the first disagreement.
int64_t user_view_selfcheck(const HostModel& hm, u64 first, u64 n) {
  const Layout& L = hm.L;
  int64_t checked = 0;
  if (L.N > 8 || code_bits(L) > 31) return 0;  // no on-chip engine takes the model
  const bool wide = state_words(L) == 2;
  for (u64 idx = first; idx < first + n && idx < hm.n_init; ++idx) {
    const u128 s0 = wide ? init_state<u128>(L, idx) : (u128)init_state<u64>(L, idx);
    const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)s0));
    std::vector<u128> todo{s0};
    std::unordered_set<u64> seen{mix64((u64)s0) ^ (u64)(s0 >> 64)};
    while (!todo.empty()) {
      const u128 w = todo.back();
      todo.pop_back();
      if (!(wide ? user_views_agree<u128>(hm, kc, w) : user_views_agree<u64>(hm, kc, (u64)w))) return -(1 + checked);
      ++checked;
      u128 succ[64];
      int ns;
      if (wide) {
        ns = host_successors<u128>(L, w, succ, nullptr, 64);
      } else {
        u64 s1[64];
        ns = host_successors<u64>(L, (u64)w, s1, nullptr, 64);
        for (int i = 0; i < ns && i < 64; ++i) succ[i] = s1[i];
      }
      for (int i = 0; i < ns && i < 64; ++i)
        if (seen.insert(mix64((u64)succ[i]) ^ (u64)(succ[i] >> 64)).second) todo.push_back(succ[i]);
    }
  }
  return checked;
}

}  // namespace

extern "C" {

int tlcg_abi_version(void) { return TLCG_ABI_VERSION; }

int tlcg_check_model(const tlcg_model* m, char* err, int32_t cap) {
  HostModel hm;
  std::string e;
  if (!m) return -1;
  if (!build_model(*m, &hm, &e)) {
    if (err && cap > 0) std::snprintf(err, (size_t)cap, "%s", e.c_str());
    return -1;
  }
  if (err && cap > 0) err[0] = 0;
  return 0;
}

int tlcg_state_bits(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  return hm.L.bits;
}

uint64_t tlcg_init_count(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return 0;
  return hm.n_init;
}

int tlcg_ordinal_bits(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  return hm.L.ord_bits;
}

int tlcg_action_of_ordinal(const tlcg_model* m, int32_t ordinal) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -2;
  return action_of_ordinal(hm.L, ordinal);
}

int tlcg_state_words(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  return state_words(hm.L);
}

int tlcg_decode_words(const tlcg_model* m, const uint64_t* state, char* buf, int32_t cap) {
  HostModel hm;
  std::string e;
  if (!m || !state || !build_model(*m, &hm, &e)) return -1;
  const int w = state_words(hm.L);
  std::string s = w == 1 ? format_state<u64>(hm, state[0]) : format_state<u128>(hm, join_words(state, 2));
  if (buf && cap > 0) std::snprintf(buf, (size_t)cap, "%s", s.c_str());
  return (int)s.size();
}

int tlcg_decode(const tlcg_model* m, uint64_t state, char* buf, int32_t cap) {
  if (tlcg_state_words(m) != 1) return -2;  // wide layout: tlcg_decode_words
  return tlcg_decode_words(m, &state, buf, cap);
}

int tlcg_host_init_state_words(const tlcg_model* m, uint64_t idx, uint64_t* out) {
  HostModel hm;
  std::string e;
  if (!m || !out || !build_model(*m, &hm, &e)) return -1;
  split_words(init_state<u128>(hm.L, idx), out, state_words(hm.L));
  return 0;
}

uint64_t tlcg_host_init_state(const tlcg_model* m, uint64_t idx) {
  uint64_t w[2] = {~0ull, ~0ull};
  if (tlcg_state_words(m) != 1 || tlcg_host_init_state_words(m, idx, w)) return ~0ull;
  return w[0];
}

int tlcg_host_successors_words(const tlcg_model* m, const uint64_t* state, uint64_t* out, int32_t* actions,
                               int32_t cap) {
  HostModel hm;
  std::string e;
  if (!m || !state || !build_model(*m, &hm, &e)) return -2;
  const int w = state_words(hm.L);
  const int k = std::max(cap, 0);
  std::vector<u128> succ((size_t)k);
  std::vector<int> acts((size_t)k);
  // the u128 instantiation computes the same successors as the u64 one for any layout
  const int n = host_successors<u128>(hm.L, join_words(state, w), succ.data(), acts.data(), cap);
  for (int i = 0; i < std::min(n, (int)cap); ++i) {
    if (out) split_words(succ[(size_t)i], out + (size_t)i * w, w);
    if (actions) actions[i] = acts[(size_t)i];
  }
  return n;
}

int tlcg_host_successors(const tlcg_model* m, uint64_t state, uint64_t* out, int32_t* actions, int32_t cap) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e) || state_words(hm.L) != 1) return -2;
  std::vector<int> acts((size_t)std::max(cap, 0));
  int n = host_successors<u64>(hm.L, state, out, acts.data(), cap);
  if (actions)
    for (int i = 0; i < std::min(n, (int)cap); ++i) actions[i] = acts[(size_t)i];
  return n;
}

int tlcg_host_check_invariants_words(const tlcg_model* m, const uint64_t* state) {
  HostModel hm;
  std::string e;
  if (!m || !state || !build_model(*m, &hm, &e)) return -2;
  return host_check_all<u128>(hm, join_words(state, state_words(hm.L)));
}

int tlcg_host_check_invariants_batch(const tlcg_model* m, const uint64_t* states, uint64_t n, int32_t* out) {
  HostModel hm;
  std::string e;
  if (!m || !states || !out || !build_model(*m, &hm, &e)) return -2;
  const int w = state_words(hm.L);
  for (uint64_t i = 0; i < n; ++i) out[i] = host_check_all<u128>(hm, join_words(states + i * (uint64_t)w, w));
  return 0;
}

int tlcg_host_constraint_eval(const tlcg_model* m, const uint64_t* states, uint64_t n, uint8_t* out, char* err,
                              int32_t errlen) {
  auto fail = [&](int rc, const std::string& e) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", e.c_str());
    return rc;
  };
  HostModel hm;
  std::string e;
  if (!m || !states || !out) return fail(-1, "null argument");
  if (!build_model(*m, &hm, &e)) return fail(-2, e);
  const int w = state_words(hm.L);
  for (uint64_t i = 0; i < n; ++i) {
    int which = 0;
    out[i] = hm.constraints.empty()
                 ? (uint8_t)EV_TRUE
                 : (uint8_t)eval_constraints_v(*hm.user, UVWord<u128>{hm.L, join_words(states + i * (uint64_t)w, w)},
                                               &which);
  }
  if (err && errlen > 0) err[0] = 0;
  return 0;
}

int tlcg_host_property_form(const tlcg_model* m, const char* name, int32_t* form, char* err, int32_t cap) {
  auto fail = [&](int rc, const std::string& e) {
    if (err && cap > 0) std::snprintf(err, (size_t)cap, "%s", e.c_str());
    return rc;
  };
  HostModel hm;
  std::string e;
  if (!m || !name || !form) return fail(-3, "null argument");
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  int f = 0;
  const int rc = compile_property(*m, hm, name, &f, nullptr, &e);
  if (rc) return fail(rc, e);
  *form = f;
  if (err && cap > 0) err[0] = 0;
  return 0;
}

int tlcg_host_property_eval(const tlcg_model* m, const char* name, const uint64_t* states, uint64_t n, uint8_t* out) {
  HostModel hm;
  std::string e;
  if (!m || !name || (n && (!states || !out)) || !build_model(*m, &hm, &e)) return -3;
  const std::unique_ptr<UserProg> prog(new UserProg);
  int f = 0;
  const int rc = compile_property(*m, hm, name, &f, prog.get(), &e);
  if (rc) return rc;
  const int w = state_words(hm.L);
  for (uint64_t i = 0; i < n; ++i) {
    const u128 s = join_words(states + i * (uint64_t)w, w);
    const int p = eval_user<u128>(hm.L, *prog, 0, s), q = eval_user<u128>(hm.L, *prog, 1, s);
    out[i] = (uint8_t)((p == EV_TRUE ? 1 : 0) | (q == EV_TRUE ? 2 : 0) | (p == EV_ERROR || q == EV_ERROR ? 4 : 0));
  }
  return 0;
}

int tlcg_host_action_property_form(const tlcg_model* m, const char* name, uint32_t* var_mask, char* err,
                                   int32_t cap) {
  auto fail = [&](int rc, const std::string& e) {
    if (err && cap > 0) std::snprintf(err, (size_t)cap, "%s", e.c_str());
    return rc;
  };
  HostModel hm;
  std::string e;
  if (!m || !name) return fail(-3, "null argument");
  if (!build_model(*m, &hm, &e)) return fail(-3, e);
  uint32_t mask = 0;
  const int rc = compile_action_property(*m, hm, name, &mask, nullptr, &e);
  if (rc) return fail(rc, e);
  if (var_mask) *var_mask = mask;
  if (err && cap > 0) err[0] = 0;
  return 0;
}

int tlcg_host_action_property_eval(const tlcg_model* m, const char* name, const uint64_t* pairs, uint64_t n,
                                   uint8_t* out) {
  HostModel hm;
  std::string e;
  if (!m || !name || (n && (!pairs || !out)) || !build_model(*m, &hm, &e)) return -3;
  const std::unique_ptr<UserProg> prog(new UserProg);
  const int rc = compile_action_property(*m, hm, name, nullptr, prog.get(), &e);
  if (rc) return rc;
  const int w = state_words(hm.L);
  for (uint64_t i = 0; i < n; ++i) {
    const u128 s = join_words(pairs + 2 * i * (uint64_t)w, w), t = join_words(pairs + (2 * i + 1) * (uint64_t)w, w);
    out[i] = (uint8_t)eval_user2<u128>(hm.L, *prog, 0, s, t);
  }
  return 0;
}

int tlcg_host_check_invariants(const tlcg_model* m, uint64_t state) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e) || state_words(hm.L) != 1) return -2;
  return host_check_all(hm, state);
}

// PROPERTY Termination == <>(Len(messages) = MessageSentLimit /\
// compactorState = Compactor_In_PhaseTwoWrite /\ MaxCompactedLedgerId = ... /\
// (ModelConsumer => ...)), compaction.tla:303-307: its body is the guard of
// Terminating (:205-213), terminating_enabled.  Spec == Init /\ [][Next]_vars
// (:233) has no fairness, so every behavior may stutter forever in its initial
// state: <>P is violated iff some initial state has ~P, and the behavior
// "that state, then stuttering" is a counterexample.  Returns the first such
// initial state in TLC's Init order, or -1 when every initial state satisfies P.
int64_t tlcg_host_termination_counterexample(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -2;
  for (u64 i = 0; i < hm.n_init; ++i)
    if (!terminating_enabled(hm.L, init_state<u128>(hm.L, i))) return (int64_t)i;
  return -1;
}

// Component-specialized evaluators (component_model.h) vs the generic ones
// (model.h) on every state of the components of initial states
// [first, first + n): the compactor successor, the stutter count and the
// first failing invariant must agree.  The same for component codes
// (component_code.h): every reachable local key must encode and decode back
// to itself (the two-valued fields the code relies on), and the code
// evaluators must decode to the same successors and results.  Returns the states compared, or
// -(1 + index of the first disagreeing state) on a mismatch.
// The tree's closed-mode FPSet on component `comp`, replayed on the host
// with the engine's tuned multiplier and displacement table (built from
// component 0): out[0] = insert calls (16-lane groups, pair mode), out[1] =
// probe trips of each call's longest lane with the table, out[2] = without
// it.  0; -1 when the closed tree does not take the component (Producer
// modelled, or more than 640 states); -2 on a bad model.
int tlcg_host_tree_slot_probes(const tlcg_model* m, uint64_t comp, int64_t* out) {
  HostModel hm;
  std::string e;
  if (!m || !out || !build_model(*m, &hm, &e)) return -2;
  if (hm.L.producer || comp >= hm.n_init) return -1;
  constexpr int T = 640;  // (the closed tree's first pass, tlcgpu.hip)
  std::vector<std::vector<uint32_t>> calls;
  std::vector<uint32_t> codes;
  if (!comp_calls(hm, T, 16, comp, true, &calls, &codes)) return -1;
  const uint32_t mult = tune_slot_mult(hm, T, 16, 4096);
  uint32_t dmult = 0;
  uint16_t disp[256];  // (TREE_DISP buckets, tree.h)
  build_slot_disp(hm, T, mult, &dmult, disp);
  out[0] = (int64_t)calls.size();
  out[1] = sim_trips(calls, T, mult, dmult, disp);
  out[2] = sim_trips(calls, T, mult, 0, nullptr);
  return 0;
}

int64_t tlcg_host_component_selfcheck(const tlcg_model* m, uint64_t first, uint64_t n) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e) || hm.L.producer) return -1;
  if (hm.user) return user_view_selfcheck(hm, first, n);
  const Layout& L = hm.L;
  int64_t checked = 0;
  const int mb = L.led_sh;
  if (L.N > 8) return 0;  // the component engines do not take this model
  if (L.bits - mb > 32) {
    // wide local keys: only component codes (the component tree's closed
    // mode), on whole u128 words against model.h
    if (code_bits(L) > 31) return 0;
    for (u64 idx = first; idx < first + n && idx < hm.n_init; ++idx) {
      const u128 s0 = init_state<u128>(L, idx);
      const u128 msgs = s0 & messages_mask<u128>(L);
      const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)s0));
      std::vector<u128> todo{s0};
      std::unordered_set<u64> seen{mix64((u64)s0) ^ (u64)(s0 >> 64)};
      std::vector<u128> all{s0};
      while (!todo.empty()) {
        const u128 w = todo.back();
        todo.pop_back();
        const ckey cd = code_encode_w<u128>(L, w);
        if (code_word<u128>(L, kc, msgs, cd) != w) return -(1 + checked);
        u128 t1 = 0, t2 = 0;
        ckey ct = 0, cx = 0;
        int a1 = -1, a2 = -1;
        const int r1 = compactor_step<u128>(L, w, &t1, &a1);
        const int r2 = compactor_step_cb(L, kc, cd, &ct, &a2);
        const int x1 = crash_step<u128>(L, w, &t2), x2 = crash_step_c(L, cd, &cx);
        if (r1 != r2 || a1 != a2 || (r1 == 1 && code_word<u128>(L, kc, msgs, ct) != t1) || x1 != x2 ||
            (x1 && code_word<u128>(L, kc, msgs, cx) != t2) ||
            check_invariants<u128>(L, w) != check_invariants_cb(L, kc, cd) ||
            selfloop_count<u128>(L, w) != selfloop_count_c(L, kc, cd))
          return -(1 + checked);
        ++checked;
        u128 succ[64];
        const int ns = host_successors<u128>(L, w, succ, nullptr, 64);
        for (int i = 0; i < ns && i < 64; ++i) {
          // (a set of 64-bit digests of the 128-bit states: exact enough here,
          // a collision only skips a state of the check)
          if (seen.insert(mix64((u64)succ[i]) ^ (u64)(succ[i] >> 64)).second) todo.push_back(succ[i]);
        }
      }
    }
    return checked;
  }
  for (u64 idx = first; idx < first + n && idx < hm.n_init; ++idx) {
    const u64 s0 = init_state(L, idx);
    const u64 msgs = s0 & L.msgs_mask;
    const CompMsgs cm = comp_msgs_init(L, s0);
    if (idx < first + 16 && code_bits(L) <= 16) {
      // the kernel's branch-free code functions vs the branching ones on every
      // code of the first components, reachable or not
      const CodeConsts kc = code_consts(L, cm);
      u64 tab[STEP_TAB];
      for (int i = 0; i < STEP_TAB; ++i) tab[i] = compactor_step_entry(L, i);
      const uint32_t imask = lane_inv_mask(L, kc);
      const int term_c = lane_term_consts(L, kc);
      for (ckey cd = 0; cd < (1u << code_bits(L)); ++cd) {
        ckey t1 = 0, t2 = 0, t3 = 0;
        int a1 = -1, a2 = -1, a3 = -1;
        const int r1 = compactor_step_c(L, kc, cd, c_phase(L, cd), &t1, &a1);
        const int r2 = compactor_step_cb(L, kc, cd, &t2, &a2);
        if (r1 != r2 || a1 != a2 || (r1 == 1 && t1 != t2) || check_invariants_c(L, kc, cd) != check_invariants_cb(L, kc, cd))
          return -(1 + checked);
        // the per-lane kernel's invariant features against the component's mask
        if (((lane_inv_feat(L, cd) & imask) != 0) != (check_invariants_cb(L, kc, cd) != -1)) return -(1 + checked);
        if (L.C <= 3) {  // the per-lane kernel's table form (component_lane.h), its stutter flag included
          uint32_t term = 0;
          const int r3 = compactor_step_tab(L, kc, tab, cd, &t3, &a3, &term);
          if (r3 != r1 || a3 != a1 || (r1 == 1 && t3 != t1)) return -(1 + checked);
          if (selfloop_count_tab(L, term_c, term) != selfloop_count_c(L, kc, cd)) return -(1 + checked);
        }
      }
    }
    std::unordered_set<u64> seen{s0};
    std::vector<u64> todo{s0};
    while (!todo.empty()) {
      const u64 s = todo.back();
      todo.pop_back();
      if ((s & L.msgs_mask) != msgs || (s >> mb) > 0xffffffffull) return -(1 + checked);
      const lkey k = (lkey)(s >> mb);
      u64 t1 = 0, t2w = 0;
      lkey t2 = 0, c2 = 0;
      int a1 = -1, a2 = -1;
      const int r1 = compactor_step_ph(L, s, st_phase(L, s), &t1, &a1);
      const int r2 = compactor_step_k(L, cm, msgs, k, k_phase(L, k), &t2, &a2);
      const int x1 = crash_step(L, s, &t2w), x2 = crash_step_k(L, k, &c2);
      lkey t3 = 0;
      int a3 = -1;
      const int r3 = compactor_step_k_sel(L, cm, msgs, k, k_phase(L, k), &t3, &a3);  // the branch-free form
      if (r3 != r1 || a3 != a1 || (r1 == 1 && t3 != t2)) return -(1 + checked);
      {  // component codes
        const CodeConsts kc = code_consts(L, cm);
        const ckey cd = code_encode(L, k);
        ckey ct = 0, cx = 0;
        int ca = -1;
        const int rc = compactor_step_c(L, kc, cd, c_phase(L, cd), &ct, &ca);
        const int xc = crash_step_c(L, cd, &cx);
        if (code_decode(L, kc, cd) != k || rc != r1 || ca != a1 || (r1 == 1 && code_decode(L, kc, ct) != t2) ||
            xc != x2 || (xc && code_decode(L, kc, cx) != c2) ||
            check_invariants_c(L, kc, cd) != check_invariants_k(L, cm, k) ||
            selfloop_count_c(L, kc, cd) != selfloop_count_k(L, cm, k))
          return -(1 + checked);
      }
      if (r1 != r2 || a1 != a2 || (r1 == 1 && t1 != (msgs | ((u64)t2 << mb))) || x1 != x2 ||
          (x1 && t2w != (msgs | ((u64)c2 << mb))) || check_invariants(L, s) != check_invariants_k(L, cm, k) ||
          selfloop_count(L, s) != selfloop_count_k(L, cm, k))
        return -(1 + checked);
      // the invariants also on words off the reachable space: every single
      // ledger-position bit flipped (ledgers that are not prefix-closed, where
      // readings of CompactionHorizonCorrectness can differ) and every
      // compactionHorizon value
      for (int j1 = 1; j1 <= L.C; ++j1)
        for (int p = 0; p <= L.N; ++p) {
          const u64 v = s ^ (1ull << (led_base(L, j1) + p));
          if (check_invariants(L, v) != check_invariants_k(L, cm, (lkey)(v >> mb))) return -(1 + checked);
        }
      for (u64 h = 0; h < (1ull << L.hz_w); ++h) {
        const u64 v = fset(s, L.hz_sh, L.hz_w, h);
        if (check_invariants(L, v) != check_invariants_k(L, cm, (lkey)(v >> mb))) return -(1 + checked);
      }
      ++checked;
      u64 succ[64];
      const int nsucc = host_successors(L, s, succ, nullptr, 64);
      for (int i = 0; i < nsucc && i < 64; ++i)
        if (seen.insert(succ[i]).second) todo.push_back(succ[i]);
    }
  }
  return checked;
}

// The per-lane kernel's two table-borne predicates (component_lane.h) on
// every code below 2^code_bits and every class of component constants -- len
// 0..N x the 32 combinations of msgs_ok, hz_live, hz_false, dn0, dn1,
// reachable or not: the invariant features against the mask
// (component_code.h lane_inv_feat / lane_inv_mask vs check_invariants_cb) and
// the step entry's stutter flag (vs selfloop_count_c).  Returns the (code,
// class) pairs checked, -(1 + index) of the first pair that disagrees, 0 for
// a model the pass does not take, -1 on a bad model.
int64_t tlcg_host_lane_inv_selfcheck(const tlcg_model* m) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  const Layout& L = hm.L;
  if (L.producer || hm.user || L.N > 8 || L.C > 3 || code_bits(L) > 16) return 0;
  u64 tab[STEP_TAB];
  for (int i = 0; i < STEP_TAB; ++i) tab[i] = compactor_step_entry(L, i);
  int64_t checked = 0;
  for (int len = 0; len <= L.N; ++len)
    for (int f = 0; f < 32; ++f) {
      CodeConsts kc{};
      kc.len = (uint32_t)len;
      kc.ledbits = 1u;
      kc.msgs_ok = f & 1;
      kc.hz_live = (f >> 1) & 1;
      kc.hz_false = (f >> 2) & 1;
      kc.dn0 = (f >> 3) & 1;
      kc.dn1 = (f >> 4) & 1;
      const uint32_t imask = lane_inv_mask(L, kc);
      const int term_c = lane_term_consts(L, kc);
      for (ckey cd = 0; cd < (1u << code_bits(L)); ++cd) {
        ckey t = 0;
        int act = -1;
        uint32_t term = 0;
        compactor_step_tab(L, kc, tab, cd, &t, &act, &term);
        if (((lane_inv_feat(L, cd) & imask) != 0) != (check_invariants_cb(L, kc, cd) != -1) ||
            selfloop_count_tab(L, term_c, term) != selfloop_count_c(L, kc, cd))
          return -(1 + checked);
        ++checked;
      }
    }
  return checked;
}

// The per-lane kernel's owner table as build_lane_phash fills it (round 8),
// entry by entry against S walked here on its own (component 0's FIFO BFS,
// compactor_step_cb and crash_step_c): each code of S sits in its slot with
// code + 1, lane_inv_feat and the step index in the first word -- the index
// being the one compactor_step_tab computes, and the entry it selects giving
// compactor_step_cb's successor, result and action -- and its BFS position in
// the second, the positions a bijection onto 0..|S| - 1; every other slot is
// empty.  *overflow (when given): a
// field of some code of S does not fit its bits, by plain arithmetic (the
// pass must then be refused).  Returns |S|, 0 when build_lane_phash refuses
// the model, -(1 + position) of the first code that disagrees, -1 on a bad
// model.
int64_t tlcg_host_lane_owner_selfcheck(const tlcg_model* m, int* overflow) {
  HostModel hm;
  std::string e;
  if (overflow) *overflow = 0;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  const Layout& L = hm.L;
  std::vector<uint32_t> owner(2 * LANE_T);
  uint32_t mult = 0;
  const bool taken = build_lane_phash(hm, &mult, owner.data(), nullptr);
  if (L.producer || code_bits(L) > 16) return taken ? -1 : 0;
  const u128 s0 = init_state<u128>(L, 0);
  const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)s0));
  std::vector<uint32_t> q{code_encode_w<u128>(L, s0)};
  std::unordered_set<uint32_t> seen{q[0]};
  for (size_t head = 0; head < q.size() && q.size() <= 64; ++head) {
    ckey t = 0, t2 = 0;
    int act = 0;
    if (compactor_step_cb(L, kc, q[head], &t, &act) == 1 && seen.insert(t).second) q.push_back(t);
    if (crash_step_c(L, q[head], &t2) && seen.insert(t2).second) q.push_back(t2);
  }
  // the step index by plain arithmetic on the code's layout: phase, R, the largest ledger present
  auto plain_index = [&](uint32_t c) {
    uint32_t mx = 0;
    for (int j = 0; j < L.C; ++j)
      if ((c >> j) & 1u) mx = (uint32_t)j + 1u;
    return ((c >> (L.C + 2)) & 7u) | (((c >> L.C) & 1u) << 3) | (mx << 4);
  };
  bool ovf = q.size() > 62;
  for (uint32_t c : q)
    if (c + 1u >= (1u << 16) || lane_inv_feat(L, c) >= (1u << 9) || plain_index(c) >= (1u << 6)) ovf = true;
  if (overflow) *overflow = ovf ? 1 : 0;
  if (!taken) return 0;
  if (ovf) return -1;  // (taken although a field does not fit)
  u64 tab[STEP_TAB];
  for (int i = 0; i < STEP_TAB; ++i) tab[i] = compactor_step_entry(L, i);
  std::vector<int> slot_used(LANE_T, 0);
  u64 dense_seen = 0;
  for (size_t i = 0; i < q.size(); ++i) {
    const ckey c = q[i];
    const unsigned sl = lane_slot(c, mult);
    const uint32_t w = owner[2 * sl], d = owner[2 * sl + 1];
    const uint32_t ix = w >> LANE_OWNER_STEP_SH;
    ckey t = 0, t3 = 0;
    int a1 = -1, a3 = -1;
    const int r1 = compactor_step_cb(L, kc, c, &t, &a1);
    const int r3 = ix < (uint32_t)STEP_TAB ? compactor_step_ent(L, kc, tab[ix], ix & 7u, c, &t3, &a3) : -1;
    if (slot_used[sl]++ || (w & 0xFFFFu) != c + 1u || ((w >> LANE_OWNER_FEAT_SH) & 0x1FFu) != lane_inv_feat(L, c) ||
        ix != plain_index(c) || r3 != r1 || (r1 == 1 && t3 != t) || (r1 && a3 != a1) || d != (uint32_t)i || d >= q.size() || ((dense_seen >> d) & 1))
      return -(1 + (int64_t)i);
    dense_seen |= 1ull << d;
  }
  if (dense_seen != (q.size() >= 64 ? ~0ull : (1ull << q.size()) - 1)) return -(1 + (int64_t)q.size());
  for (int s = 0; s < LANE_T; ++s)
    if (!slot_used[s] && (owner[2 * s] || owner[2 * s + 1])) return -(1 + (int64_t)q.size());
  return (int64_t)q.size();
}

// The per-lane kernel's prefix form (component_lane.h, round 10) replayed on
// the host: the components of [first, first + n) whose FIFO BFS in the
// kernel's order (compactor successor, then BrokerCrash's, each appended when
// new) starts at S's code of dense index 0 and finds, at every insert, the
// owner entry of the inserted code with dense index = the queue's length --
// the test the kernel makes, through the same table and slot hash.  These are
// the components the prefix form keeps; the others go to the cascade.
// Components past the model's last are not counted.  Returns 0 when
// build_lane_phash refuses the model, -1 on a bad model.
int64_t tlcg_host_lane_prefix_selfcheck(const tlcg_model* m, uint64_t first, uint64_t n) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  const Layout& L = hm.L;
  std::vector<uint32_t> owner(2 * LANE_T);
  uint32_t mult = 0;
  if (!build_lane_phash(hm, &mult, owner.data(), nullptr)) return 0;
  // the entry of code c: its dense index, or -1 when c is not in S
  auto dense = [&](ckey c) -> int64_t {
    const unsigned sl = lane_slot(c, mult);
    return (owner[2 * sl] & 0xFFFFu) == c + 1u ? (int64_t)owner[2 * sl + 1] : -1;
  };
  int64_t kept = 0;
  for (u64 idx = first; idx < first + n && idx < hm.n_init; ++idx) {
    const u128 s0 = init_state<u128>(L, idx);
    const CodeConsts kc = code_consts(L, comp_msgs_init(L, (u64)s0));
    std::vector<ckey> q{code_encode_w<u128>(L, s0)};
    // (the set is kept on its own here, so "new" is not the kernel's d >= tail)
    std::unordered_set<uint32_t> seen{q[0]};
    bool ok = dense(q[0]) == 0;
    auto put = [&](ckey t) {
      if (!seen.insert(t).second) return;
      ok = ok && dense(t) == (int64_t)q.size();
      q.push_back(t);
    };
    for (size_t head = 0; ok && head < q.size(); ++head) {
      ckey t = 0, t2 = 0;
      int act = 0;
      if (compactor_step_cb(L, kc, q[head], &t, &act) == 1) put(t);
      if (ok && crash_step_c(L, q[head], &t2)) put(t2);
    }
    kept += ok ? 1 : 0;
  }
  return kept;
}

// word 0 of the owner entry of an arbitrary code (component_code.h
// lane_owner_word; 0: a field does not fit), -1 on a bad model
int64_t tlcg_host_lane_owner_word(const tlcg_model* m, uint32_t code) {
  HostModel hm;
  std::string e;
  if (!m || !build_model(*m, &hm, &e)) return -1;
  return (int64_t)lane_owner_word(hm.L, code);
}

}  // extern "C"
