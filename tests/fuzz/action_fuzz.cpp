// Host-only fuzz harness for the action front end (user_inv.cpp
// compile_action_property) and the two-state interpreter (user_inv.h
// eval_user2_v), built with -fsanitize=address,undefined by
// tests/test_action_property_host.py from host_model.cpp and user_inv.cpp.  No
// GPU, no HIP runtime.
//
//   action_fuzz MUTANTS SEED
//
// Every accepted spelling below is compiled as written (it must be accepted)
// and as MUTANTS deterministic mutations; each call must end in a program or in
// a message, never a crash or undefined behaviour, and an accepted program
// returns TRUE / FALSE / error on every step of a small model.  Prints one
// summary line; exit 0 unless a check fails (the sanitizers abort on their own
// findings).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "host_model.h"

namespace {

const char* const kSpellings[] = {
    "[][crashTimes' >= crashTimes /\\ crashTimes' <= crashTimes + 1]_vars",
    "[][compactionHorizon' >= compactionHorizon]_vars",
    "([][compactedTopicContext' >= compactedTopicContext]_compactorVars)",
    "[][Len(messages') >= Len(messages) /\\ \\A i \\in 1..Len(messages) : messages'[i] = messages[i]]_messages",
    "[][(\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil /\\ compactedLedgers'[i] = Nil)\n"
    "     => compactorState = Compactor_In_PhaseTwoDeleteLedger]_vars",
    "[][cursor' # cursor => compactorState' = Compactor_In_PhaseTwoDeleteLedger]_<<cursor, compactorState>>",
    "[][compactorState' = compactorState => UNCHANGED <<compactedLedgers, cursor>>]_vars",
    "[][crashTimes' # crashTimes => UNCHANGED bookieVars /\\ phaseOneResult' = Nil]_vars",
    "[][phaseOneResult = Nil \\/ phaseOneResult' = Nil\n"
    "    \\/ phaseOneResult'.readPosition = phaseOneResult.readPosition]_vars",
    "[][cursor # Nil => cursor' # Nil /\\ cursor'.compactionHorizon >= cursor.compactionHorizon]_cursor",
    "[][Len(compactedLedgers'[compactedTopicContext']) >= 0]_vars",
    "[][ /\\ (Done => crashTimes' >= crashTimes)\n    /\\ LET d == compactionHorizon' - compactionHorizon IN d >= 0 ]_pair",
    "[][phaseOneResult' # Nil => \\A k \\in DOMAIN phaseOneResult'.latestForKey :\n"
    "      messages'[phaseOneResult'.latestForKey[k]].key = k]_vars",
};

const char* const kTokens[] = {"'", "''", "[]", "[", "]", "_", "_vars", "_<<", ">>", "<<", "UNCHANGED ", "ENABLED ",
                               "\\cdot ", "WF_vars(Next)", "<>", "(", ")", "/\\ ", "\\/ ", " => ", "\n", "  ", "Done",
                               "cursor", "messages", "Nil", "vars", "bookieVars", "{", "}", "\\* c\n", "(* c *)",
                               "@@DEF X\n", "1", " # ", " = ", "LET x == ", " IN ", "\\A i \\in 1..2 : "};

struct Rng {
  uint64_t x;
  uint64_t next() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  }
  size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

std::string mutate(const std::string& s, Rng& r) {
  std::string t = s;
  const int edits = 1 + (int)r.below(3);
  for (int e = 0; e < edits; ++e) {
    const size_t at = r.below(t.size() + 1);
    switch (r.below(5)) {
      case 0:
        if (!t.empty()) t.erase(r.below(t.size()), 1);
        break;
      case 1:
        t.insert(at, kTokens[r.below(sizeof kTokens / sizeof kTokens[0])]);
        break;
      case 2: {
        const size_t a = r.below(t.size() + 1), n = r.below(12);
        t.insert(at, t.substr(a, n));
        break;
      }
      case 3:
        t.resize(at);
        break;
      default:
        if (!t.empty()) t[r.below(t.size())] = (char)(32 + r.below(95));
        break;
    }
  }
  return t;
}

tlcg_model small_model() {
  tlcg_model m{};
  m.msg_sent_limit = 2;
  m.compaction_times_limit = 2;
  m.max_crash_times = 1;
  m.retain_null_key = 1;
  m.check_deadlock = 1;
  m.n_keys = 2;
  m.keys[0] = 1;
  m.keys[1] = 2;
  m.n_values = 1;
  m.values[0] = 1;
  return m;
}

// every step (s, t), t a successor of s that differs from it
std::vector<std::pair<uint64_t, uint64_t>> steps_of(const tlcg::HostModel& hm) {
  std::vector<uint64_t> all;
  std::unordered_set<uint64_t> seen;
  for (uint64_t i = 0; i < hm.n_init; ++i) {
    const uint64_t s = tlcg::init_state<uint64_t>(hm.L, i);
    if (seen.insert(s).second) all.push_back(s);
  }
  std::vector<std::pair<uint64_t, uint64_t>> steps;
  std::vector<uint64_t> out(256);
  for (size_t k = 0; k < all.size(); ++k) {
    const int n = tlcg::host_successors<uint64_t>(hm.L, all[k], out.data(), nullptr, (int)out.size());
    for (int j = 0; j < n; ++j) {
      if (out[(size_t)j] != all[k]) steps.push_back({all[k], out[(size_t)j]});
      if (seen.insert(out[(size_t)j]).second) all.push_back(out[(size_t)j]);
    }
  }
  return steps;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s MUTANTS SEED\n", argv[0]);
    return 2;
  }
  const int mutants = std::atoi(argv[1]);
  Rng rng{std::strtoull(argv[2], nullptr, 10) | 1};
  tlcg::HostModel hm;
  std::string err;
  tlcg_model m = small_model();
  if (!tlcg::build_model(m, &hm, &err)) {
    std::fprintf(stderr, "the small model does not build: %s\n", err.c_str());
    return 1;
  }
  const auto steps = steps_of(hm);
  const std::unique_ptr<tlcg::UserProg> prog(new tlcg::UserProg);
  long accepted = 0, refused = 0, not_action = 0, unmutated_ok = 0, evals = 0;
  long outcome[3] = {0, 0, 0};
  for (const char* sp : kSpellings) {
    for (int k = 0; k <= mutants; ++k) {
      const std::string body = k == 0 ? sp : mutate(sp, rng);
      const std::string text = "@@DEF Done\ncompactorState = Compactor_In_PhaseTwoWrite /\\ crashTimes = MaxCrashTimes\n"
                               "@@DEF pair\n<<compactionHorizon, <<cursor>>>>\n"
                               "@@DEF Prop @9\n" + body + "\n";
      m.user_defs = text.c_str();
      uint32_t mask = 0;
      std::string msg;
      const int rc = tlcg::compile_action_property(m, hm, "Prop", &mask, prog.get(), &msg);
      if (rc != 0) {
        if (msg.empty() || rc > 0 || rc < -3) {
          std::fprintf(stderr, "a refusal without a message (rc %d): %s\n", rc, body.c_str());
          return 1;
        }
        if (k == 0) {
          std::fprintf(stderr, "an accepted spelling is refused: %s: %s\n", body.c_str(), msg.c_str());
          return 1;
        }
        ++(rc == -1 ? refused : not_action);
        continue;
      }
      // the front end alone (no program kept) must agree
      uint32_t mask2 = 0;
      if (tlcg::compile_action_property(m, hm, "Prop", &mask2, nullptr, &msg) != 0 || mask2 != mask || mask >= 1u << 9) {
        std::fprintf(stderr, "the form-only call disagrees on %s\n", body.c_str());
        return 1;
      }
      ++accepted;
      if (k == 0) ++unmutated_ok;
      for (const auto& st : steps) {
        const int r = tlcg::eval_user2<uint64_t>(hm.L, *prog, 0, st.first, st.second);
        if (r != tlcg::EV_TRUE && r != tlcg::EV_FALSE && r != tlcg::EV_ERROR) {
          std::fprintf(stderr, "evaluation returned %d on %s\n", r, body.c_str());
          return 1;
        }
        ++evals;
        ++outcome[r];
      }
    }
  }
  std::printf("{\"spellings\": %zu, \"unmutated_ok\": %ld, \"accepted\": %ld, \"refused\": %ld, \"not_action\": %ld, "
              "\"steps\": %zu, \"evals\": %ld, \"true\": %ld, \"false\": %ld, \"error\": %ld}\n",
              sizeof kSpellings / sizeof kSpellings[0], unmutated_ok, accepted, refused, not_action, steps.size(), evals,
              outcome[0], outcome[1], outcome[2]);
  return 0;
}
