// Host-only fuzz harness for the temporal front end (user_inv.cpp
// compile_property), built with -fsanitize=address,undefined by
// tests/test_property_host.py from host_model.cpp and user_inv.cpp.  No GPU,
// no HIP runtime.
//
//   property_fuzz MUTANTS SEED
//
// Every accepted spelling below is classified as written (the form must be the
// one listed) and as MUTANTS deterministic mutations; each call must end in a
// form or in a message, never a crash or undefined behaviour, and an accepted
// property's P and Q evaluate to TRUE / FALSE / error on every reachable state
// of a small model.  Prints one summary line; exit 0 unless a check fails (the
// sanitizers abort on their own findings).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "host_model.h"

namespace {

struct Spelling {
  int form;
  const char* body;
};

const Spelling kSpellings[] = {
    {TLCG_PROP_EVENTUALLY, "<>(cursor # Nil)"},
    {TLCG_PROP_EVENTUALLY, "<>Done"},
    {TLCG_PROP_EVENTUALLY, "(<>(compactionHorizon > 0 /\\ cursor # Nil))"},
    {TLCG_PROP_INFINITELY_OFTEN, "[]<>(compactorState = Compactor_In_PhaseOne)"},
    {TLCG_PROP_INFINITELY_OFTEN, "[]<>Done"},
    {TLCG_PROP_LEADS_TO, "compactorState = Compactor_In_PhaseTwoUpdateContext ~> cursor # Nil"},
    {TLCG_PROP_LEADS_TO, "(crashTimes = MaxCrashTimes /\\ crashTimes > 0) ~> compactorState = Compactor_In_PhaseTwoWrite"},
    {TLCG_PROP_LEADS_TO, "(\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil) ~> compactionHorizon > 0"},
    {TLCG_PROP_LEADS_TO, "[]((\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil) => <>(compactionHorizon > 0))"},
    {TLCG_PROP_LEADS_TO, "[](Done => <>Done)"},
    {TLCG_PROP_LEADS_TO, "  (/\\ crashTimes > 0\n   /\\ cursor = Nil) ~> (\\/ cursor # Nil\n                       \\/ Done)"},
};

const char* const kTokens[] = {"<>", "[]", "~>", " => ", " <=> ", "(", ")", "/\\ ", "\\/ ", "'", "ENABLED ", "WF_vars(Next)",
                               "SF_vars(Next)", "\\E i \\in 1..2 : ", "IF ", " THEN ", " ELSE ", "CASE ", " -> ", "~", "\n",
                               "  ", "Done", "cursor", "Nil", "<<", ">>", "[", "]", "{", "}", "\\* c\n", "(* c *)",
                               "@@DEF X\n", "1", " # ", " = "};

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

std::vector<uint64_t> reachable(const tlcg::HostModel& hm) {
  std::vector<uint64_t> all;
  std::unordered_set<uint64_t> seen;
  for (uint64_t i = 0; i < hm.n_init; ++i) {
    const uint64_t s = tlcg::init_state<uint64_t>(hm.L, i);
    if (seen.insert(s).second) all.push_back(s);
  }
  std::vector<uint64_t> out(256);
  for (size_t k = 0; k < all.size(); ++k) {
    const int n = tlcg::host_successors<uint64_t>(hm.L, all[k], out.data(), nullptr, (int)out.size());
    for (int j = 0; j < n; ++j)
      if (seen.insert(out[(size_t)j]).second) all.push_back(out[(size_t)j]);
  }
  return all;
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
  const std::vector<uint64_t> states = reachable(hm);
  const std::unique_ptr<tlcg::UserProg> prog(new tlcg::UserProg);
  long accepted = 0, refused = 0, not_temporal = 0, unmutated_ok = 0, evals = 0, errors = 0;
  long forms[3] = {0, 0, 0};
  for (const Spelling& sp : kSpellings) {
    for (int k = 0; k <= mutants; ++k) {
      const std::string body = k == 0 ? sp.body : mutate(sp.body, rng);
      const std::string text = "@@DEF Done\ncompactorState = Compactor_In_PhaseTwoWrite /\\ crashTimes = MaxCrashTimes\n"
                               "@@DEF Prop @7\n" + body + "\n";
      m.user_defs = text.c_str();
      int form = -1;
      std::string msg;
      const int rc = tlcg::compile_property(m, hm, "Prop", &form, prog.get(), &msg);
      if (rc != 0) {
        if (msg.empty() || rc > 0) {
          std::fprintf(stderr, "a refusal without a message (rc %d): %s\n", rc, body.c_str());
          return 1;
        }
        if (k == 0) {
          std::fprintf(stderr, "an accepted spelling is refused: %s: %s\n", body.c_str(), msg.c_str());
          return 1;
        }
        ++(rc == -2 ? not_temporal : refused);
        continue;
      }
      if (form < 0 || form > 2 || (k == 0 && form != sp.form)) {
        std::fprintf(stderr, "form %d for %s\n", form, body.c_str());
        return 1;
      }
      // the form alone (no program kept) must agree
      int form2 = -1;
      if (tlcg::compile_property(m, hm, "Prop", &form2, nullptr, &msg) != 0 || form2 != form) {
        std::fprintf(stderr, "the form-only call disagrees on %s\n", body.c_str());
        return 1;
      }
      ++accepted;
      ++forms[form];
      if (k == 0) ++unmutated_ok;
      for (uint64_t s : states)
        for (int e = 0; e < 2; ++e) {
          const int r = tlcg::eval_user<uint64_t>(hm.L, *prog, e, s);
          if (r != tlcg::EV_TRUE && r != tlcg::EV_FALSE && r != tlcg::EV_ERROR) {
            std::fprintf(stderr, "evaluation returned %d on %s\n", r, body.c_str());
            return 1;
          }
          if (e == 0 && form != TLCG_PROP_LEADS_TO && r != tlcg::EV_TRUE) {
            std::fprintf(stderr, "entry 0 of a form without P is not TRUE: %s\n", body.c_str());
            return 1;
          }
          ++evals;
          errors += r == tlcg::EV_ERROR;
        }
    }
  }
  std::printf("{\"spellings\": %zu, \"unmutated_ok\": %ld, \"accepted\": %ld, \"refused\": %ld, \"not_temporal\": %ld, "
              "\"eventually\": %ld, \"infinitely_often\": %ld, \"leads_to\": %ld, \"states\": %zu, \"evals\": %ld, "
              "\"errors\": %ld}\n",
              sizeof kSpellings / sizeof kSpellings[0], unmutated_ok, accepted, refused, not_temporal, forms[0], forms[1],
              forms[2], states.size(), evals, errors);
  return 0;
}
