// Host-only runner of the user invariants' generated code (user_inv.cpp
// user_device_source), built with -fsanitize=address,undefined by
// tests/test_user_codegen_host.py.  No GPU, no HIP runtime: the generated text
// is plain C++ over the headers the run-time specialized kernels include.
//
//   user_codegen_run emit INPUT     the generated text of INPUT's model, once
//                                   per TLCG_UTAB setting ("@@UTAB <setting>"
//                                   before each: unset, 0, dyn, slow)
//   user_codegen_run run INPUT      every user invariant on every state
//
// INPUT: the constants, the invariants' names, the user_defs text and the
// packed states (the format tests/user_eval_cases.py write_input writes).
//
// `run` prints one line per state: four characters per invariant,
//   (a) the interpreter (user_inv.h eval_user),
//   (b) the generated tlcg_user_eval over the word (model.h UVWord),
//   (c) the generated tlcg_user_eval over the component code (UVCode),
//   (d) code_consts_user + user_eval_c (the outcome tables),
// each an EV_* digit; (c) and (d) are 'x' for a state without a component
// code (its word does not come back from code_encode / the code's word).
// (b)-(d) need the generated text compiled in (-DTLCG_GEN_SRC='"file"', and
// -DTLCG_GEN_WIDE for a two-word layout); without it they print '-', and 'x'
// as before.  Then "H <k> <opcode>[:imm] <count>" for the needed instructions
// reachable from invariant k's entry.
#if defined(TLCG_GEN_SRC)
#define TLCG_USER_INV 1
#define __constant__
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "component_code.h"
#include "host_model.h"

#if defined(TLCG_GEN_SRC)
#include TLCG_GEN_SRC
#endif

namespace {

const char* const kOpNames[] = {
    "U_LDI", "U_MOV", "U_LEN", "U_MKEY", "U_MVAL", "U_PHASE", "U_P1R", "U_HZ", "U_CTX", "U_CRASH", "U_CURP",
    "U_CURH", "U_CURC", "U_LEDP", "U_LEDM", "U_LFK", "U_ADD", "U_SUB", "U_MUL", "U_DIV", "U_MOD", "U_NEG",
    "U_EQ", "U_NE", "U_LT", "U_LE", "U_NOT", "U_AND", "U_OR", "U_ADDI", "U_BIT", "U_POPC", "U_NTH", "U_MASK",
    "U_KIN", "U_KAT", "U_JMP", "U_JZ", "U_JNZ", "U_ERR", "U_RET"};
static_assert(sizeof kOpNames / sizeof kOpNames[0] == (size_t)tlcg::U_RET + 1, "kOpNames follows user_inv.h UOp");
static_assert(tlcg::U_LDI == 0 && tlcg::U_LFK == 15 && tlcg::U_BIT == 30 && tlcg::U_KAT == 35, "UOp order");

struct Input {
  tlcg_model m{};
  std::string defs;
  std::vector<std::string> invariants;
  int words = 1;
  std::vector<uint64_t> states;  // words per state
};

bool read_input(const char* path, Input* in) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::string tag;
  int consumer = 0, producer = 0, retain = 0, deadlock = 0, n = 0;
  if (!(f >> tag >> in->m.msg_sent_limit >> in->m.compaction_times_limit >> in->m.consume_times_limit >>
        in->m.max_crash_times >> consumer >> producer >> retain >> deadlock) || tag != "model")
    return false;
  in->m.model_consumer = (uint8_t)consumer;
  in->m.model_producer = (uint8_t)producer;
  in->m.retain_null_key = (uint8_t)retain;
  in->m.check_deadlock = (uint8_t)deadlock;
  if (!(f >> tag >> n) || tag != "keys" || n < 0 || n > TLCG_MAX_SET) return false;
  in->m.n_keys = n;
  for (int i = 0; i < n; ++i) f >> in->m.keys[i];
  if (!(f >> tag >> n) || tag != "values" || n < 0 || n > TLCG_MAX_SET) return false;
  in->m.n_values = n;
  for (int i = 0; i < n; ++i) f >> in->m.values[i];
  if (!(f >> tag >> n) || tag != "invariants" || n < 1 || n > TLCG_MAX_INV) return false;
  in->invariants.resize((size_t)n);
  for (std::string& s : in->invariants) f >> s;
  size_t bytes = 0;
  if (!(f >> tag >> bytes) || tag != "defs" || bytes > (1u << 20)) return false;
  f.get();  // the newline after the count
  in->defs.resize(bytes);
  if (!f.read(&in->defs[0], (std::streamsize)bytes)) return false;
  size_t ns = 0;
  if (!(f >> tag >> ns >> in->words) || tag != "states" || in->words < 1 || in->words > 2 || ns > (1u << 24))
    return false;
  in->states.resize(ns * (size_t)in->words);
  for (uint64_t& w : in->states) {
    std::string h;
    if (!(f >> h)) return false;
    w = std::strtoull(h.c_str(), nullptr, 16);
  }
  // the invariants by their definitions' indices (tlcg_model.invariants)
  const std::vector<std::string> names = tlcg::user_def_names(in->defs.c_str());
  in->m.n_invariants = (int32_t)in->invariants.size();
  for (size_t q = 0; q < in->invariants.size(); ++q) {
    size_t k = 0;
    while (k < names.size() && names[k] != in->invariants[q]) ++k;
    if (k == names.size()) return false;
    in->m.invariants[q] = TLCG_INV_USER + (int32_t)k;
  }
  in->m.user_defs = in->defs.c_str();
  return true;
}

// the needed instructions reachable from entry k, by opcode (U_KIN / U_KAT by set)
std::map<std::string, long> histogram(const tlcg::UserProg& P, const tlcg::UserProg& pruned, int k) {
  std::map<std::string, long> h;
  std::vector<bool> seen((size_t)P.n_ins, false);
  std::vector<int> todo{P.entry[k]};
  while (!todo.empty()) {
    const int pc = todo.back();
    todo.pop_back();
    if (pc < 0 || pc >= P.n_ins || seen[(size_t)pc]) continue;
    seen[(size_t)pc] = true;
    const tlcg::UInsn& in = P.ins[pc];
    if (in.op != tlcg::U_RET && in.op != tlcg::U_ERR) {
      if (in.op != tlcg::U_JMP) todo.push_back(pc + 1);
      if (in.op == tlcg::U_JMP || in.op == tlcg::U_JZ || in.op == tlcg::U_JNZ) todo.push_back(in.imm);
    }
    if (std::memcmp(&in, &pruned.ins[pc], sizeof in) != 0) continue;  // (dead: user_prune_dead replaced it)
    std::string name = in.op <= tlcg::U_RET ? kOpNames[in.op] : "unknown";
    if (in.op == tlcg::U_KIN || in.op == tlcg::U_KAT) name += in.imm ? ":1" : ":0";
    ++h[name];
  }
  return h;
}

template <typename W>
int run(const Input& in, const tlcg::HostModel& hm) {
  const tlcg::Layout& L = hm.L;
  const tlcg::UserProg& P = *hm.user;
  const bool coded = !(L.N > 8 || tlcg::code_bits(L) > 31);
  std::printf("@@RUN n_user %d states %zu words %d generated %d coded %d\n", P.n_user,
              in.states.size() / (size_t)in.words, in.words,
#if defined(TLCG_GEN_SRC)
              1,
#else
              0,
#endif
              coded ? 1 : 0);
  std::string line;
  for (size_t i = 0; i < in.states.size(); i += (size_t)in.words) {
    const W s = (W)tlcg::join_words(&in.states[i], in.words);
    const tlcg::CodeConsts K = tlcg::code_consts(L, tlcg::comp_msgs_init(L, (uint64_t)s));
    const tlcg::ckey c = tlcg::code_encode_w<W>(L, s);
    const bool has_code = coded && tlcg::UVCode<W>{L, K, c}.word() == s;
#if defined(TLCG_GEN_SRC)
    tlcg::CodeConsts Kd = K;
    if (has_code) tlcg::code_consts_user<W>(L, Kd);
#endif
    line.clear();
    for (int k = 0; k < P.n_user; ++k) {
      line += (char)('0' + tlcg::eval_user<W>(L, P, k, s));
#if defined(TLCG_GEN_SRC)
      line += (char)('0' + tlcg::tlcg_user_eval(k, tlcg::UVWord<W>{L, s}));
      line += has_code ? (char)('0' + tlcg::tlcg_user_eval(k, tlcg::UVCode<W>{L, K, c})) : 'x';
      line += has_code ? (char)('0' + tlcg::user_eval_c<W>(L, Kd, k, c)) : 'x';
#else
      line += '-';
      line += has_code ? '-' : 'x';
      line += has_code ? '-' : 'x';
#endif
    }
    std::puts(line.c_str());
  }
  const tlcg::UserProg pruned = tlcg::user_prune_dead(P);
  for (int k = 0; k < P.n_user; ++k)
    for (const auto& e : histogram(P, pruned, k)) std::printf("H %d %s %ld\n", k, e.first.c_str(), e.second);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s emit|run INPUT\n", argv[0]);
    return 2;
  }
  Input in;
  if (!read_input(argv[2], &in)) {
    std::fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  tlcg::HostModel hm;
  std::string err;
  if (!tlcg::build_model(in.m, &hm, &err) || !hm.user) {
    std::fprintf(stderr, "the model does not build: %s\n", err.c_str());
    return 2;
  }
  if (tlcg::state_words(hm.L) != in.words) {
    std::fprintf(stderr, "the layout takes %d words, the input has %d\n", tlcg::state_words(hm.L), in.words);
    return 2;
  }
  const std::string mode = argv[1];
  if (mode == "emit") {
    const char* const settings[][2] = {{"unset", nullptr}, {"0", "0"}, {"dyn", "dyn"}, {"slow", "slow"}};
    for (const auto& s : settings) {
      if (s[1]) setenv("TLCG_UTAB", s[1], 1);
      else unsetenv("TLCG_UTAB");
      std::printf("@@UTAB %s\n%s", s[0], tlcg::user_device_source(*hm.user, hm.L).c_str());
    }
    return 0;
  }
  if (mode != "run") return 2;
#if defined(TLCG_GEN_WIDE)
  if (in.words != 2) return 2;
  return run<tlcg::u128>(in, hm);
#else
  if (in.words != 1) {
#if defined(TLCG_GEN_SRC)
    return 2;  // (the generated text of a two-word layout is built with -DTLCG_GEN_WIDE)
#else
    return run<tlcg::u128>(in, hm);
#endif
  }
  return run<tlcg::u64>(in, hm);
#endif
}
