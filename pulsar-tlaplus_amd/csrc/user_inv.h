// pulsar-tlaplus_amd/csrc/user_inv.h -- invariants a user adds to the module
// (BASELINE config 5: "mutated compaction.tla with an injected invariant
// violation at depth"), compiled on the host (user_inv.cpp) from their TLA+
// text into a small register program over the packed state word, and run
// by this interpreter on the host and on the GPU (k_user_check, tlcgpu.hip).
//
// A user invariant is a state predicate over the spec's variables
// (compaction.tla:57-70) and constants (:10-18, :38-54): the compiler resolves
// every composite value (message records, sequences, the ledger function,
// the cursor and phaseOneResult records, sets) statically, so the program
// only moves 64-bit integers: field reads of the packed state (model.h
// layout), arithmetic, comparisons, bit operations on the ledgers' position
// masks, and jumps for short-circuit logic, IF, quantifiers and CHOOSE.
// Evaluation errors (out-of-domain application, a field of Nil, an empty
// CHOOSE, ...) end the program with EV_ERROR, as TLC's evaluator would.
#pragma once
#if !defined(__HIPCC_RTC__)
#include "model.h"
#endif

namespace tlcg {

constexpr int UI_MAXINS = 4096;  // instructions over all user invariants of a model (32 KB, device memory)
constexpr int UI_MAXREG = 64;    // registers (int64) of the program
constexpr int UI_MAXSET = 64;    // KeySet / ValueSet elements (incl. NullKey / NullValue)
// (INV_USER, model.h: tlcg_model.invariants INV_USER + k = the k-th user invariant)

// model values as integers (compactorState's phases and Nil); disjoint from
// every integer the spec's variables take, and compared only with each other
enum { UV_NIL = -1000, UV_PHASE0 = -999 /* + phase (compaction.tla:39-44) */ };

enum UOp : uint8_t {
  U_LDI,     // r[a] = imm
  U_MOV,     // r[a] = r[b]
  U_LEN,     // r[a] = Len(messages)
  U_MKEY,    // r[a] = messages[r[b]].key (the key's value; r[b] in 1..N)
  U_MVAL,    // r[a] = messages[r[b]].value
  U_PHASE,   // r[a] = compactorState (UV_PHASE0 + phase)
  U_P1R,     // r[a] = phaseOneResult.readPosition, 0 = Nil
  U_HZ,      // r[a] = compactionHorizon
  U_CTX,     // r[a] = compactedTopicContext
  U_CRASH,   // r[a] = crashTimes
  U_CURP,    // r[a] = cursor # Nil
  U_CURH,    // r[a] = cursor.compactionHorizon (cursor not Nil)
  U_CURC,    // r[a] = cursor.compactedTopicContext
  U_LEDP,    // r[a] = compactedLedgers[r[b]] # Nil (r[b] in 1..C)
  U_LEDM,    // r[a] = position mask of compactedLedgers[r[b]] (bit p-1: messages[p])
  U_LFK,     // r[a] = max i in 1..r[c] with messages[i].key = r[b], 0 if none
  U_ADD, U_SUB, U_MUL,
  U_DIV,     // r[a] = r[b] \div r[c] (floor; r[c] > 0 checked by the program)
  U_MOD,     // r[a] = r[b] % r[c] (0..r[c]-1)
  U_NEG,     // r[a] = -r[b]
  U_EQ, U_NE, U_LT, U_LE,  // r[a] = r[b] op r[c] (0/1)
  U_NOT,     // r[a] = !r[b]
  U_AND, U_OR,  // r[a] = r[b] & r[c], r[b] | r[c] (on 0/1)
  U_ADDI,    // r[a] = r[b] + imm
  U_BIT,     // r[a] = (r[b] >> (r[c] - 1)) & 1 (r[c] in 1..63)
  U_POPC,    // r[a] = popcount(r[b])
  U_NTH,     // r[a] = position of the r[c]-th set bit of r[b] (1-based), 0 if fewer
  U_MASK,    // r[a] = (1 << r[b]) - 1 (r[b] in 0..62)
  U_KIN,     // r[a] = r[b] \in KeySet (imm 0) / ValueSet (imm 1)
  U_KAT,     // r[a] = the r[b]-th (0-based) element of KeySet in ascending order (imm 0), ValueSet (imm 1)
  U_JMP,     // pc = imm
  U_JZ,      // if (!r[a]) pc = imm
  U_JNZ,     // if (r[a]) pc = imm
  U_ERR,     // evaluation error
  U_RET,     // return r[a] ? TRUE : FALSE
};
// Two-state programs (an action property's A \/ UNCHANGED v,
// compile_action_property): a state-reading op (U_LEN .. U_LFK) with imm = 1
// reads the successor state of the step (x'), and one op more compares the
// two states.  Only the two-view interpreter eval_user2_v runs such programs;
// the one-view interpreter, the generated device code and the read analysis
// never see one.
enum UOp2 : uint8_t {
  U2_MSAME = 64,  // r[a] = messages[p] is the same message in both states, for every bit p-1 of r[b]
};

struct UInsn {
  uint8_t op, a, b, c;
  int32_t imm;
};

struct UserProg {
  int32_t n_user;                 // user invariants
  int32_t n_ins;
  int32_t n_con;                  // state constraints (cfg CONSTRAINT): entries n_user .. n_user + n_con - 1
  int32_t entry[16];              // first instruction of user invariant k, then of each constraint
  int32_t nk, nv;                 // |KeySet|, |ValueSet|
  int32_t keyval[UI_MAXSET];      // key index -> value (model.h: index 0 = NullKey = 0)
  int32_t valval[UI_MAXSET];      // value index -> value
  int32_t keysorted[UI_MAXSET];   // KeySet in ascending order
  int32_t valsorted[UI_MAXSET];   // ValueSet in ascending order
  UInsn ins[UI_MAXINS];
};

// (+, -, * and unary - past TLC's 32-bit integers: model.h ui_overflows)
// Programs run at most UI_MAXLOOP taken backward jumps (quantifier / CHOOSE
// iterations; forward code runs each instruction at most once), then fail as
// an evaluation error.  The generated device code (user_inv.cpp) counts the
// same way, so both give the same result on every state.
constexpr int UI_MAXLOOP = 1 << 20;

// Runs user invariant k on the state behind view v (model.h UVWord, or an
// on-chip engine's view): EV_TRUE / EV_FALSE / EV_ERROR.
template <class V>
TLCG_HD int eval_user_v(const UserProg& P, int k, const V& v) {
  long long r[UI_MAXREG];
  int pc = P.entry[k];
  int loops = 0;
  for (;;) {
    const int at = pc;
    const UInsn in = P.ins[pc++];
    switch (in.op) {
      case U_LDI: r[in.a] = in.imm; break;
      case U_MOV: r[in.a] = r[in.b]; break;
      case U_LEN: r[in.a] = v.len(); break;
      case U_MKEY: r[in.a] = P.keyval[v.key((int)r[in.b]) & (UI_MAXSET - 1)]; break;
      case U_MVAL: r[in.a] = P.valval[v.val((int)r[in.b]) & (UI_MAXSET - 1)]; break;
      case U_PHASE: r[in.a] = UV_PHASE0 + v.phase(); break;
      case U_P1R: r[in.a] = v.p1r(); break;
      case U_HZ: r[in.a] = v.hz(); break;
      case U_CTX: r[in.a] = v.ctx(); break;
      case U_CRASH: r[in.a] = v.crash(); break;
      case U_CURP: r[in.a] = v.curp(); break;
      case U_CURH: r[in.a] = v.curh(); break;
      case U_CURC: r[in.a] = v.curc(); break;
      case U_LEDP: r[in.a] = v.ledp((int)r[in.b]); break;
      case U_LEDM: r[in.a] = (long long)v.ledm((int)r[in.b]); break;
      case U_LFK: {
        long long best = 0;
        for (int i = 1; i <= (int)r[in.c] && i <= v.L.N; ++i)
          if (P.keyval[v.key(i) & (UI_MAXSET - 1)] == r[in.b]) best = i;
        r[in.a] = best;
        break;
      }
      case U_ADD: r[in.a] = r[in.b] + r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_SUB: r[in.a] = r[in.b] - r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_MUL: r[in.a] = r[in.b] * r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_DIV: {
        const long long q = r[in.b] / r[in.c];
        r[in.a] = (r[in.b] % r[in.c] != 0 && ((r[in.b] < 0) != (r[in.c] < 0))) ? q - 1 : q;
        break;
      }
      case U_MOD: {
        const long long m = r[in.b] % r[in.c];
        r[in.a] = m < 0 ? m + r[in.c] : m;
        break;
      }
      case U_NEG: r[in.a] = -r[in.b]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_EQ: r[in.a] = r[in.b] == r[in.c]; break;
      case U_NE: r[in.a] = r[in.b] != r[in.c]; break;
      case U_LT: r[in.a] = r[in.b] < r[in.c]; break;
      case U_LE: r[in.a] = r[in.b] <= r[in.c]; break;
      case U_NOT: r[in.a] = !r[in.b]; break;
      case U_AND: r[in.a] = r[in.b] & r[in.c]; break;
      case U_OR: r[in.a] = r[in.b] | r[in.c]; break;
      case U_ADDI: r[in.a] = r[in.b] + in.imm; break;
      case U_BIT: r[in.a] = (r[in.c] >= 1 && r[in.c] <= 63) ? (r[in.b] >> (r[in.c] - 1)) & 1 : 0; break;
      case U_POPC: r[in.a] = popcount64((u64)r[in.b]); break;
      case U_NTH: r[in.a] = ui_nth((u64)r[in.b], r[in.c]); break;
      case U_MASK: r[in.a] = (long long)((1ull << (r[in.b] & 63)) - 1); break;
      case U_KIN: {
        const int n = in.imm ? P.nv : P.nk;
        const int32_t* t = in.imm ? P.valsorted : P.keysorted;
        long long f = 0;
        for (int i = 0; i < n && i < UI_MAXSET; ++i) f |= t[i] == r[in.b];
        r[in.a] = f;
        break;
      }
      case U_KAT: {
        const int i = (int)r[in.b] & (UI_MAXSET - 1);
        r[in.a] = in.imm ? P.valsorted[i] : P.keysorted[i];
        break;
      }
      case U_JMP: pc = in.imm; break;
      case U_JZ: if (!r[in.a]) pc = in.imm; break;
      case U_JNZ: if (r[in.a]) pc = in.imm; break;
      case U_ERR: return EV_ERROR;
      case U_RET: return r[in.a] ? EV_TRUE : EV_FALSE;
      default: return EV_ERROR;
    }
    if (pc <= at && ++loops > UI_MAXLOOP) return EV_ERROR;  // a taken backward jump
  }
}

// Runs entry k of a two-state program on the step v -> vn (the views of the
// state and of its successor): EV_TRUE / EV_FALSE / EV_ERROR.  The one-state
// interpreter above with the state-reading ops choosing their view by imm.
template <class V>
TLCG_HD int eval_user2_v(const UserProg& P, int k, const V& v, const V& vn) {
  long long r[UI_MAXREG];
  int pc = P.entry[k];
  int loops = 0;
  for (;;) {
    const int at = pc;
    const UInsn in = P.ins[pc++];
    const V& w = in.op >= U_LEN && in.op <= U_LFK && in.imm ? vn : v;
    switch (in.op) {
      case U_LDI: r[in.a] = in.imm; break;
      case U_MOV: r[in.a] = r[in.b]; break;
      case U_LEN: r[in.a] = w.len(); break;
      case U_MKEY: r[in.a] = P.keyval[w.key((int)r[in.b]) & (UI_MAXSET - 1)]; break;
      case U_MVAL: r[in.a] = P.valval[w.val((int)r[in.b]) & (UI_MAXSET - 1)]; break;
      case U_PHASE: r[in.a] = UV_PHASE0 + w.phase(); break;
      case U_P1R: r[in.a] = w.p1r(); break;
      case U_HZ: r[in.a] = w.hz(); break;
      case U_CTX: r[in.a] = w.ctx(); break;
      case U_CRASH: r[in.a] = w.crash(); break;
      case U_CURP: r[in.a] = w.curp(); break;
      case U_CURH: r[in.a] = w.curh(); break;
      case U_CURC: r[in.a] = w.curc(); break;
      case U_LEDP: r[in.a] = w.ledp((int)r[in.b]); break;
      case U_LEDM: r[in.a] = (long long)w.ledm((int)r[in.b]); break;
      case U_LFK: {
        long long best = 0;
        for (int i = 1; i <= (int)r[in.c] && i <= w.L.N; ++i)
          if (P.keyval[w.key(i) & (UI_MAXSET - 1)] == r[in.b]) best = i;
        r[in.a] = best;
        break;
      }
      case U_ADD: r[in.a] = r[in.b] + r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_SUB: r[in.a] = r[in.b] - r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_MUL: r[in.a] = r[in.b] * r[in.c]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_DIV: {
        const long long q = r[in.b] / r[in.c];
        r[in.a] = (r[in.b] % r[in.c] != 0 && ((r[in.b] < 0) != (r[in.c] < 0))) ? q - 1 : q;
        break;
      }
      case U_MOD: {
        const long long m = r[in.b] % r[in.c];
        r[in.a] = m < 0 ? m + r[in.c] : m;
        break;
      }
      case U_NEG: r[in.a] = -r[in.b]; if (ui_overflows(r[in.a])) return EV_ERROR; break;
      case U_EQ: r[in.a] = r[in.b] == r[in.c]; break;
      case U_NE: r[in.a] = r[in.b] != r[in.c]; break;
      case U_LT: r[in.a] = r[in.b] < r[in.c]; break;
      case U_LE: r[in.a] = r[in.b] <= r[in.c]; break;
      case U_NOT: r[in.a] = !r[in.b]; break;
      case U_AND: r[in.a] = r[in.b] & r[in.c]; break;
      case U_OR: r[in.a] = r[in.b] | r[in.c]; break;
      case U_ADDI: r[in.a] = r[in.b] + in.imm; break;
      case U_BIT: r[in.a] = (r[in.c] >= 1 && r[in.c] <= 63) ? (r[in.b] >> (r[in.c] - 1)) & 1 : 0; break;
      case U_POPC: r[in.a] = popcount64((u64)r[in.b]); break;
      case U_NTH: r[in.a] = ui_nth((u64)r[in.b], r[in.c]); break;
      case U_MASK: r[in.a] = (long long)((1ull << (r[in.b] & 63)) - 1); break;
      case U_KIN: {
        const int n = in.imm ? P.nv : P.nk;
        const int32_t* t = in.imm ? P.valsorted : P.keysorted;
        long long f = 0;
        for (int i = 0; i < n && i < UI_MAXSET; ++i) f |= t[i] == r[in.b];
        r[in.a] = f;
        break;
      }
      case U_KAT: {
        const int i = (int)r[in.b] & (UI_MAXSET - 1);
        r[in.a] = in.imm ? P.valsorted[i] : P.keysorted[i];
        break;
      }
      case U_JMP: pc = in.imm; break;
      case U_JZ: if (!r[in.a]) pc = in.imm; break;
      case U_JNZ: if (r[in.a]) pc = in.imm; break;
      case U_ERR: return EV_ERROR;
      case U_RET: return r[in.a] ? EV_TRUE : EV_FALSE;
      case U2_MSAME: {
        long long same = 1;
        for (int i = 1; i <= v.L.N && i <= 63; ++i)
          if (((u64)r[in.b] >> (i - 1)) & 1) same &= v.key(i) == vn.key(i) && v.val(i) == vn.val(i);
        r[in.a] = same;
        break;
      }
      default: return EV_ERROR;
    }
    if (pc <= at && ++loops > UI_MAXLOOP) return EV_ERROR;  // a taken backward jump
  }
}

// Runs user invariant k on state s: EV_TRUE / EV_FALSE / EV_ERROR.
template <typename W>
TLCG_HD int eval_user(const Layout& L, const UserProg& P, int k, W s) {
  return eval_user_v(P, k, UVWord<W>{L, s});
}

// Runs entry k on the step s -> t.
template <typename W>
TLCG_HD int eval_user2(const Layout& L, const UserProg& P, int k, W s, W t) {
  return eval_user2_v(P, k, UVWord<W>{L, s}, UVWord<W>{L, t});
}

// Every invariant of the cfg in its order -- the spec's own (model.h) and the
// user's: -1 if all hold, else (index << 1) | is_error (as check_invariants).
template <typename W>
TLCG_HD int check_invariants_all(const Layout& L, const UserProg& P, W s) {
  for (int q = 0; q < L.n_inv; ++q) {
    const int kind = L.inv[q];
    const int r = kind >= INV_USER ? eval_user(L, P, kind - INV_USER, s) : eval_invariant(L, kind, s);
    if (r != EV_TRUE) return (q << 1) | (r == EV_ERROR ? 1 : 0);
  }
  return -1;
}

// The conjunction of the model's state constraints on the state behind view
// v, left to right (TLC's isInModel): EV_TRUE in the model, EV_FALSE discarded,
// EV_ERROR with *which = the failing constraint.
template <class V>
TLCG_HD int eval_constraints_v(const UserProg& P, const V& v, int* which) {
  for (int k = 0; k < P.n_con; ++k) {
    const int r = eval_user_v(P, P.n_user + k, v);
    if (r != EV_TRUE) {
      *which = k;
      return r;
    }
  }
  return EV_TRUE;
}

}  // namespace tlcg
