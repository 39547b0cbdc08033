"""A test-side reference for action properties [][A]_v, independent of the
product: A is rewritten to a state predicate over two copies of the variables
(x' -> x__next, UNCHANGED e -> the conjunction of x__next = x) and evaluated by
the oracle's TLA+ evaluator (oracle/tla_eval.py, unchanged) in the state's
environment extended by the successor's variables under the __next names; the
subscript's v' = v is applied on top.  Also the plain reference of the step
pass on an explicit graph (counts and the reported step)."""
import re

import tla_eval
from user_inv_cases import oracle_model

VARIABLES = ("messages", "compactedLedgers", "cursor", "compactorState", "phaseOneResult", "compactionHorizon",
             "compactedTopicContext", "crashTimes", "consumeTimes")
TUPLES = {"bookieVars": ("messages", "compactedLedgers", "cursor"),
          "compactorVars": ("phaseOneResult", "compactorState", "compactionHorizon", "compactedTopicContext"),
          "otherVars": ("crashTimes", "consumeTimes"), "vars": VARIABLES}
TRUE, FALSE, ERROR = 0, 1, 2


def flatten(text):
    """the variables of a subscript / an UNCHANGED operand, in declaration order"""
    names = set()
    for w in re.findall(r"[A-Za-z_]\w*", text):
        if w in TUPLES:
            names.update(TUPLES[w])
        elif w in VARIABLES:
            names.add(w)
        else:
            raise ValueError(f"{w} is not a variable")
    return tuple(v for v in VARIABLES if v in names)


def rewrite(text):
    """x' -> x__next; UNCHANGED <<..>> / UNCHANGED name -> (x__next = x /\\ ...)"""
    def unchanged(m):
        vs = flatten(m.group(1))
        return "(" + " /\\ ".join(f"{v}__next = {v}" for v in vs) + ")" if vs else "TRUE"
    text = re.sub(r"UNCHANGED\s*(<<[^<>]*(?:<<[^<>]*>>[^<>]*)*>>|[A-Za-z_]\w*)", unchanged, text)
    return re.sub(r"([A-Za-z_]\w*)'", r"\1__next", text)


class ActionRef:
    """[][A]_v over an oracle model: verdict(s, t) of one step"""

    def __init__(self, model, a_text, subscript="vars", defs=None):
        d = {k: rewrite(v) for k, v in (defs or {}).items() if k not in TUPLES}
        d["A__"] = rewrite(a_text)
        self.om = oracle_model(model, user_defs=d)
        self.ev = self.om.user
        self.sub = [VARIABLES.index(v) for v in flatten(subscript)]

    def verdict(self, s, t):
        env = self.ev.state_env(s)
        nxt = self.ev.state_env(t)
        for v in VARIABLES:
            env[v + "__next"] = nxt[v]
        _, e = self.ev.body("A__")
        try:
            r = self.ev.ev(e, dict(state=env, env={}))
        except tla_eval.EvalError:
            return ERROR
        if not isinstance(r, bool):
            return ERROR
        if r:
            return TRUE
        return TRUE if all(s[i] == t[i] for i in self.sub) else FALSE


def model_steps(m, pairs):
    """[(word s, word t, oracle s, oracle t, level of s, state index)] for every
    step of the reachable graph behind pairs (user_inv_cases.paired_states), in
    BFS order and, per state, in move order; and the level of every state"""
    import tlcgpu
    om = oracle_model(m, user_defs={})
    level = {}  # (counted from 1, as TLC's depth and the product's step_depth: Init is level 1)
    n_init = tlcgpu.init_count(m)
    for i, (w, _) in enumerate(pairs):
        if i < n_init:
            level[w] = 1
    out = []
    for i, (w, o) in enumerate(pairs):
        ps = tlcgpu.host_successors(m, w)
        os_ = list(om.successors(o))
        assert len(ps) == len(os_)
        for (_, t), (_, u) in zip(ps, os_):
            level.setdefault(t, level[w] + 1)
            if u != o:
                assert t != w
                out.append((w, t, o, u, level[w], i))
    return out, level


def summary(verdicts, steps):
    """counts and the reported step of a model's graph by the rule of the pass:
    the shallowest level with a flagged state, its least packed flagged state,
    that state's lowest flagged move.  steps as model_steps gives them"""
    viol = sum(v == FALSE for v in verdicts)
    errs = sum(v == ERROR for v in verdicts)
    flagged = [(lv, w, j) for j, ((w, _, _, _, lv, _), v) in enumerate(zip(steps, verdicts)) if v != TRUE]
    rep = None
    if flagged:
        lv, w, j = min(flagged)  # (per state the steps are in move order, so the least j is the lowest move)
        rep = dict(level=lv, source=w, target=steps[j][1], verdict=verdicts[j])
    return dict(steps=len(steps), violating=viol, erroring=errs, reported=rep)


def graph_ref(row, col, verdict, n_init, word_of):
    """the step pass on an explicit CSR graph: reachable nodes, steps, violating
    and erroring steps, and the reported (level, source word, target word, edge
    ordinal, verdict), None when it holds"""
    level = {v: 1 for v in range(n_init)}
    queue = list(range(n_init))
    for v in queue:
        for e in range(row[v], row[v + 1]):
            if col[e] not in level:
                level[col[e]] = level[v] + 1
                queue.append(col[e])
    steps = [(level[v], word_of(v), e - row[v], e) for v in queue for e in range(row[v], row[v + 1]) if col[e] != v]
    bad = [s for s in steps if verdict[s[3]]]
    rep = None
    if bad:
        lv, w, k, e = min(bad)
        rep = (lv, w, word_of(col[e]), k, verdict[e])
    return dict(reachable=len(queue), depth=max(level.values()) if level else 0, steps=len(steps),
                violating=sum(verdict[s[3]] == 1 for s in steps), erroring=sum(verdict[s[3]] == 2 for s in steps),
                reported=rep)
