"""A test-side reference for state constraints (a cfg's CONSTRAINT section),
independent of the product: a plain level-synchronous BFS in TLC's order over
the oracle's successors (oracle/oracle_py.py), with the constraints and the user
invariants evaluated by the oracle's TLA+ evaluator (oracle/tla_eval.py) and the
built-in invariants by the oracle's own.

The rules, for every successor t of a queued state, in order:
  1. t counts as generated whether or not it satisfies the constraints;
  2. any successor spares its parent the deadlock;
  3. t in the model and already known: nothing more;
  4. t not known, or outside the model: the constraints were evaluated first
     (an evaluation error there is the error), then every invariant of the cfg;
  5. only a state inside the model is distinct, stored, queued and expanded.
Initial states alike.  Like the product's level-synchronous engine the search
finishes the level on which the first error (in TLC's order) lies: `generated`
covers the whole expansion, the level is filtered and counted."""
import oracle_py
import tla_eval
from user_inv_cases import oracle_model

TRUE, FALSE, ERROR = 0, 1, 2


class ConstraintRef:
    def __init__(self, model):
        """model: tlcgpu.Model with .constraints (names of .user_defs)"""
        self.m = model
        self.om = oracle_model(model)
        self.names = list(model.constraints or ())

    def verdict(self, s):
        """(TRUE / FALSE / ERROR of the conjunction, the constraint that decided it)"""
        for nm in self.names:
            try:
                r = self.om.user.holds(nm, s)
            except tla_eval.EvalError:
                return ERROR, nm
            if not r:
                return FALSE, nm
        return TRUE, None

    def bad(self, s):
        for name in self.om.invariants:
            try:
                if not self.om.inv(name, s):
                    return ("invariant", name)
            except oracle_py.EvalError:
                return ("invariant_error", name)
        return None

    def run(self):
        om = self.om
        states, parent, seen = [], [], {}
        levels, generated = [], 0
        first = None       # the first error in TLC's order: dict(result, name, trace)
        level_errors = []  # every error of the level the search stops on: (result, name)
        discarded = 0
        raw_levels = []    # per level, the new states the constraints were evaluated on (kept or not)

        def trace(k, extra=None):
            out = []
            while k is not None and k >= 0:
                out.append((parent[k][1], states[k]))
                k = parent[k][0]
            out.reverse()
            if extra:
                out.append(extra)
            return out

        def error(result, name, tr):
            nonlocal first
            level_errors.append((result, name))
            if first is None:
                first = dict(result=result, name=name, trace=tr)

        def visit(t, par, act, checked):
            """rules 3-5 for one generated state; `checked`: the states of this level
            already examined outside the model (their verdicts are known)"""
            nonlocal discarded
            if t in seen:
                return
            if t not in checked:
                raw_levels[-1] += 1
            v, nm = self.verdict(t)
            tr = lambda: trace(par, (act, t))  # noqa: E731
            if v == ERROR:
                if t not in checked:
                    error("constraint_error", nm, tr())
                    checked.add(t)
                    discarded += 1  # (not in the model either)
                return
            if t not in checked or v == TRUE:
                b = self.bad(t)
                if b:
                    error(b[0], b[1], tr())
            if v == TRUE:
                checked.add(t)
                seen[t] = len(states)
                states.append(t)
                parent.append((par, act))
            elif t not in checked:
                checked.add(t)
                discarded += 1

        checked = set()
        raw_levels.append(0)
        for t in om.inits():
            generated += 1
            visit(t, -1, "Init", checked)
        if states:
            levels.append(len(states))
        head = 0
        while first is None and head < len(states):
            end = len(states)
            checked = set()
            raw_levels.append(0)
            for p in range(head, end):
                n = 0
                try:
                    for a, t in om.successors(states[p]):
                        generated += 1
                        n += 1
                        visit(t, p, oracle_py.ACTIONS[a], checked)
                except oracle_py.EvalError:
                    error("action_error", None, trace(p))
                    for a, t in om.tail_actions(states[p]):
                        generated += 1
                        n += 1
                        visit(t, p, oracle_py.ACTIONS[a], checked)
                if n == 0 and om.deadlock:
                    error("deadlock", None, trace(p))
            head = end
            if len(states) > end:
                levels.append(len(states) - end)
        return dict(result=first["result"] if first else "ok", name=first["name"] if first else None,
                    trace=first["trace"] if first else [], generated=generated, distinct=len(states),
                    depth=len(levels), levels=levels, states=list(states), discarded=discarded,
                    raw_levels=raw_levels, level_errors=sorted(set(level_errors), key=str))
