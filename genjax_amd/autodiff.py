"""Reverse-mode differentiation of the site-program IR.

`grad(out, wrt)` returns d out / d w for each Expr w in `wrt` as new expressions in the same
graph (the tracer's operators build them), so a gradient costs no extra launch: it is more
straight-line code in the program that needed it.  This is what `jax.grad(assess)` is to the
reference's HMC (src/genjax/_src/inference/requests/hmc.py:69-97).

The `wrt` nodes are treated as independent inputs: propagation stops at them.  Integer / boolean
ops, comparisons and table indices carry no gradient.  Density ops differentiate in closed form:
  L_NORMAL(x; m, s):  z = x/s - m/s;  d/dx = -z/s,  d/dm = z/s,  d/ds = (z*z - 1)/s
(the derivative of TFP's  -0.5*squared_difference(x/s, m/s) - log s - 0.5*log(2 pi)).

Where a derivative is a convention it is jax.grad's: abs'(+-0) = 0, maximum / minimum at a tie give each argument half,
d pow(x, y) / d y = 0 at x = 0 < y.  One deliberate difference: L_FLIP forms only the term of the observed outcome, so its
gradient is finite wherever its density is (jax.grad gives 0 * inf = NaN at p = 1 observed True); DESIGN.md section 3.
"""
from __future__ import annotations

from . import tracer as T
from .tracer import Expr
from .engine import new_cache as _new_program_cache


class NotDifferentiable(NotImplementedError):
    pass


def grad(out: Expr, wrt: list) -> list:
    g = T.current_graph()
    wrt_idx = {w.node.idx for w in wrt}
    # a loop-carried SUM whose loop accumulated its own derivatives (static._vector_site_loop: the score of a long
    # vector-valued site, d / d w summed over the elements in the same loop): var idx -> [(w node, derivative node)]
    custom = g.__dict__.get("_custom_grads", {})
    # nodes that depend on a wrt node (forward reachability), restricted to ancestors of `out`
    anc = set()
    stack = [out.node]
    while stack:
        n = stack.pop()
        if n.idx in anc:
            continue
        anc.add(n.idx)
        if n.idx in wrt_idx:
            continue
        stack.extend(a for a in n.args if a is not None)
        if n.op == "LOOPVAR" and n.idx in custom:
            stack.extend(wn for wn, _ in custom[n.idx])
    dep = set(wrt_idx)
    order = sorted(anc)
    by_idx = {i: g.nodes[i] for i in order}
    for i in order:                              # args precede their users in the node list
        n = by_idx[i]
        if i not in dep and any(a is not None and a.idx in dep for a in n.args):
            dep.add(i)
        if i not in dep and n.op == "LOOPVAR" and any(wn.idx in dep for wn, _ in custom.get(i, ())):
            dep.add(i)
    adj = {out.node.idx: T.lift(1.0)}

    def push(node, contribution):
        if node is None or node.idx not in dep:
            return
        cur = adj.get(node.idx)
        adj[node.idx] = contribution if cur is None else cur + contribution

    for i in reversed(order):
        if i not in dep or i in wrt_idx:
            continue
        a_ = adj.get(i)
        if a_ is None:
            continue
        n = by_idx[i]
        if n.op == "LOOPVAR":
            push(n.args[0], a_)                    # the initial value
            for wn, gv in custom.get(i, ()):
                push(wn, a_ * Expr(gv))            # d (sum over the loop) / d w, accumulated by the loop itself
            continue
        _rule(n, a_, push)
    zero = T.lift(0.0)
    return [adj.get(w.node.idx, zero) for w in wrt]


# ops with a derivative rule in _rule (LOOPVAR: in grad itself) ...
DIFFERENTIABLE = frozenset({
    "MOV", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "EXP", "LOG", "LOG1P", "SQRT", "SQUARE", "RECIP", "SIN", "COS", "TANH",
    "SIGMOID", "SOFTPLUS", "POW", "MIN", "MAX", "SEL", "L_NORMAL", "L_BERNL", "L_FLIP", "L_UNIFORM", "LOOPVAR"})
# ... and the ops through which no gradient flows, by NAME: roundings, conversions, loads, comparisons, logic and integer
# arithmetic.  Every other op (LGAMMA, L_BETA, the samplers, ...) raises NotDifferentiable.
ZERO_GRADIENT = frozenset({
    "FLOOR", "CEIL", "ROUND", "I2F", "F2I", "LDTAB", "LDIN", "LDINX", "UNI", "CONST", "LDIDX", "LDT",
    "FLT", "FLE", "FGT", "FGE", "FEQ", "FNE", "IEQ", "INE", "ILT", "ILE", "IGT", "IGE",
    "AND", "OR", "NOT", "XOR", "IADD", "ISUB", "IMUL", "INEG"})


def _rule(n, a, push):
    op = n.op
    E = lambda node: Expr(node)
    if op in ("MOV",):
        push(n.args[0], a)
    elif op == "ADD":
        push(n.args[0], a); push(n.args[1], a)
    elif op == "SUB":
        push(n.args[0], a); push(n.args[1], -a)
    elif op == "MUL":
        push(n.args[0], a * E(n.args[1])); push(n.args[1], a * E(n.args[0]))
    elif op == "DIV":
        x, y = E(n.args[0]), E(n.args[1])
        push(n.args[0], a / y); push(n.args[1], -(a * E(n)) / y)
    elif op == "NEG":
        push(n.args[0], -a)
    elif op == "ABS":                  # a * sign(x): 0 at +0 and -0, NaN at NaN (jax.grad's rule)
        x = E(n.args[0])
        push(n.args[0], T.where(x > 0.0, a, T.where(x < 0.0, -a, a * (x * 0.0))))
    elif op == "EXP":
        push(n.args[0], a * E(n))
    elif op == "LOG":
        push(n.args[0], a / E(n.args[0]))
    elif op == "LOG1P":
        push(n.args[0], a / (E(n.args[0]) + 1.0))
    elif op == "SQRT":
        push(n.args[0], a / (E(n) * 2.0))
    elif op == "SQUARE":
        push(n.args[0], a * (E(n.args[0]) * 2.0))
    elif op == "RECIP":
        push(n.args[0], -(a * E(n) * E(n)))
    elif op == "SIN":
        push(n.args[0], a * T.unary("COS")(E(n.args[0])))
    elif op == "COS":
        push(n.args[0], -(a * T.unary("SIN")(E(n.args[0]))))
    elif op == "TANH":
        push(n.args[0], a * (1.0 - E(n) * E(n)))
    elif op == "SIGMOID":
        push(n.args[0], a * (E(n) * (1.0 - E(n))))
    elif op == "SOFTPLUS":
        push(n.args[0], a * T.unary("SIGMOID")(E(n.args[0])))
    elif op == "POW":
        x, y = E(n.args[0]), E(n.args[1])
        push(n.args[0], a * (y * T.power(x, y - 1.0)))
        # d/dy = x^y log x, with log(0) replaced by log(1): 0 at x = 0, y > 0 where the limit is 0 (jax's replace_zero)
        push(n.args[1], a * (E(n) * T.unary("LOG")(T.where(x == 0.0, 1.0, x))))
    elif op in ("MIN", "MAX"):         # at an exact tie each argument gets half the adjoint (jax's balanced rule)
        x, y = E(n.args[0]), E(n.args[1])
        first = (x < y) if op == "MIN" else (x > y)
        tie, half = x == y, a * 0.5
        push(n.args[0], T.where(first, a, T.where(tie, half, 0.0)))
        push(n.args[1], T.where(first, 0.0, T.where(tie, half, a)))
    elif op == "SEL":
        c, x, y = n.args
        push(x, T.where(E(c), a, 0.0)); push(y, T.where(E(c), 0.0, a))
    elif op == "L_NORMAL":
        x, m, s = (E(v) for v in n.args)
        z = x / s - m / s
        push(n.args[0], -(a * (z / s)))
        push(n.args[1], a * (z / s))
        push(n.args[2], a * ((z * z - 1.0) / s))
    elif op == "L_BERNL":              # x*l - softplus(l):  d/dl = x - sigmoid(l)
        x, l = n.args
        push(l, a * (T.as_float(E(x)) - T.unary("SIGMOID")(E(l))))
    elif op == "L_FLIP":               # x log p + (1-x) log(1-p): only the live term is formed (at p = 1, x = True the
        x, p = n.args                  # other one is 0/0), so the gradient is finite wherever the density is
        pf = E(p)
        push(p, T.where(E(x), a / pf, -(a / (1.0 - pf))))
    elif op == "L_UNIFORM":
        x, lo, hi = (E(v) for v in n.args)
        inside = T.where((x >= lo), 1.0, 0.0) * T.where((x <= hi), 1.0, 0.0)
        w = hi - lo
        push(n.args[1], a * (inside / w)); push(n.args[2], -(a * (inside / w)))
    elif op in ZERO_GRADIENT:
        return                          # piecewise constant / not a float function of its inputs
    else:
        raise NotDifferentiable(f"no derivative rule for {op}")


# ---------------------------------------------------------------------------
# value_and_grad of a plain numeric function (the `jax.value_and_grad` of this stack): one launch
# ---------------------------------------------------------------------------
_VG_CACHE = _new_program_cache()


def value_and_grad(fn):
    """`value_and_grad(fn)(*xs)`: xs are float tensors of one common batch shape; returns
    (fn(*xs), (d fn / d x_k for each k)) computed per element in ONE launch.  Every result is a float32 tensor of the
    batch shape on the backend's device, a gradient that folds to a constant (d (a + b) / d b) included."""
    def run(*xs):
        import torch
        from . import _lib
        from .engine import Compiled, Flat, leaf_spec, resolve, traced
        from .static import _fnkey
        flat = Flat()
        tree = flat.add(tuple(xs))
        batch = tuple(xs[0].shape)
        specs = tuple(leaf_spec(v, batch) for v in flat.leaves)
        ck = (_fnkey(fn), tree, specs)
        ent = _VG_CACHE.get(ck)
        if ent is None:
            with traced(specs, len(batch)) as p:
                ins = [T.as_float(s.value) for s in p.syms]
                out = T.as_float(fn(*ins))
                gs = grad(out, ins)
                oo = p.tr.emit_output(out)
                go = [p.tr.emit_output(g + 0.0) for g in gs]
            ent = (Compiled(p.tr), oo, go)
            _VG_CACHE[ck] = ent
        comp, oo, go = ent
        outs = comp.run(flat.leaves, batch, None)
        dev = _lib.get().device

        def tensor(v):
            if isinstance(v, torch.Tensor):
                return v
            return torch.full(batch, float(v), dtype=torch.float32, device=dev)
        return tensor(resolve(oo, outs, flat.leaves)), tuple(tensor(resolve(g, outs, flat.leaves)) for g in go)
    return run
