"""Shared drivers of tests/test_grad_cpu.py (the C-ABI's CPU mirror) and tests/test_grad_gpu.py (the HIP library, interpreter
and hiprtc-specialised): genjax_amd/autodiff.py held to torch.float64 autograd on the CPU, rule by rule (RULES), pinned at
the edges where a rule's convention decides the result (EDGES), the classification of every op, `value_and_grad` as an API,
and one leapfrog step of HMC through the non-normal densities, unrolled and in loop form, reconstructed from its outputs.

Tolerances.  Nothing here is fixed from what the kernels give.  Every RULES case carries a hand-written derivative that is
evaluated in plain numpy float32 on the same inputs; its worst |g - g64| / (1 + |g64|) against the float64 reference is a
number between two references, and the kernel is allowed 4 times that (the device's elementary functions are a few ulp
where numpy's are at most one, and reverse-mode accumulation adds in another order than the formula), never less than
8 * 2^-23.  The replay follows the FORM the product documents where the form decides the rounding: the normal density is
TFP's x/s - m/s (autodiff.py's docstring), `pow` is exp(y log x) (csrc/gmx_math.h: gmx_powf), the traced compositions of
genjax_amd/numpy.py are what their source says.  The measured replay error of each case is the last column of RULES."""
from __future__ import annotations

import contextlib
import functools
import math
from collections import namedtuple

import numpy as np
import torch

FLOOR = 8.0 * 2.0 ** -23
N_TILE = 1027                  # one 1024 tile and a ragged tail; 4 per thread leaves a remainder in the specialised form
SIZES = [N_TILE, 1]
F = np.float32


# --- inputs ------------------------------------------------------------------------------------------------------------------
def _domain(rng, dom, n):
    if dom == "s":                         # signed
        return (rng.normal(size=n) * 3.0).astype(F)
    if dom == "p":                         # positive, over four decades
        return np.exp(rng.uniform(-6.0, 3.0, size=n)).astype(F)
    if dom == "t":                         # trig arguments: the rule, not float32 argument reduction
        return np.clip(rng.normal(size=n) * 3.0, -8.0, 8.0).astype(F)
    if dom == "q":                         # a probability away from 0 and 1 (the ends are EDGES)
        return rng.uniform(0.01, 0.99, size=n).astype(F)
    raise ValueError(dom)


@functools.lru_cache(maxsize=None)
def inputs(name, n):
    """the case's float32 operands (never modified); n = 1 is the first of the 1027"""
    case = RULE[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + 17)
    out = tuple(_domain(rng, d, N_TILE)[:n].copy() for d in case.doms)
    for a in out:
        a.setflags(write=False)
    return out


# --- numpy float32 helpers of the hand-written derivatives ----------------------------------------------------------------------
def _sig(x):
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, F(1) / (F(1) + e), e / (F(1) + e)).astype(F)


def _softplus(x):
    return (np.maximum(x, F(0)) + np.log1p(np.exp(-np.abs(x)))).astype(F)


_HL2PI = F(0.918938533204672741780329736406)
_ONE = lambda a: np.ones_like(a)          # noqa: E731


def _normal_hand(x, m, s):
    z = x / s - m / s
    return -F(0.5) * (z * z) - (_HL2PI + np.log(s)), -(z / s), z / s, (z * z - F(1)) / s


def _uniform_hand(lo, hi, x=F(0.25)):
    inside = (x >= lo) & (x <= hi)
    w = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(inside, -np.log(w), F(-np.inf)).astype(F)
        g = np.where(inside, F(1) / w, F(0)).astype(F)
    return v, g, -g


BIG_H = 9


def _big_fn(xp, a, b):
    """sum_k e_k e_{k+H}, e_k = exp(c_k a) (b + k): every e_k (and its exp, for the reverse pass) is alive at once"""
    e = [xp.exp(a * (0.05 * (k + 1))) * (b + float(k)) for k in range(2 * BIG_H)]
    out = e[0] * e[BIG_H]
    for k in range(1, BIG_H):
        out = out + e[k] * e[k + BIG_H]
    return out


def _big_hand(a, b):
    c = [F(0.05 * (k + 1)) for k in range(2 * BIG_H)]
    ex = [np.exp(a * c[k]) for k in range(2 * BIG_H)]
    e = [ex[k] * (b + F(k)) for k in range(2 * BIG_H)]
    da = [c[k] * e[k] for k in range(2 * BIG_H)]
    v = sum(e[k] * e[k + BIG_H] for k in range(BIG_H))
    ga = sum(da[k] * e[k + BIG_H] + e[k] * da[k + BIG_H] for k in range(BIG_H))
    gb = sum(ex[k] * e[k + BIG_H] + e[k] * ex[k + BIG_H] for k in range(BIG_H))
    return v, ga, gb


def _fan_fn(xp, a, b):
    t = xp.exp(a * 0.25) + b * b           # used three times
    return t * xp.log(t) + xp.sqrt(t)


def _fan_hand(a, b):
    ea = np.exp(a * F(0.25))
    t = ea + b * b
    dt = np.log(t) + F(1) + F(0.5) / np.sqrt(t)
    return t * np.log(t) + np.sqrt(t), dt * (F(0.25) * ea), dt * (F(2) * b)


def _jnp():
    from genjax_amd import numpy as jnp
    return jnp


def _T():
    from genjax_amd import tracer
    return tracer


def _G():
    import genjax_amd
    return genjax_amd


def _mod_hand(a, b):
    q = np.floor(a / b)
    return a - q * b, _ONE(a), -q


def _clip_hand(a, b):
    lo, hi = b - F(1), b + F(1)
    inside = (a > lo) & (a < hi)
    return np.minimum(np.maximum(a, lo), hi), inside.astype(F), (~inside).astype(F)


def _lae_hand(a, b):
    d = a - b
    return np.maximum(a, b) + np.log1p(np.exp(-np.abs(d))), _sig(d), _sig(-d)


def _pow_hand(a, b):
    la = np.log(a)
    v = np.exp(b * la)
    return v, b * np.exp((b - F(1)) * la), v * la


Case = namedtuple("Case", "name doms fn ref hand ops measured")
# name, domains of the operands, the traced function, the same function on float64 torch tensors, (value, gradients) by hand
# in numpy float32, the ops whose rule the case is there for, and the hand-written replay's own worst deviation from float64
# on the case's 1027 inputs (measured by replay_error; test_replay_errors_are_the_recorded_ones holds the column to it)
RULES = [
    Case("add", "ss", lambda a, b: a + b, lambda a, b: a + b, lambda a, b: (a + b, _ONE(a), _ONE(a)), {"ADD"}, 5.2e-08),
    Case("sub", "ss", lambda a, b: a - b, lambda a, b: a - b, lambda a, b: (a - b, _ONE(a), -_ONE(a)), {"SUB"}, 5.3e-08),
    Case("mul", "ss", lambda a, b: a * b, lambda a, b: a * b, lambda a, b: (a * b, b, a), {"MUL"}, 5.1e-08),
    Case("div", "sp", lambda a, b: a / b, lambda a, b: a / b, lambda a, b: (a / b, F(1) / b, -(a / b) / b), {"DIV"}, 1.0e-07),
    Case("neg", "s", lambda a: -a, lambda a: -a, lambda a: (-a, -_ONE(a)), {"NEG"}, 0.0),
    Case("abs", "s", lambda a: abs(a), lambda a: a.abs(), lambda a: (np.abs(a), np.sign(a)), {"ABS"}, 0.0),
    Case("square", "s", lambda a: _jnp().square(a), lambda a: a * a, lambda a: (a * a, F(2) * a), {"SQUARE"}, 5.5e-08),
    Case("recip", "s", lambda a: _T().unary("RECIP")(a), lambda a: 1.0 / a, lambda a: (F(1) / a, -(F(1) / a) * (F(1) / a)),
         {"RECIP"}, 1.2e-07),
    Case("mov", "s", lambda a: _T().unary("MOV")(a) * 3.0, lambda a: a * 3.0, lambda a: (a * F(3), F(3) * _ONE(a)), {"MOV"}, 5.6e-08),
    Case("exp", "s", lambda a: _jnp().exp(a), torch.exp, lambda a: (np.exp(a), np.exp(a)), {"EXP"}, 1.3e-07),
    Case("log", "p", lambda a: _jnp().log(a), torch.log, lambda a: (np.log(a), F(1) / a), {"LOG"}, 5.5e-08),
    Case("log1p", "p", lambda a: _jnp().log1p(a), torch.log1p, lambda a: (np.log1p(a), F(1) / (a + F(1))), {"LOG1P"}, 4.3e-08),
    Case("sqrt", "p", lambda a: _jnp().sqrt(a), torch.sqrt, lambda a: (np.sqrt(a), F(0.5) / np.sqrt(a)), {"SQRT"}, 7.2e-08),
    Case("sin", "t", lambda a: _jnp().sin(a), torch.sin, lambda a: (np.sin(a), np.cos(a)), {"SIN"}, 3.5e-08),
    Case("cos", "t", lambda a: _jnp().cos(a), torch.cos, lambda a: (np.cos(a), -np.sin(a)), {"COS"}, 3.4e-08),
    Case("tanh", "s", lambda a: _jnp().tanh(a), torch.tanh, lambda a: (np.tanh(a), F(1) - np.tanh(a) * np.tanh(a)), {"TANH"}, 1.4e-07),
    Case("sigmoid", "s", lambda a: _jnp().sigmoid(a), torch.sigmoid, lambda a: (_sig(a), _sig(a) * (F(1) - _sig(a))), {"SIGMOID"}, 7.7e-08),
    Case("softplus", "s", lambda a: _jnp().softplus(a), lambda a: torch.logaddexp(torch.zeros_like(a), a),
         lambda a: (_softplus(a), _sig(a)), {"SOFTPLUS"}, 5.1e-08),
    Case("pow", "ps", lambda a, b: _jnp().power(a, b), torch.pow, _pow_hand, {"POW"}, 2.8e-06),
    Case("pow_negative_constant", "p", lambda a: a ** -2.5, lambda a: a ** -2.5,
         lambda a: (np.exp(F(-2.5) * np.log(a)), F(-2.5) * np.exp(F(-3.5) * np.log(a))), {"POW"}, 1.8e-06),
    Case("pow_two_is_square", "s", lambda a: a ** 2.0, lambda a: a ** 2.0, lambda a: (a * a, F(2) * a), {"SQUARE"}, 5.3e-08),
    Case("pow_half_is_sqrt", "p", lambda a: _jnp().power(a, 0.5), lambda a: a ** 0.5, lambda a: (np.sqrt(a), F(0.5) / np.sqrt(a)),
         {"SQRT"}, 7.6e-08),
    Case("min", "ss", lambda a, b: _jnp().minimum(a, b), torch.minimum,
         lambda a, b: (np.minimum(a, b), (a < b).astype(F), (a >= b).astype(F)), {"MIN"}, 0.0),
    Case("max", "ss", lambda a, b: _jnp().maximum(a, b), torch.maximum,
         lambda a, b: (np.maximum(a, b), (a > b).astype(F), (a <= b).astype(F)), {"MAX"}, 0.0),
    Case("sel", "ss", lambda a, b: _jnp().where(a > 0.5, a * b, a - b), lambda a, b: torch.where(a > 0.5, a * b, a - b),
         lambda a, b: (np.where(a > F(0.5), a * b, a - b), np.where(a > F(0.5), b, F(1)).astype(F),
                       np.where(a > F(0.5), a, F(-1)).astype(F)), {"SEL"}, 5.0e-08),
    Case("normal", "ssp", lambda x, m, s: _G().normal.sym_logpdf(x, (m, s)),
         lambda x, m, s: -0.5 * ((x - m) / s) ** 2 - torch.log(s) - 0.5 * math.log(2.0 * math.pi), _normal_hand, {"L_NORMAL"}, 2.2e-06),
    Case("bernoulli_logits_0", "s", lambda l: _G().bernoulli.sym_logpdf(0, (l,)), lambda l: -torch.logaddexp(torch.zeros_like(l), l),
         lambda l: (-_softplus(l), -_sig(l)), {"L_BERNL"}, 4.9e-08),
    Case("bernoulli_logits_1", "s", lambda l: _G().bernoulli.sym_logpdf(1, (l,)), lambda l: -torch.logaddexp(torch.zeros_like(l), -l),
         lambda l: (-_softplus(-l), F(1) - _sig(l)), {"L_BERNL"}, 8.4e-08),
    Case("flip_true", "q", lambda p: _G().flip.sym_logpdf(True, (p,)), torch.log, lambda p: (np.log(p), F(1) / p), {"L_FLIP"}, 5.3e-08),
    Case("flip_false", "q", lambda p: _G().flip.sym_logpdf(False, (p,)), lambda p: torch.log1p(-p),
         lambda p: (np.log1p(-p), -(F(1) / (F(1) - p))), {"L_FLIP"}, 5.5e-08),
    Case("uniform_bounds", "pp", lambda a, b: _G().uniform.sym_logpdf(0.25, (-a, b)),
         lambda a, b: torch.where(b >= 0.25, -torch.log(b + a), torch.full_like(a, -math.inf)),
         lambda a, b: tuple(np.asarray(x) * s for x, s in zip(_uniform_hand(-a, b), (F(1), F(-1), F(1)))), {"L_UNIFORM", "NEG"}, 5.6e-08),
    Case("clip", "ss", lambda a, b: _jnp().clip(a, b - 1.0, b + 1.0), lambda a, b: torch.minimum(torch.maximum(a, b - 1.0), b + 1.0),
         _clip_hand, {"MIN", "MAX"}, 4.5e-08),
    Case("logaddexp", "ss", lambda a, b: _jnp().logaddexp(a, b), torch.logaddexp, _lae_hand, {"MAX", "ABS", "LOG1P", "EXP"}, 5.9e-08),
    Case("sinh", "s", lambda a: _jnp().sinh(a), torch.sinh,
         lambda a: ((np.exp(a) - np.exp(-a)) * F(0.5), (np.exp(a) + np.exp(-a)) * F(0.5)), {"EXP", "NEG"}, 1.7e-07),
    Case("cosh", "s", lambda a: _jnp().cosh(a), torch.cosh,
         lambda a: ((np.exp(a) + np.exp(-a)) * F(0.5), (np.exp(a) - np.exp(-a)) * F(0.5)), {"EXP", "NEG"}, 1.6e-07),
    Case("tan", "t", lambda a: _jnp().tan(a), torch.tan,
         lambda a: (np.sin(a) / np.cos(a), F(1) + (np.sin(a) / np.cos(a)) * (np.sin(a) / np.cos(a))), {"SIN", "COS", "DIV"}, 2.5e-07),
    Case("expm1", "s", lambda a: _jnp().expm1(a), torch.expm1, lambda a: (np.exp(a) - F(1), np.exp(a)), {"EXP"}, 1.4e-07),
    Case("mod", "sp", lambda a, b: _jnp().mod(a, b), torch.remainder, _mod_hand, {"FLOOR"}, 4.3e-07),
    Case("fan_out", "ss", lambda a, b: _fan_fn(_jnp(), a, b), lambda a, b: _fan_fn(torch, a, b), _fan_hand, {"ADD", "MUL", "LOG", "SQRT"}, 2.1e-07),
    Case("big", "sp", lambda a, b: _big_fn(_jnp(), a, b), lambda a, b: _big_fn(torch, a, b), _big_hand, {"ADD", "MUL", "EXP"}, 3.9e-07),
]
RULE = {c.name: c for c in RULES}
RULE_NAMES = [c.name for c in RULES]
BIG = "big"                    # the case the 31-register interpreter cannot hold


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """[value, gradient per operand] of torch.float64 autograd on the float32 inputs widened (never modified)"""
    case = RULE[name]
    xs = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in inputs(name, n)]
    v = case.ref(*xs)
    gs = torch.autograd.grad(v.sum(), xs, allow_unused=True)
    out = [v.detach().numpy()] + [np.zeros(n) if g is None else g.numpy() for g in gs]
    for a in out:
        a.setflags(write=False)
    return out


def deviation(got, want, what):
    """max |got - want| / (1 + |want|) where `want` (float64) is finite; NaNs and infinities must sit where want's do"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist())
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, "infinities", np.argwhere(inf & (got != want))[:5].tolist())
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(got[fin] - want[fin]) / (1.0 + np.abs(want[fin]))))


@functools.lru_cache(maxsize=None)
def replay_error(name):
    """the hand-written float32 derivative against float64, on the case's 1027 inputs"""
    case = RULE[name]
    with np.errstate(all="ignore"):
        mine = case.hand(*inputs(name, N_TILE))
    want = reference(name, N_TILE)
    assert len(mine) == len(want)
    for m in mine:
        assert np.asarray(m).dtype == np.float32, (name, np.asarray(m).dtype)
    return max(deviation(m, w, (name, "replay", k)) for k, (m, w) in enumerate(zip(mine, want)))


def bound(name):
    return max(4.0 * replay_error(name), FLOOR)


# --- running one case ------------------------------------------------------------------------------------------------------------
def launch(be, fn, xs):
    """value_and_grad(fn) on numpy operands -> ([value, gradients ...] as numpy, the compiled program)"""
    from genjax_amd import autodiff
    ts = [torch.from_numpy(np.array(x)).to(be.device) for x in xs]
    v, gs = autodiff.value_and_grad(fn)(*ts)
    comp = next(reversed(autodiff._VG_CACHE.values()))[0]
    assert len(gs) == len(xs)
    out = []
    for t in (v,) + tuple(gs):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == tuple(ts[0].shape), t
        assert t.device.type == ts[0].device.type
        out.append(t.detach().cpu().numpy())
    return out, comp


@contextlib.contextmanager
def every_program_specialised(be):
    """the idiom of test_hmc_programs_over_long_vector_sites_as_specialised_kernels: every program goes through hiprtc, and
    none of them may be rejected by the first-launch cross-check against the interpreter"""
    from genjax_amd import engine
    old = engine.JIT_MIN_PARTICLES
    before = int(be.c.gmx_jit_rejected_count())
    engine.JIT_MIN_PARTICLES = 1
    try:
        engine.clear_caches()
        yield
    finally:
        engine.JIT_MIN_PARTICLES = old
        engine.clear_caches()
    assert int(be.c.gmx_jit_rejected_count()) == before


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_rule(be, name, n):
    """CPU mirror / the device's default at this n (the interpreter; the specialised kernel where the interpreter cannot
    hold the program)"""
    case = RULE[name]
    got, comp = launch(be, case.fn, inputs(name, n))
    if name == BIG:
        assert comp.max_regs > 31, comp.max_regs
        assert not be.uses_streams or comp.is_specialized()
    elif be.uses_streams:
        assert not comp.is_partly_specialized()
    lim = bound(name)
    for k, (g, w) in enumerate(zip(got, reference(name, n))):
        d = deviation(g, w, (name, n, k))
        print(f"{name} n={n} output {k}: deviation {d:.3g} (replay {replay_error(name):.3g}, bound {lim:.3g})")
        assert d <= lim, (name, n, k, d, lim)
    return got


def check_rule_specialised(be, name):
    """GPU: the case at both sizes interpreted, then specialised; equal bit for bit where the interpreter holds the program,
    and the specialised outputs held to float64 in every case"""
    case = RULE[name]
    plain = {n: check_rule(be, name, n) for n in SIZES} if name != BIG else {}
    lim = bound(name)
    with every_program_specialised(be):
        for n in SIZES:
            got, comp = launch(be, case.fn, inputs(name, n))
            assert comp.is_specialized()
            assert (comp.max_regs > 31) == (name == BIG), comp.max_regs
            for k, (g, w) in enumerate(zip(got, reference(name, n))):
                d = deviation(g, w, (name, n, k, "specialised"))
                print(f"{name} n={n} output {k} specialised: deviation {d:.3g} (bound {lim:.3g})")
                assert d <= lim, (name, n, k, d, lim)
                if name != BIG:
                    assert np.array_equal(_bits(g), _bits(plain[n][k])), (name, n, k, "specialised != interpreted")


# --- edges: operands with exact expected results ----------------------------------------------------------------------------------
_E24 = 2.0 ** -24
_INF, _NAN = math.inf, math.nan
_R = float(F(1) / F(1 - _E24))                 # 1 / (1 - 2^-24) in float32: one correctly rounded division
_LN2 = math.log(2.0)

Edge = namedtuple("Edge", "name fn rows want vtol gtol")
# rows: one tuple of operands per particle; want: per row (value, gradient per operand).  vtol / gtol (value / gradients)
# = 0: every finite number is the float32 nearest to `want` exactly (+0 and -0 alike) — every pinned gradient is one
# correctly rounded operation on exact operands; = FLOOR where the number passes through a device logarithm or exponential
# (a transcendental value, or a limit reached up to exp(-100): |got - want| <= FLOOR (1 + |want|)).  NaN and infinities
# always exactly.
EDGES = [
    Edge("flip_true_ends", lambda p: _G().flip.sym_logpdf(True, (p,)), [(0.0,), (1.0,), (_E24,), (1 - _E24,)],
         [(-_INF, _INF), (0.0, 1.0), (-24 * _LN2, 2.0 ** 24), (math.log1p(-_E24), _R)], FLOOR, 0.0),
    Edge("flip_false_ends", lambda p: _G().flip.sym_logpdf(False, (p,)), [(0.0,), (1.0,), (_E24,), (1 - _E24,)],
         [(0.0, -1.0), (-_INF, -_INF), (math.log1p(-_E24), -_R), (-24 * _LN2, -(2.0 ** 24))], FLOOR, 0.0),
    Edge("bernoulli_logits_saturated", lambda l, x: _G().bernoulli.sym_logpdf(x > 0.5, (l,)) + x * 0.0,
         [(100.0, 1.0), (-100.0, 1.0), (100.0, 0.0), (-100.0, 0.0)],
         [(0.0, 0.0, 0.0), (-100.0, 1.0, 0.0), (-100.0, -1.0, 0.0), (0.0, 0.0, 0.0)], FLOOR, FLOOR),
    Edge("softplus_saturated", lambda a: _jnp().softplus(a), [(100.0,), (-100.0,)], [(100.0, 1.0), (0.0, 0.0)], FLOOR, FLOOR),
    Edge("abs_at_zero", lambda a: abs(a), [(0.0,), (-0.0,), (1.5,), (-1.5,)], [(0.0, 0.0), (0.0, 0.0), (1.5, 1.0), (1.5, -1.0)], 0.0, 0.0),
    Edge("max_tie", lambda a, b: _jnp().maximum(a, b), [(1.5, 1.5), (0.0, 0.0), (-2.0, -2.0), (1.0, 2.0), (2.0, 1.0)],
         [(1.5, 0.5, 0.5), (0.0, 0.5, 0.5), (-2.0, 0.5, 0.5), (2.0, 0.0, 1.0), (2.0, 1.0, 0.0)], 0.0, 0.0),
    Edge("min_tie", lambda a, b: _jnp().minimum(a, b), [(1.5, 1.5), (0.0, 0.0), (-2.0, -2.0), (1.0, 2.0), (2.0, 1.0)],
         [(1.5, 0.5, 0.5), (0.0, 0.5, 0.5), (-2.0, 0.5, 0.5), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0)], 0.0, 0.0),
    Edge("clip_tie", lambda a, b: _jnp().clip(a, b, b + 2.0), [(1.0, 1.0), (3.0, 1.0), (2.0, 1.0), (0.0, 1.0), (5.0, 1.0)],
         [(1.0, 0.5, 0.5), (3.0, 0.5, 0.5), (2.0, 1.0, 0.0), (1.0, 0.0, 1.0), (3.0, 0.0, 1.0)], 0.0, 0.0),
    Edge("pow_at_zero_and_negative_base", lambda a, b: _jnp().power(a, b), [(0.0, 2.5), (0.0, 1.0), (-2.0, 3.0), (-1.5, 3.0), (-2.0, 2.0)],
         [(0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-8.0, 12.0, _NAN), (-3.375, 6.75, _NAN), (4.0, -4.0, _NAN)], FLOOR, 0.0),
    Edge("uniform_at_the_bounds", lambda x, lo, hi: _G().uniform.sym_logpdf(x, (lo, hi)),
         [(1.0, 1.0, 3.0), (3.0, 1.0, 3.0), (2.0, 1.0, 3.0), (0.0, 1.0, 3.0), (4.0, 1.0, 3.0)],
         [(-_LN2, 0.0, 0.5, -0.5), (-_LN2, 0.0, 0.5, -0.5), (-_LN2, 0.0, 0.5, -0.5), (-_INF, 0.0, 0.0, 0.0), (-_INF, 0.0, 0.0, 0.0)], FLOOR, 0.0),
    Edge("sqrt_at_zero", lambda a: _jnp().sqrt(a), [(0.0,), (4.0,)], [(0.0, _INF), (2.0, 0.25)], 0.0, 0.0),
    Edge("log_at_zero", lambda a: _jnp().log(a), [(0.0,), (1.0,)], [(-_INF, _INF), (0.0, 1.0)], 0.0, 0.0),
    Edge("sqrt_of_square_at_zero", lambda a: _jnp().sqrt(a * a), [(0.0,), (3.0,)], [(0.0, _NAN), (3.0, 1.0)], 0.0, 0.0),
]
EDGE = {e.name: e for e in EDGES}
EDGE_NAMES = [e.name for e in EDGES]


def _edge_operands(e):
    return [np.array([r[k] for r in e.rows], dtype=F) for k in range(len(e.rows[0]))]


def _assert_edge(e, got, how):
    for k in range(len(got)):
        want = np.array([w[k] for w in e.want], dtype=np.float64)
        g = got[k].astype(np.float64)
        what = (e.name, how, "value" if k == 0 else "gradient %d" % (k - 1), g.tolist(), want.tolist())
        assert np.array_equal(np.isnan(g), np.isnan(want)), what
        inf = np.isinf(want)
        assert np.array_equal(g[inf], want[inf]), what
        fin = np.isfinite(want)
        assert np.all(np.isfinite(g[fin])), what
        tol = e.vtol if k == 0 else e.gtol
        if tol == 0.0:
            assert np.array_equal(g[fin], want[fin].astype(F).astype(np.float64)), what
        else:
            assert np.all(np.abs(g[fin] - want[fin]) <= tol * (1.0 + np.abs(want[fin]))), what


def check_edge(be, name):
    e = EDGE[name]
    got, _ = launch(be, e.fn, _edge_operands(e))
    _assert_edge(e, got, "default")
    return got


def check_edge_specialised(be, name):
    e = EDGE[name]
    plain = check_edge(be, name)
    with every_program_specialised(be):
        got, comp = launch(be, e.fn, _edge_operands(e))
        assert comp.is_specialized()
        _assert_edge(e, got, "specialised")
        for a, b in zip(got, plain):
            assert np.array_equal(_bits(a), _bits(b)), (name, "specialised != interpreted")


def check_hmc_through_a_saturated_flip(be):
    """`flip(sigmoid(30 w)) @ "y"` observed True: sigmoid is exactly 1.0f from about 30 w = 17, the density there is 0 and
    its gradient 1 — every particle must come back with a finite position and weight"""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    from genjax_amd import SelectionBuilder as S
    from genjax_amd import numpy as jnp
    from genjax_amd.inference.requests import HMC

    @G.gen
    def model():
        w = G.normal(0.0, 1.0) @ "w"
        G.flip(jnp.sigmoid(30.0 * w)) @ "y"
        return w
    n = 64
    w0 = np.random.default_rng(11).normal(size=n).astype(F)
    assert (w0 > 0.6).sum() >= 8, "the case needs particles where the sigmoid is saturated"
    tr, _ = model.importance(G.split(G.key(5), n), C["w"].set(torch.from_numpy(w0.copy()).to(be.device)).set("y", True), ())
    new, lw, _, _ = HMC(S["w"], 1e-2, L=2).edit(G.split(G.key(6), n), tr, G.Diff.no_change(()))
    w1 = new.get_choices()["w"].cpu().numpy()
    assert np.all(np.isfinite(w1)), np.argwhere(~np.isfinite(w1)).ravel().tolist()
    lw = lw.cpu().numpy()
    assert np.all(np.isfinite(lw)), np.argwhere(~np.isfinite(lw)).ravel().tolist()
    assert np.all(w1 != w0)


# --- op classification -------------------------------------------------------------------------------------------------------------
IR_ONLY = {"LOOPVAR", "SETVAR", "LDINX", "COPY", "CATIDX", "RELOAD2"}      # program.py: IR nodes without an opcode of their own
RAISES = {"END", "STOUT", "LDKEY", "KDERIVE", "KDERIVER", "KSPLITU", "LGAMMA", "S_NORMAL", "S_UNIFORM", "S_FLIP", "S_BERNL", "S_BETA",
          "S_CATSTEP", "S_LOGGAMMA", "L_BETA", "REDMAX", "REDLSE", "LOOP", "ENDLOOP", "SETVAR", "COPY", "CATIDX", "RELOAD2"}


def all_ops():
    from genjax_amd import program as P
    ops = set(P.OPC) | P.UNARY | P.BINARY | P.LOGPDF1 | P.LOGPDF2 | P.SAMPLER1 | P.SAMPLER2 | P.EFFECT | IR_ONLY | {"SEL", "LDT", "S_CATSTEP"}
    return sorted(ops)


def _arity(op):
    from genjax_amd import program as P
    if op == "SEL" or op in P.LOGPDF2 or op in P.SAMPLER2:
        return 3
    if op in P.BINARY or op in P.LOGPDF1 or op in P.SAMPLER1 or op in ("SETVAR", "KDERIVER", "KSPLITU"):
        return 2
    return 1


def observed_class(op):
    """what autodiff._rule does with a node of this op: 'differentiable' (it pushes an adjoint), 'zero' (it returns without),
    'raises' (NotDifferentiable naming the op)"""
    from genjax_amd import autodiff, program, tracer
    g = program.Graph()
    with tracer.tracing(g):
        args = tuple(g.input("f32") for _ in range(_arity(op)))
        node = g.add(op, args, dtype="f32")
        assert node.op == op
        pushed = []
        try:
            autodiff._rule(node, tracer.lift(1.0), lambda n, c: pushed.append(n))
        except autodiff.NotDifferentiable as err:
            assert str(err).endswith(" " + op), (op, str(err))
            return "raises"
    return "differentiable" if pushed else "zero"


def rule_ops_of(name):
    """the ops autodiff._rule is called on when the case's function is differentiated (traced without a launch)"""
    from genjax_amd import autodiff, program, tracer
    case = RULE[name]
    g = program.Graph()
    seen = set()
    real = autodiff._rule

    def spy(n, a, push):
        seen.add(n.op)
        return real(n, a, push)
    autodiff._rule = spy
    try:
        with tracer.tracing(g):
            ins = [tracer.Expr(g.input("f32")) for _ in case.doms]
            autodiff.grad(tracer.as_float(case.fn(*ins)), ins)
    finally:
        autodiff._rule = real
    return seen


def check_classification():
    from genjax_amd import autodiff
    ops = all_ops()
    declared = {}
    for op in ops:
        kinds = [k for k, s in (("differentiable", autodiff.DIFFERENTIABLE), ("zero", autodiff.ZERO_GRADIENT), ("raises", RAISES)) if op in s]
        assert len(kinds) == 1, (op, kinds)
        declared[op] = kinds[0]
    assert autodiff.DIFFERENTIABLE | autodiff.ZERO_GRADIENT <= set(ops)
    for op in ops:
        if op == "LOOPVAR":                # differentiated in grad() itself (the loop's own accumulated derivative): the
            continue                       # loop-form HMC checks below are its case
        assert observed_class(op) == declared[op], (op, observed_class(op), declared[op])
    # every differentiable op is what some RULES case is there for, and that case's differentiation really reaches its rule
    covered = set()
    for c in RULES:
        reached = rule_ops_of(c.name)
        assert c.ops <= reached, (c.name, c.ops - reached)
        covered |= c.ops & autodiff.DIFFERENTIABLE
    assert covered == autodiff.DIFFERENTIABLE - {"LOOPVAR"}, autodiff.DIFFERENTIABLE - {"LOOPVAR"} - covered


def check_not_differentiable_by_name(be):
    import pytest
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    from genjax_amd import SelectionBuilder as S
    from genjax_amd import numpy as jnp
    from genjax_amd.autodiff import NotDifferentiable, value_and_grad
    from genjax_amd.inference.requests import HMC
    x = torch.full((3,), 0.4, dtype=torch.float32, device=be.device)
    with pytest.raises(NotDifferentiable, match="LGAMMA"):
        value_and_grad(lambda a: jnp.lgamma(a))(x + 1.0)
    with pytest.raises(NotDifferentiable, match="L_BETA"):
        value_and_grad(lambda a, b: G.beta.sym_logpdf(a, (b, 2.0)))(x, x + 1.0)

    @G.gen
    def model():
        p = G.beta(2.0, 3.0) @ "p"
        G.normal(p, 1.0) @ "y"
        return p
    tr, _ = model.importance(G.split(G.key(1), 5), C["y"].set(0.3), ())
    with pytest.raises(NotDifferentiable, match="L_BETA"):
        HMC(S["p"], 1e-2, L=1).edit(G.key(2), tr, G.Diff.no_change(()))


# --- value_and_grad as an API ------------------------------------------------------------------------------------------------------
def check_cache_key_sees_defaults(be):
    import genjax_amd as G
    from genjax_amd.autodiff import value_and_grad
    a = np.array([0.3, 0.6, 0.9], dtype=F)
    b = np.array([1.0, -2.0, 0.5], dtype=F)
    want = {True: (np.log(a.astype(np.float64)) + b, 1.0 / a.astype(np.float64)),
            False: (np.log1p(-a.astype(np.float64)) + b, -1.0 / (1.0 - a.astype(np.float64)))}
    for ev in (True, False, True):
        got, _ = launch(be, lambda p, q, ev=ev: G.flip.sym_logpdf(ev, (p,)) + q, (a, b))
        assert np.allclose(got[0], want[ev][0], rtol=0, atol=1e-5) and np.allclose(got[1], want[ev][1], rtol=1e-5), ev
    for scale in (2.0, 3.0):               # keyword-only defaults
        got, _ = launch(be, lambda p, q, *, s=scale: p * s + q, (a, b))
        assert np.array_equal(got[1], np.full(3, scale, F)), scale
    for tab in ([1.0, 2.0], [5.0, 7.0]):   # unhashable: by identity
        got, _ = launch(be, lambda p, q, t=tab: p * t[0] + q * t[1], (a, b))
        assert np.array_equal(got[1], np.full(3, tab[0], F)) and np.array_equal(got[2], np.full(3, tab[1], F)), tab


def check_fnkey():
    from genjax_amd.static import _fnkey
    fs = [lambda a, ev=ev: (a, ev) for ev in (True, False, True)]
    assert _fnkey(fs[0]) != _fnkey(fs[1]) and _fnkey(fs[0]) == _fnkey(fs[2])
    ks = [lambda a, *, s=s: (a, s) for s in (1.0, 2.0, 1.0)]
    assert _fnkey(ks[0]) != _fnkey(ks[1]) and _fnkey(ks[0]) == _fnkey(ks[2])
    t1, t2 = [1.0], [1.0]
    us = [lambda a, t=t: (a, t) for t in (t1, t2, t1)]
    assert _fnkey(us[0]) != _fnkey(us[1]) and _fnkey(us[0]) == _fnkey(us[2])
    hash(_fnkey(us[0]))


def check_rejuvenate_argument_mappings_that_differ_in_a_default(be):
    """two Rejuvenate requests whose argument_mapping differs only in a default value: each proposes around ITS centre"""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    from genjax_amd.inference.requests import Rejuvenate

    @G.gen
    def model():
        x = G.normal(0.0, 10.0) @ "x"
        G.normal(x, 10.0) @ "y"
        return x

    n = 16
    tr, _ = model.importance(G.split(G.key(3), n), C["y"].set(0.0), ())
    for centre in (5.0, -7.0, 5.0):
        req = G.StaticRequest({"x": Rejuvenate(G.normal, lambda chm, c=centre: (c, 0.001))})
        new = req.edit(G.split(G.key(4), n), tr, G.Diff.no_change(()))[0]
        x = new.get_choices()["x"].cpu().numpy()
        assert np.all(np.abs(x - centre) < 0.1), (centre, x[:4].tolist())


def check_constant_gradients_are_tensors(be):
    a = np.array([0.25, 1.0, 4.0, 9.0, 16.0], dtype=F)
    b = np.array([1.0, 2.0, 3.0, 4.0, 5.0], dtype=F)
    jnp = _jnp()
    got, _ = launch(be, lambda p, q: jnp.sqrt(p) + q, (a, b))             # d/dq folds to the constant 1
    assert np.array_equal(got[2], np.ones(5, F)) and np.array_equal(got[1], F(0.5) / np.sqrt(a))
    got, _ = launch(be, lambda p, q: p * 2.0, (a, b))                     # q unused: a zero gradient
    assert np.array_equal(got[2], np.zeros(5, F)) and np.array_equal(got[1], np.full(5, 2.0, F))
    got, _ = launch(be, lambda p, q: p * 0.0 + 3.0, (a, b))
    assert got[0].shape == (5,) and np.array_equal(got[0], np.full(5, 3.0, F))
    got, _ = launch(be, lambda p, q: p + q, (a.reshape(5, 1)[:, 0:1].copy(), b.reshape(5, 1).copy()))    # a batch of two axes
    assert got[1].shape == (5, 1) and np.array_equal(got[1], np.ones((5, 1), F))


# --- one leapfrog step of HMC through the non-normal densities, reconstructed from its outputs ----------------------------------------
# Logistic regression, a, b ~ normal(0, 2): 8 observations unroll the site (the plain rules), 40 make it a counted loop whose
# loop-carried registers accumulate d score / d a, d score / d b (static._vector_site_loop, LOOPVAR's custom derivative).
# With L = 1 the move is determined by what it returns: p_half = (x' - x) / eps, p0 = p_half - eps/2 g(x),
# p1 = p_half + eps/2 g(x'), weight = logp(x') - logp(x) - p1^2/2 + p0^2/2 summed over a and b — in float64 with torch's
# gradient.  The bound: the same reconstruction in numpy float32 (scores summed in element order, as the site sums them)
# from the same trajectory, its worst deviation from float64 times 4, by the metric of the rules; measured on the CPU
# mirror's trajectories: bernoulli 8: 2.3e-6, bernoulli 40: 1.2e-5, flip 40: 1.3e-5, uniform 40: 4.3e-5 (weights up to 0.07, 2.6,
# 1.4 and 21; the scores the weight is a difference of are sums of 10 to 42 float32 terms of magnitude up to 100).
HMC_K, HMC_EPS = 257, 0.25
HMC_CASES = [(8, "bernoulli"), (40, "bernoulli"), (40, "flip"), (40, "uniform")]


@functools.lru_cache(maxsize=None)
def hmc_data(n_obs, density):
    """(xs, ys, a0, b0), never modified"""
    rng = np.random.default_rng(1000 + n_obs + len(density))
    xs = np.linspace(-1.0, 1.0, n_obs).astype(F)
    if density == "uniform":
        ys = rng.uniform(-0.9, 0.9, size=n_obs).astype(F)
    else:
        ys = (rng.uniform(size=n_obs) < 1.0 / (1.0 + np.exp(-(1.5 * xs - 0.3)))).astype(np.int32)
    a0, b0 = rng.normal(size=HMC_K).astype(F), rng.normal(size=HMC_K).astype(F)
    for v in (xs, ys, a0, b0):
        v.setflags(write=False)
    return xs, ys, a0, b0


def _hmc_model(n_obs, density):
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    xs, ys, _, _ = hmc_data(n_obs, density)

    @G.gen
    def model():
        a = G.normal(0.0, 2.0) @ "a"
        b = G.normal(0.0, 2.0) @ "b"
        if density == "bernoulli":
            G.bernoulli(logits=a * jnp.array(xs) + b) @ "y"
        elif density == "flip":
            G.flip(jnp.sigmoid(a * jnp.array(xs) + b)) @ "y"
        else:
            G.uniform((-abs(a) - 1.0) * jnp.ones(n_obs), (abs(b) + 1.0) * jnp.ones(n_obs)) @ "y"
        return a
    obs = jnp.array(ys if density == "uniform" else (ys.astype(bool) if density == "flip" else ys))
    return model, obs


def _logp64(density, xs, ys, a, b):
    """the model's log-density at (a, b) [K] in float64 torch"""
    x, y = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
    prior = sum(-0.5 * (v / 2.0) ** 2 - math.log(2.0) - 0.5 * math.log(2.0 * math.pi) for v in (a, b))
    if density == "uniform":
        return prior - len(xs) * torch.log(a.abs() + b.abs() + 2.0)
    z = a[:, None] * x[None, :] + b[:, None]
    if density == "bernoulli":
        ll = y * z - torch.logaddexp(torch.zeros_like(z), z)
    else:
        p = torch.sigmoid(z)
        ll = torch.where(y > 0.5, torch.log(p), torch.log1p(-p))
    return prior + ll.sum(dim=1)


def _logp32(density, xs, ys, a, b):
    """(log-density, d/da, d/db) by hand in numpy float32, the site's terms added in element order"""
    lp = np.zeros_like(a)
    ga, gb = np.zeros_like(a), np.zeros_like(a)
    for v, g in ((a, ga), (b, gb)):
        z = v / F(2) - F(0) / F(2)
        lp = lp + (-F(0.5) * (z * z) - (_HL2PI + np.log(F(2))))
        g += -(z / F(2))
    s, sa, sb = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    for j in range(len(xs)):
        if density == "uniform":
            w = (np.abs(b) + F(1)) - (-np.abs(a) - F(1))
            s = s + (-np.log(w))
            sa = sa + (-(np.sign(a) / w))
            sb = sb + (-(np.sign(b) / w))
            continue
        z = a * xs[j] + b
        if density == "bernoulli":
            t = -_softplus(-z) if ys[j] else -_softplus(z)
            dz = F(ys[j]) - _sig(z)
        else:
            p = _sig(z)
            t = np.log(p) if ys[j] else np.log1p(-p)
            dz = (F(1) / p if ys[j] else -(F(1) / (F(1) - p))) * (p * (F(1) - p))
        s = s + t
        sa = sa + dz * xs[j]
        sb = sb + dz
    return lp + s, ga + sa, gb + sb


def hmc_weight64(density, xs, ys, x0, x1):
    """x0 = (a, b), x1 = (a', b') float32 [K] -> the float64 weight of the one-step move between them"""
    def lp_g(x):
        v = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in x]
        lp = _logp64(density, xs, ys, *v)
        g = torch.autograd.grad(lp.sum(), v)
        return lp.detach().numpy(), [t.numpy() for t in g]
    (l0, g0), (l1, g1) = lp_g(x0), lp_g(x1)
    w = l1 - l0
    for k in range(2):
        ph = (x1[k].astype(np.float64) - x0[k].astype(np.float64)) / HMC_EPS
        p0, p1 = ph - 0.5 * HMC_EPS * g0[k], ph + 0.5 * HMC_EPS * g1[k]
        w = w - 0.5 * p1 * p1 + 0.5 * p0 * p0
    return w


def hmc_weight32(density, xs, ys, x0, x1):
    eps, half = F(HMC_EPS), F(HMC_EPS) / F(2)
    l0, *g0 = _logp32(density, xs, ys, *x0)
    l1, *g1 = _logp32(density, xs, ys, *x1)
    w = l1 - l0
    k0 = k1 = np.zeros_like(l0)
    for k in range(2):
        ph = (x1[k] - x0[k]) / eps
        p0, p1 = ph - half * g0[k], ph + half * g1[k]
        k0, k1 = k0 + (-F(0.5) * (p0 * p0)), k1 + (-F(0.5) * (p1 * p1))
    return (w + (k1 - k0)).astype(F)


def _hmc_move(be, n_obs, density):
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    from genjax_amd import SelectionBuilder as S
    from genjax_amd.inference import requests
    _, _, a0, b0 = hmc_data(n_obs, density)
    model, obs = _hmc_model(n_obs, density)
    dev = lambda v: torch.from_numpy(v.copy()).to(be.device)      # noqa: E731
    tr, _ = model.importance(G.split(G.key(21), HMC_K), C["a"].set(dev(a0)).set("b", dev(b0)).set("y", obs), ())
    new, w, _, _ = requests.HMC(S["a"] | S["b"], HMC_EPS, L=1).edit(G.split(G.key(22), HMC_K), tr, G.Diff.no_change(()))
    comp = next(reversed(requests._CACHE.values()))[0]
    ch = new.get_choices()
    return ch["a"].cpu().numpy(), ch["b"].cpu().numpy(), w.cpu().numpy(), comp


def _assert_hmc(n_obs, density, a1, b1, w, how):
    xs, ys, a0, b0 = hmc_data(n_obs, density)
    assert a1.shape == (HMC_K,) and b1.shape == (HMC_K,) and w.shape == (HMC_K,)
    assert np.all(np.isfinite(a1)) and np.all(np.isfinite(b1)) and np.all(a1 != a0) and np.all(b1 != b0)
    want = hmc_weight64(density, xs, ys, (a0, b0), (a1, b1))
    replay = deviation(hmc_weight32(density, xs, ys, (a0, b0), (a1, b1)), want, (n_obs, density, "replay"))
    lim = max(4.0 * replay, FLOOR)
    d = deviation(w, want, (n_obs, density, how))                 # every particle
    print(f"hmc {density} {n_obs} {how}: weight deviation {d:.3g} (float32 replay {replay:.3g}, bound {lim:.3g}); "
          f"|weight| up to {np.abs(want).max():.3g}")
    assert d <= lim, (n_obs, density, how, d, lim)


def check_hmc_step(be, n_obs, density):
    a1, b1, w, comp = _hmc_move(be, n_obs, density)
    loops = sum(1 for wd in np.asarray(comp.blob[10:10 + 2 * int(comp.blob[2]):2]) if (int(wd) & 0xFF) == 100) if not comp.links else None
    if loops is not None:
        assert (loops > 0) == (n_obs > 16), (n_obs, loops)       # the form the case is there for
    _assert_hmc(n_obs, density, a1, b1, w, "default")
    return a1, b1, w


def check_hmc_step_specialised(be, n_obs, density):
    plain = check_hmc_step(be, n_obs, density)
    with every_program_specialised(be):
        a1, b1, w, comp = _hmc_move(be, n_obs, density)
        assert comp.is_specialized()
        _assert_hmc(n_obs, density, a1, b1, w, "specialised")
        for u, v in zip((a1, b1, w), plain):
            assert np.array_equal(_bits(u), _bits(v)), (n_obs, density, "specialised != interpreted")
