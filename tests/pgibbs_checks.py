"""Shared drivers of tests/test_pgibbs_cpu.py (the C-ABI's CPU mirror) and tests/test_pgibbs_gpu.py (the HIP library):
gmx_pg_open, gmx_pg_propose and gmx_pg_accept against their definitions in numpy (BootstrapBank._key_tables and
random._derive_host for the keys, the helpers of tests/pmmh_checks.py for the draws and the decisions, float32 / float64
numpy for the rest), smc.ParticleGibbs against the same chain composed in a Python loop from public parts, the captured
sweep against the uncaptured run, the device against the mirror, the API's refusals, and the law: the chains' last states
against the exact posterior, with a float64 numpy particle Gibbs of the same design beside it."""
from __future__ import annotations

import ctypes
import functools
import math
import types

import numpy as np
import torch

from tests import history_checks as H
from tests import pmmh_checks as M

POISON = M.POISON
ITERS = 6
SEED = 20103                            # the run key of every chain case; no reference decision is a near-tie (asserted)
NEAR_TIE = M.NEAR_TIE
# (R, n, T, P): the base case; chain boundaries off multiples of 4 inside a span; more than 256 chains in a span and more
# than one workgroup of the per-chain kernels; one parameter; T = 1 (no transition term); one chain per span and the pinned
# resampler's largest n; spans straddling chains with leaves off 16-byte alignment
CASES = {"tiny": (5, 8, 3, 2), "edges": (3, 100, 4, 2), "wide": (300, 4, 2, 2), "one": (5, 8, 3, 1), "single_step": (4, 8, 1, 2),
         "full_tile": (2, 1024, 2, 2), "straddle": (3, 1023, 2, 1)}
# (case, ancestor_sampling, backward) of every chain test
CHAINS = [(c, False, False) for c in CASES] + [("tiny", True, False), ("edges", True, False), ("tiny", False, True)]
STEP_SIZE = (0.05, 0.1)
PRIOR = (M.PRIOR[0], (0.5, 2.0))        # uniform priors on the transition coefficient and on the OBSERVATION scale


def chain_id(c):
    return c[0] + ("-ancestors" if c[1] else "") + ("-backward" if c[2] else "")


def _np(t):
    return t.detach().cpu().numpy()


def _up(be, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(be.device)


def same64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


# --- the key schedule ---------------------------------------------------------------------------------------------------------
def iter_keys(key_words, j):
    """(k_sweep, k_draw, k_prop, k_acc) of iteration j: split(fold_in(key, j), 4)"""
    from genjax_amd.random import _derive_host
    k_it = _derive_host(np.asarray(key_words, np.uint32).reshape(2), np.uint64(j))
    ks = _derive_host(k_it[None, :], np.arange(4, dtype=np.uint64))
    return ks[0], ks[1], ks[2], ks[3]


def key_tables3(chain_keys, T):
    """BootstrapBank._key_tables(keys, third=True) under the R keys `chain_keys`: three [T, R, 2] uint32 tables"""
    from genjax_amd.inference.smc import BootstrapBank
    from genjax_amd.random import Key
    me = types.SimpleNamespace(R=chain_keys.shape[0], T=T)
    return tuple(t.view(np.uint32) for t in
                 BootstrapBank._key_tables(me, Key(host=np.ascontiguousarray(chain_keys, dtype=np.uint32)), third=True))


def start_of(R, P, seed=0):
    rng = np.random.default_rng(2000 + seed)
    lo = np.array([PRIOR[p][0] for p in range(P)], np.float32)[:, None]
    hi = np.array([PRIOR[p][1] for p in range(P)], np.float32)[:, None]
    return (lo + (hi - lo) * rng.uniform(0.05, 0.95, size=(P, R))).astype(np.float32)


# --- gmx_pg_open ------------------------------------------------------------------------------------------------------------
def run_open(be, key_words, j, theta, n, T, lead=0, pad=5, third=True):
    """the leaves are rows of ONE poisoned buffer, `lead` floats into their row: rows start at every 4-byte alignment"""
    dev = be.device
    P, R = theta.shape
    N = R * n
    th = _up(be, theta, np.float32)
    buf = torch.full((P, lead + N + pad), float(POISON), dtype=torch.float32, device=dev)
    table = torch.tensor([buf[p].data_ptr() + 4 * lead for p in range(P)], dtype=torch.int64, device=dev)
    kp, kr, ka = (torch.full((T, R, 2), -3, dtype=torch.int32, device=dev) for _ in range(3))
    rc = be.c.gmx_pg_open(M._words(key_words), int(j), be.ptr(th), P, R, n, T, be.ptr(kp), be.ptr(kr),
                          be.ptr(ka) if third else None, be.ptr(table), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    b = buf.cpu().numpy()
    assert np.all(b[:, :lead] == POISON) and np.all(b[:, lead + N:] == POISON), "the padding around a leaf was written"
    assert H.same_bits(_np(th), np.ascontiguousarray(theta, dtype=np.float32)), "theta was written"
    return b[:, lead:lead + N], [_np(k).view(np.uint32) for k in (kp, kr, ka)]


def check_open(be, case):
    """the three key tables and the broadcast leaves, bit for bit, at every alignment of a leaf; keys_as null: two tables"""
    R, n, T, P = CASES[case]
    key = np.array([0x4321, 0xABC0 + R], np.uint32)
    theta = start_of(R, P)
    for j, lead, third in ((0, 0, True), (1, 1, True), (5, 2, False), (2 ** 32 - 2, 3, True)):
        leaves, tables = run_open(be, key, j, theta, n, T, lead=lead, third=third)
        want = key_tables3(M.split_host(iter_keys(key, j)[0], R), T)
        assert H.same_bits(leaves, np.repeat(theta, n, axis=1)), (case, j, lead, "leaves", np.argwhere(leaves != np.repeat(theta, n, axis=1))[:5].tolist())
        assert np.array_equal(tables[0], want[0]), (case, j, "keys_prop")
        assert np.array_equal(tables[1], want[1]), (case, j, "keys_res")
        if third:
            assert np.array_equal(tables[2], want[2]), (case, j, "keys_as")
        else:
            assert np.all(tables[2].view(np.int32) == -3), (case, j, "keys_as was written through a null argument's neighbour")


# --- gmx_pg_propose ---------------------------------------------------------------------------------------------------------
def run_propose(be, key_words, j, theta, scale):
    P, R = theta.shape
    th, sc = _up(be, theta, np.float32), _up(be, scale, np.float32)
    out = torch.full((P, 2 * R), float(POISON), dtype=torch.float32, device=be.device)
    rc = be.c.gmx_pg_propose(M._words(key_words), int(j), be.ptr(th), be.ptr(sc), P, R, be.ptr(out), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    assert H.same_bits(_np(th), np.ascontiguousarray(theta, dtype=np.float32)), "theta was written"
    return _np(out)


def check_propose(be, case):
    """[theta | theta'] bit for bit; iteration 0 moves too"""
    R, _n, _T, P = CASES[case]
    key = np.array([0x1234, 0x9ABC + R], np.uint32)
    theta, scale = start_of(R, P), np.asarray(STEP_SIZE[:P], np.float32)
    for j in (0, 1, 5, 2 ** 32 - 2):
        got = run_propose(be, key, j, theta, scale)
        want = M.proposals(be, iter_keys(key, j)[2], 1, theta, scale)        # (pmmh's j only says "not the start")
        assert H.same_bits(got[:, :R], theta), (case, j, "the current half")
        assert H.same_bits(got[:, R:], want), (case, j, "the proposals")
        assert not np.any(got[:, R:] == theta), (case, j, "a proposal did not move")


# --- gmx_pg_accept ----------------------------------------------------------------------------------------------------------
def sequential_sums(joint):
    """[T, C] float32 -> [C] float64, summed in ascending t"""
    acc = np.zeros((joint.shape[1],), np.float64)
    with np.errstate(invalid="ignore"):
        for t in range(joint.shape[0]):
            acc = acc + joint[t].astype(np.float64)
    return acc


def decide(be, k_acc, joint, lp, what):
    """(take [R] bool, S [2R] float64) by the host helpers; asserts that no decision is a near-tie"""
    R = lp.size // 2
    S = sequential_sums(joint)
    with np.errstate(invalid="ignore", over="ignore"):
        log_alpha = ((S[R:] - S[:R]) + (lp[R:].astype(np.float64) - lp[:R].astype(np.float64))).astype(np.float32)
    keys = M.split_host(k_acc, R)
    take = M.mh_accept_of(be, keys, log_alpha) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.abs(np.log(M.unit_of(M.bits_of(be, keys)).astype(np.float64)) - log_alpha.astype(np.float64))
    assert not np.any(gap < NEAR_TIE), (what, "a decision of the reference is a near-tie: choose another seed", np.nanmin(gap))
    return take, S


def run_accept(be, key_words, j, joint, obs, lp, theta_pair, theta, row, cap):
    dev = be.device
    P, R = theta.shape
    T = joint.shape[0]
    jt, ob, l, tp, th = (_up(be, a, np.float32) for a in (joint, obs, lp, theta_pair, theta))
    lj = torch.full((R,), float(POISON), dtype=torch.float64, device=dev)
    ref = torch.full((T, R), float(POISON), dtype=torch.float32, device=dev)
    rt = torch.full((cap, P, R), float(POISON), dtype=torch.float32, device=dev)
    rl = torch.full((cap, R), float(POISON), dtype=torch.float64, device=dev)
    ra = torch.full((cap, R), 9, dtype=torch.uint8, device=dev)
    rc = be.c.gmx_pg_accept(M._words(key_words), int(j), be.ptr(jt), be.ptr(ob), be.ptr(l), be.ptr(tp), T, R, P, be.ptr(th),
                            be.ptr(lj), be.ptr(ref), be.ptr(rt), be.ptr(rl), be.ptr(ra), row, cap, be.stream())
    assert rc == 0, be.c.gmx_last_error()
    for a, was in ((jt, joint), (ob, obs), (l, lp), (tp, theta_pair)):
        assert H.same_bits(_np(a), np.ascontiguousarray(was, dtype=np.float32)), "an input was written"
    return dict(theta=_np(th), log_joint=_np(lj), ref_lw=_np(ref), rec_theta=_np(rt), rec_lj=_np(rl), rec_acc=_np(ra))


def accept_case(R, T, P, seed=5):
    """synthetic scores (never modified): chain 0's current column holds -inf, chain 1's proposal is outside the prior,
    chain 2 holds -inf on both, chain 3's proposal column holds a NaN; the observation scores hold -inf and NaN entries"""
    rng = np.random.default_rng(seed + 11 * R + T)
    joint = (2.0 * rng.normal(size=(T, 2 * R))).astype(np.float32)
    obs = rng.normal(size=(T, 2 * R)).astype(np.float32)
    lp = rng.normal(size=(2 * R,)).astype(np.float32)
    theta_pair = rng.normal(size=(P, 2 * R)).astype(np.float32)
    joint[0, 0] = -np.inf
    obs[T - 1, 0], obs[0, R] = -np.inf, np.float32(3.25)
    if R > 3:
        lp[R + 1] = -np.inf
        joint[T - 1, 2], joint[0, R + 2] = -np.inf, -np.inf
        joint[T // 2, R + 3] = np.nan
        obs[0, 3], obs[0, R + 3] = np.nan, -np.inf
    return joint, obs, lp, theta_pair


def check_accept(be, R, T, P):
    joint, obs, lp, theta_pair = accept_case(R, T, P)
    key = np.array([78, 2000 + R], np.uint32)
    j, row, cap = 7, 2, 4
    take, S = decide(be, iter_keys(key, j)[3], joint, lp, ("accept", R, T, P))
    assert take[0]
    if R > 3:
        assert not take[1] and not take[2] and not take[3]
    if R > 8:
        assert take[4:].any() and not take[4:].all(), take
    theta = theta_pair[:, :R].copy()
    theta[:, -1] += 1.0                  # (the state is REPLACED by a column of the pair, not kept)
    got = run_accept(be, key, j, joint, obs, lp, theta_pair, theta, row, cap)
    col = np.where(take, np.arange(R) + R, np.arange(R))
    with np.errstate(invalid="ignore"):
        want_lj = S[col] + lp[col].astype(np.float64)
    assert not np.isnan(want_lj).any()
    assert np.array_equal(got["rec_acc"][row], take.astype(np.uint8)), (got["rec_acc"][row], take)
    assert H.same_bits(got["theta"], theta_pair[:, col]) and H.same_bits(got["rec_theta"][row], theta_pair[:, col])
    assert same64(got["log_joint"], want_lj) and same64(got["rec_lj"][row], want_lj), (got["log_joint"], want_lj)
    assert H.same_bits(got["ref_lw"], obs[:, col]), "ref_lw is the selected column of obs, for takers and non-takers alike"
    others = [k for k in range(cap) if k != row]
    assert np.all(got["rec_theta"][others] == POISON) and np.all(got["rec_lj"][others] == POISON) and np.all(got["rec_acc"][others] == 9)


# --- refusals ----------------------------------------------------------------------------------------------------------------
def refusal_calls():
    """(entry point, arguments, what the message has to name) the three entry points must refuse before any launch"""
    N, i64, i32, u32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    buf = (ctypes.c_int64 * 8)()
    Pt = ctypes.cast(buf, ctypes.c_void_p)
    key = (ctypes.c_uint32 * 2)(1, 2)

    def open_(key=key, theta=Pt, P=2, R=3, n=4, T=2, kp=Pt, kr=Pt, ka=N, leaves=Pt):
        return (key, u32(1), theta, i32(P), i64(R), i64(n), i32(T), kp, kr, ka, leaves, N)

    def propose(key=key, theta=Pt, scale=Pt, P=2, R=3, out=Pt):
        return (key, u32(1), theta, scale, i32(P), i64(R), out, N)

    def accept(key=key, joint=Pt, obs=Pt, lp=Pt, pair=Pt, T=2, R=3, P=2, theta=Pt, lj=Pt, ref=Pt, rt=Pt, rl=Pt, ra=Pt, row=0, cap=4):
        return (key, u32(1), joint, obs, lp, pair, i32(T), i64(R), i32(P), theta, lj, ref, rt, rl, ra, i64(row), i64(cap), N)
    calls = [("gmx_pg_open", open_(**{a: None if a == "key" else N}), b"null") for a in ("key", "theta", "kp", "kr", "leaves")]
    calls += [("gmx_pg_open", open_(P=0), b"P = 0 is outside [1, 8]"), ("gmx_pg_open", open_(P=9), b"P = 9"),
              ("gmx_pg_open", open_(R=0), b"R = 0"), ("gmx_pg_open", open_(n=0), b"n = 0"), ("gmx_pg_open", open_(T=0), b"T = 0"),
              ("gmx_pg_open", open_(R=2 ** 20, n=2 ** 11), b"R * n = 2147483648"),
              ("gmx_pg_open", open_(R=2 ** 30, n=1, T=2), b"T * R = 2147483648")]
    calls += [("gmx_pg_propose", propose(**{a: None if a == "key" else N}), b"null") for a in ("key", "theta", "scale", "out")]
    calls += [("gmx_pg_propose", propose(P=0), b"P = 0"), ("gmx_pg_propose", propose(P=9), b"P = 9"),
              ("gmx_pg_propose", propose(R=0), b"R = 0"), ("gmx_pg_propose", propose(R=2 ** 31), b"R = 2147483648")]
    calls += [("gmx_pg_accept", accept(**{a: None if a == "key" else N}), b"null")
              for a in ("key", "joint", "obs", "lp", "pair", "theta", "lj", "ref", "rt", "rl", "ra")]
    calls += [("gmx_pg_accept", accept(P=9), b"P = 9"), ("gmx_pg_accept", accept(R=2 ** 31), b"R = 2147483648"),
              ("gmx_pg_accept", accept(T=0), b"T = 0"), ("gmx_pg_accept", accept(R=2 ** 30, T=2), b"T * R = 2147483648"),
              ("gmx_pg_accept", accept(cap=0), b"cap = 0"), ("gmx_pg_accept", accept(row=4), b"row = 4"),
              ("gmx_pg_accept", accept(row=-1), b"row = -1")]
    return calls, (buf, key)


def refusal_messages(lib):
    """lib: a ctypes library (the HIP library without a GPU, or the mirror): every call refused, naming what it refuses"""
    lib.gmx_last_error.restype = ctypes.c_char_p
    saved = {}
    for name in ("gmx_pg_open", "gmx_pg_propose", "gmx_pg_accept"):
        saved[name] = getattr(lib, name).argtypes
        getattr(lib, name).argtypes = None
    calls, _keep = refusal_calls()
    out = []
    try:
        for name, args, names in calls:
            assert getattr(lib, name)(*args) != 0, (name, names)
            msg = lib.gmx_last_error()
            assert name.encode() in msg and names in msg, (msg, names)
            out.append(msg)
    finally:
        for name, was in saved.items():
            getattr(lib, name).argtypes = was
    return out


# --- the models ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def models(P):
    """P = 1: pmmh_checks.models(1), the transition coefficient.  P = 2: (a, sy) — the OBSERVATION scale is a parameter, so
    the observation term depends on theta and the refresh of ref_lw is exercised."""
    if P == 1:
        return M.models(1)
    import genjax_amd as G
    from genjax_amd import workloads
    p = workloads.LGSSM
    s0, sx = p["s0"], p["sx"]

    @G.gen
    def init(a, sy):
        x = G.normal(0.0, s0) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x

    @G.gen
    def step(x_prev, a, sy):
        x = G.normal(a * x_prev, sx) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x

    @G.gen
    def prior():
        a = G.uniform(PRIOR[0][0], PRIOR[0][1]) @ "a"
        _ = G.uniform(PRIOR[1][0], PRIOR[1][1]) @ "sy"
        return a
    return init, step, prior, ("a", "sy")


def _data(T):
    from genjax_amd import workloads
    return torch.from_numpy(workloads.lgssm_data(T))


def make_chain(chain, specialize, max_iters=ITERS):
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleGibbs
    case, ancestors, backward = chain
    R, n, T, P = CASES[case]
    init, step, prior, addrs = models(P)
    pg = ParticleGibbs(init, step, prior, n, R, T, addrs, STEP_SIZE[:P], ancestor_sampling=ancestors, backward=backward,
                       specialize=specialize)
    th0 = start_of(R, P, seed=2)
    return pg.prepare(G.key(SEED), _data(T), tuple(torch.from_numpy(th0[p].copy()) for p in range(P)), max_iters)


def snapshot(pg, res):
    """everything the run comparisons hold equal: the records, the draws, the final state, the bank's tables and pins"""
    th, lj, x = pg.state()
    out = dict(theta=_np(res.theta), log_joint=_np(res.log_joint), accepted=_np(res.accepted), paths=_np(res.paths),
               s_theta=_np(th), s_lj=_np(lj), s_x=_np(x), keys_prop=_np(pg.bank.keys_prop), keys_res=_np(pg.bank.keys_res),
               ref_lw=_np(pg.bank.ref_lw), ref_x=_np(pg.bank.ref_x), theta_pair=_np(pg.theta_pair), joint=_np(pg.joint),
               obs=_np(pg.obs), lp=_np(pg.lp), leaves=np.stack([_np(v) for v in pg.bank.params_full]))
    if pg.bank.ancestor_sampling:
        out["keys_as"] = _np(pg.bank.keys_as)
    return out


def assert_same_run(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = a[k], b[k]
        same = same64(x, y) if x.dtype == np.float64 else (H.same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y))
        assert same, (what, k)


@functools.lru_cache(maxsize=None)
def run_of(device_type, chain, specialize):
    """ParticleGibbs.run(6, paths=True) of a chain case, once per backend (never modified)"""
    pg = make_chain(chain, specialize)
    return snapshot(pg, pg.run(ITERS, paths=True))


# --- the chain is the composition ------------------------------------------------------------------------------------------------
def public_scores(be, init, step, prior, addrs, x, theta, ys):
    """joint [T, R], obs [T, R], lp [R] (float32) of the paths x [R, T] under theta [P, R], by the public init.assess /
    step.assess / prior.assess over a batch of R and the observation term through importance + project"""
    import genjax_amd as G
    from genjax_amd.core.choice_map import ChoiceMap, Selection
    R, T = x.shape
    dev = be.device
    th = tuple(torch.from_numpy(theta[p].copy()).to(dev) for p in range(theta.shape[0]))
    xs = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)                    # [T, R]
    keys = G.split(G.key(0), R)                                                 # (nothing is left to draw)
    joint, obs = np.empty((T, R), np.float32), np.empty((T, R), np.float32)
    for t in range(T):
        con = ChoiceMap.empty().set("y", ys[t].to(dev).float()).set("x", xs[t])
        model, args = (init, th) if t == 0 else (step, (xs[t - 1],) + th)
        joint[t] = _np(model.assess(con, args, batch_shape=(R,))[0]).astype(np.float32).reshape(R)
        tr, _w = model.importance(keys, con, args)
        from genjax_amd import engine
        obs[t] = _np(engine.materialize(model.project(keys, tr, Selection.at["y"]))).reshape(R)
    con = ChoiceMap.empty()
    for p, a in enumerate(addrs):
        con = con.set(a, th[p])
    lp = _np(prior.assess(con, (), batch_shape=(R,))[0]).astype(np.float32).reshape(R)
    return joint, obs, lp


@functools.lru_cache(maxsize=None)
def composed_chain(device_type, chain, specialize):
    """The same chain as a Python loop over public parts, once per backend: per iteration a fresh
    ConditionalBank(params=theta_j).prepare(split(k_sweep, R), ys, retained=x_{j-1}), launch(), draw(k_draw, backward); the
    public assess calls under theta_j and theta'_j; sequential float64 sums; the decision by the host helpers.  Asserts that
    no decision is a near-tie."""
    import genjax_amd as G
    from genjax_amd import _lib
    from genjax_amd.inference.smc import ConditionalBank
    be = _lib.get()
    case, ancestors, backward = chain
    R, n, T, P = CASES[case]
    init, step, prior, addrs = models(P)
    run_key = G.key(SEED)
    key = np.asarray(run_key.host(), np.uint32)
    ys = _data(T)
    theta = start_of(R, P, seed=2)
    scale = np.asarray(STEP_SIZE[:P], np.float32)
    x_prev, out = None, []
    for j in range(ITERS):
        _ks, _kd, k_prop, k_acc = iter_keys(key, j)
        ks = G.split(G.fold_in(run_key, j), 4)
        bank = ConditionalBank(init, step, n, R, T, params=tuple(torch.from_numpy(theta[p].copy()) for p in range(P)),
                               ancestor_sampling=ancestors, specialize=specialize)
        bank.prepare(G.split(ks[0], R), ys, retained=x_prev)
        pins = _np(bank.ref_lw).copy()                       # set_retained(x_{j-1}) under theta_j
        bank.launch()
        x = bank.draw(ks[1], backward=backward).clone()      # [R, T]
        xh = _np(x)
        th1 = M.proposals(be, k_prop, 1, theta, scale)
        j0, o0, l0 = public_scores(be, init, step, prior, addrs, xh, theta, ys)
        j1, o1, l1 = public_scores(be, init, step, prior, addrs, xh, th1, ys)
        joint, lp = np.concatenate([j0, j1], axis=1), np.concatenate([l0, l1])
        take, S = decide(be, k_acc, joint, lp, (chain, j))
        col = np.where(take, np.arange(R) + R, np.arange(R))
        theta = np.where(take[None, :], th1, theta)
        with np.errstate(invalid="ignore"):
            lj = S[col] + lp[col].astype(np.float64)
        out.append(dict(x=xh, theta_prop=th1, take=take, theta=theta.copy(), log_joint=lj, ref_lw=np.where(take[None, :], o1, o0),
                        pins=pins, outside=np.isneginf(l1), refreshed=take & np.any(o0 != o1, axis=0)))
        x_prev = x
    return out


def check_chain_is_the_composition(be, chain, specialize):
    case, _ancestors, _backward = chain
    R, n, T, P = CASES[case]
    want = composed_chain(be.device.type, chain, specialize)
    takes = np.stack([w["take"] for w in want])
    print("composed chain", chain_id(chain), ": accepted", int(takes.sum()), "of", takes.size, "; proposals outside the prior",
          int(sum(w["outside"].sum() for w in want)))
    assert takes.any() and not takes.all()
    pg = make_chain(chain, specialize)
    for j, w in enumerate(want):
        if j > 0:
            # what the move left in the bank IS what set_retained computes under the accepted theta
            assert H.same_bits(_np(pg.bank.ref_lw), w["pins"]), (chain, j, "ref_lw against set_retained under the accepted theta")
        res = pg.run(1, paths=True)
        assert H.same_bits(_np(res.paths)[0], w["x"]), (chain, j, "the drawn paths")
        assert H.same_bits(_np(pg.theta_pair)[:, R:], w["theta_prop"]), (chain, j, "theta'")
        assert np.array_equal(_np(res.accepted)[0], w["take"]), (chain, j, "decisions", _np(res.accepted)[0], w["take"])
        assert H.same_bits(_np(res.theta)[0], w["theta"]), (chain, j, "theta")
        assert same64(_np(res.log_joint)[0], w["log_joint"]), (chain, j, "log_joint", _np(res.log_joint)[0], w["log_joint"])
        assert H.same_bits(_np(pg.bank.ref_lw), w["ref_lw"]), (chain, j, "ref_lw")
        assert H.same_bits(_np(pg.bank.ref_x)[:, 0, :].T, w["x"]), (chain, j, "the retained paths")
    if P == 2:
        assert any(w["refreshed"].any() for w in want), "no accepted move changed the observation term: the refresh of ref_lw was not exercised"
    th, lj, x = pg.state()
    assert H.same_bits(_np(th), want[-1]["theta"]) and same64(_np(lj), want[-1]["log_joint"]) and H.same_bits(_np(x), want[-1]["x"])
    # run(6) in one go, and run(2) + run(4): the same records and the same final state, bit for bit
    whole = run_of(be.device.type, chain, specialize)
    assert np.array_equal(whole["accepted"], takes) and H.same_bits(whole["theta"], np.stack([w["theta"] for w in want]))
    assert H.same_bits(whole["paths"], np.stack([w["x"] for w in want]))
    pg = make_chain(chain, specialize)
    first, second = pg.run(2, paths=True), pg.run(4, paths=True)
    parts = types.SimpleNamespace(**{k: torch.cat([getattr(first, k), getattr(second, k)]) for k in ("theta", "log_joint", "accepted", "paths")})
    assert_same_run(snapshot(pg, parts), whole, (chain, "run(2) + run(4) against run(6)"))
    assert pg.run(0).paths is None
    import pytest
    with pytest.raises(ValueError, match="max_iters"):
        pg.run(1)


def check_captured(be, chain, specialize=True):
    """capture() after iteration 0 captures the conditional sweep; the replays agree with the uncaptured run bit for bit"""
    whole = run_of(be.device.type, chain, specialize)
    pg = make_chain(chain, specialize)
    first = pg.run(1, paths=True)
    before = [t.clone() for t in (pg.theta, pg.log_joint, pg.bank.ref_lw, pg.bank.ref_x)]
    pg.capture()
    assert pg.bank.graph is not None and pg.bank.conditional
    for was, now in zip(before, (pg.theta, pg.log_joint, pg.bank.ref_lw, pg.bank.ref_x)):
        assert same64(_np(was), _np(now)) if was.dtype == torch.float64 else H.same_bits(_np(was), _np(now))
    second = pg.run(ITERS - 1, paths=True)
    assert pg.bank.graph is not None
    parts = types.SimpleNamespace(**{k: torch.cat([getattr(first, k), getattr(second, k)]) for k in ("theta", "log_joint", "accepted", "paths")})
    assert_same_run(snapshot(pg, parts), whole, (chain, "captured"))


def check_device_is_the_mirror(be, chain):
    """every record, the draws, the final state, the key tables and the pins of the device equal the mirror's"""
    import genjax_amd as G
    import tests.hostsim as hs
    from genjax_amd import _lib
    assert be.device.type == "cuda"
    got = run_of("cuda", chain, True)
    G.clear_caches()
    hs.install()
    try:
        pg = make_chain(chain, specialize=False)
        want = snapshot(pg, pg.run(ITERS, paths=True))
    finally:
        hs.uninstall()
        G.clear_caches()
        _lib.install(None)
    assert_same_run(got, want, (chain, "device against mirror"))


# --- states of more than one component -----------------------------------------------------------------------------------------------
def check_state_shapes(be):
    """a vector state (the binding of its strided [2R, D] leaf is not kept) and a tuple state: after every iteration the pins
    are what a fresh bank's set_retained(state()'s paths) computes under the chains' theta, and the paths round-trip"""
    import genjax_amd as g
    import genjax_amd.numpy as jnp
    from genjax_amd.inference.smc import ConditionalBank, ParticleGibbs

    def tracker(stack, at):
        @g.gen
        def init(sy):
            p = g.normal(0.0, 1.0) @ "p"
            v = g.normal(0.0, 0.5) @ "v"
            g.normal(p, sy) @ "y"
            return stack(p, v)

        @g.gen
        def step(s, sy):
            p = g.normal(at(s, 0) + 0.1 * at(s, 1), 0.05) @ "p"
            v = g.normal(at(s, 1), 0.1) @ "v"
            g.normal(p, sy) @ "y"
            return stack(p, v)
        return init, step

    @g.gen
    def prior():
        return g.uniform(0.1, 2.0) @ "sy"
    R, n, T = 5, 16, 4
    forms = (("vector", tracker(lambda a, b: jnp.stack([a, b]), lambda s, d: s[..., d])),
             ("tuple", tracker(lambda a, b: (a, b), lambda s, d: s[d])))
    for name, (init, step) in forms:
        pg = ParticleGibbs(init, step, prior, n, R, T, ("sy",), (0.2,), state_sites=("p", "v"), specialize=False)
        pg.prepare(g.key(5), _data(T), (torch.linspace(0.3, 0.9, R),), 4)
        for j in range(4):
            res = pg.run(1, paths=True)
            th, _lj, x = pg.state()
            last = tuple(v[0] for v in res.paths) if name == "tuple" else res.paths[0]
            for a, b in zip(x if name == "tuple" else (x,), last if name == "tuple" else (last,)):
                assert tuple(a.shape) == ((R, T) if name == "tuple" else (R, T, 2)) and H.same_bits(_np(a), _np(b)), (name, j)
            cb = ConditionalBank(init, step, n, R, T, params=(th[0].clone(),), state_sites=("p", "v"), specialize=False)
            cb.prepare(g.split(g.key(1), R), _data(T), retained=x)
            assert H.same_bits(_np(cb.ref_lw), _np(pg.bank.ref_lw)) and H.same_bits(_np(cb.ref_x), _np(pg.bank.ref_x)), (name, j)
        assert _np(pg.rec_acc).any()
    with __import__("pytest").raises(NotImplementedError, match="state_sites="):
        ParticleGibbs(init, step, prior, n, R, T, ("sy",), (0.2,), specialize=False).prepare(g.key(5), _data(T), (torch.linspace(0.3, 0.9, R),), 4)


# --- the API's refusals -----------------------------------------------------------------------------------------------------------
def check_api_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleGibbs
    init, step, prior, addrs = models(2)
    R, n, T = 3, 8, 2
    ys = _data(T)
    th0 = tuple(torch.from_numpy(start_of(R, 2)[p].copy()) for p in range(2))

    def make(**kw):
        a = dict(init=init, step=step, prior=prior, n_particles=n, n_chains=R, T=T, param_addrs=addrs, step_size=STEP_SIZE,
                 specialize=False)
        a.update(kw)
        return ParticleGibbs(**a)
    pg = make()
    with pytest.raises(ValueError, match="ParticleGibbs.prepare takes ONE key"):
        pg.prepare(G.split(G.key(1), R), ys, th0, 4)
    for bad in (th0[:1], (th0[0], th0[1][:2]), (th0[0].reshape(1, R), th0[1])):
        with pytest.raises(ValueError, match="ParticleGibbs.prepare: theta0"):
            pg.prepare(G.key(1), ys, bad, 4)
    for bad in ((0.1,), (0.1, 0.0), (0.1, -0.2), (0.1, math.nan), 0.1):
        with pytest.raises(ValueError, match="ParticleGibbs: step_size"):
            make(step_size=bad)
    with pytest.raises(NotImplementedError, match="ParticleGibbs: 9 parameters; param_addrs names between 1 and 8"):
        make(param_addrs=tuple("p%d" % i for i in range(9)), step_size=(0.1,) * 9)
    with pytest.raises(NotImplementedError, match="between 1 and 8"):
        make(param_addrs=(), step_size=())
    with pytest.raises(ValueError, match="ParticleGibbs: param_addrs = .* names a site twice"):
        make(param_addrs=("a", "a"))
    _i1, _s1, prior1, _a1 = models(1)
    with pytest.raises(ValueError, match="ParticleGibbs: the prior's sites are not exactly param_addrs"):      # no site "sy"
        make(prior=prior1).prepare(G.key(1), ys, th0, 4)
    with pytest.raises(ValueError, match="ParticleGibbs: the prior's sites are not exactly param_addrs"):      # "sy" is no parameter
        i1, s1, _p1, a1 = models(1)
        ParticleGibbs(i1, s1, prior, n, R, T, a1, STEP_SIZE[:1], specialize=False).prepare(G.key(1), ys, th0[:1], 4)

    @G.gen
    def step_extra_site(x_prev, a, sy):
        z = G.normal(0.0, 1.0) @ "z"
        x = G.normal(a * x_prev + 0.0 * z, 0.5) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x
    with pytest.raises(NotImplementedError, match="ParticleGibbs: the step model samples 'z'"):
        make(step=step_extra_site).prepare(G.key(1), ys, th0, 4)
    for bad in (0, 2 ** 32):
        with pytest.raises(ValueError, match="ParticleGibbs.prepare: max_iters"):
            pg.prepare(G.key(1), ys, th0, bad)
    with pytest.raises(RuntimeError, match="prepare"):
        make().run(1)
    pg.prepare(G.key(1), ys, th0, 2)
    pg.run(2)
    with pytest.raises(ValueError, match="ParticleGibbs.run: 2 iterations done and 1 asked for, past max_iters = 2"):
        pg.run(1)
    # whatever ConditionalBank refuses is refused by it, by name
    with pytest.raises(NotImplementedError, match="ConditionalBank: ess_threshold="):
        make(ess_threshold=0.5)
    for kind in ("systematic", "stratified"):
        with pytest.raises(NotImplementedError, match="ConditionalBank\\(resample='%s'\\)" % kind):
            make(resample=kind)
    with pytest.raises(ValueError, match="BootstrapBank: n_particles, n_filters and T must be positive"):
        make(n_chains=0)
    with pytest.raises(NotImplementedError, match="BootstrapBank: n_particles = 2097153 > 2\\^21"):
        make(n_particles=2 ** 21 + 1)
    with pytest.raises(NotImplementedError, match="BootstrapBank: R \\* n >= 2\\^31"):
        make(n_particles=2 ** 21, n_chains=1024)
    with pytest.raises(ValueError, match="ParticleGibbs: state_sites names 2 addresses for a state of 1 components"):
        make(state_sites=("x", "z")).prepare(G.key(1), ys, th0, 4)
    with pytest.raises(NotImplementedError, match="BootstrapBank.prepare: per-filter observations"):
        make().prepare(G.key(1), torch.zeros((R, T)), th0, 4)
    with pytest.raises(ValueError, match="ConditionalBank.set_retained: the retained paths are"):
        make().prepare(G.key(1), ys, th0, 4, retained=torch.zeros((R, T + 1)))
    with pytest.raises(NotImplementedError, match="ConditionalBank\\(ancestor_sampling=True\\): the step model samples 'z'"):
        make(step=step_extra_site, ancestor_sampling=True).prepare(G.key(1), ys, th0, 4)


# --- the law ---------------------------------------------------------------------------------------------------------------------
LAW_R, LAW_N, LAW_T, LAW_ITERS, LAW_STEP, LAW_SEED = M.LAW_R, 8, M.LAW_T, 60, 0.15, 778


def numpy_pgibbs_reference(seed=1, n=LAW_N, iters=LAW_ITERS):
    """The same design in float64 numpy with numpy's own generator — multinomial conditional SMC (slot n - 1 pinned, the new
    path drawn from the final weights and traced through the ancestors), then the random-walk move of the coefficient given
    the path: the coefficient of the R chains after `iters` iterations.  What says that 60 iterations at this step size leave
    no burn-in bias the bound could see."""
    from genjax_amd import workloads
    p = workloads.LGSSM
    ys = workloads.lgssm_data(LAW_T).astype(np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = M.PRIOR[0]
    R, T = LAW_R, LAW_T
    rows = np.arange(R)

    def sweep(a, ref):
        xs, ancs = np.empty((T, R, n)), np.empty((T, R, n), np.int64)
        x = p["s0"] * rng.normal(size=(R, n))
        for t in range(T):
            if t > 0:
                x = a[:, None] * np.take_along_axis(x, ancs[t - 1], axis=1) + p["sx"] * rng.normal(size=(R, n))
            if ref is not None:
                x[:, n - 1] = ref[:, t]
            xs[t] = x
            lw = -0.5 * ((ys[t] - x) / p["sy"]) ** 2
            c = np.cumsum(np.exp(lw - lw.max(axis=1, keepdims=True)), axis=1)
            u = rng.uniform(size=(R, n)) * c[:, -1:]
            ancs[t] = np.minimum((c[:, None, :] < u[:, :, None]).sum(axis=2), n - 1)
            if ref is not None:
                ancs[t][:, n - 1] = n - 1
        k = ancs[T - 1][:, 0]                # (slot 0's draw from the final weights: one multinomial pick per chain)
        path = np.empty((R, T))
        for t in range(T - 1, -1, -1):
            path[:, t] = xs[t][rows, k]
            if t > 0:
                k = ancs[t - 1][rows, k]
        return path

    def transition(a, x):
        return (-0.5 * ((x[:, 1:] - a[:, None] * x[:, :-1]) / p["sx"]) ** 2).sum(axis=1)
    a = M.law_start().astype(np.float64)
    ref, taken = None, 0
    for _ in range(iters):
        ref = sweep(a, ref)
        prop = a + LAW_STEP * rng.normal(size=(R,))
        inside = (prop >= lo) & (prop <= hi)
        take = inside & (np.log(rng.uniform(size=(R,))) < transition(np.where(inside, prop, a), ref) - transition(a, ref))
        a = np.where(take, prop, a)
        taken += int(take.sum())
    return a, taken / (iters * R)


def check_numpy_reference():
    a, rate = numpy_pgibbs_reference()
    z1, z2 = M.law_z_scores(a)
    print("numpy particle Gibbs: acceptance rate", rate, "z of the mean", z1, "z of the second moment", z2)
    assert abs(z1) <= 3.0 and abs(z2) <= 3.0, (z1, z2)


def check_law(be, specialize=True):
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleGibbs
    init, step, prior, addrs = models(1)
    pg = ParticleGibbs(init, step, prior, LAW_N, LAW_R, LAW_T, addrs, (LAW_STEP,), specialize=specialize)
    pg.prepare(G.key(LAW_SEED), _data(LAW_T), (torch.from_numpy(M.law_start()),), LAW_ITERS)
    res = pg.run(LAW_ITERS)
    a_last = _np(res.theta)[-1, 0]
    lo, hi = M.PRIOR[0]
    assert np.all((a_last >= lo) & (a_last <= hi))
    z1, z2 = M.law_z_scores(a_last)
    print("law: acceptance rate", float(_np(res.accepted).mean()), "exact posterior (mean, sd, second moment, its sd)",
          M.exact_posterior(), "z of the mean", z1, "z of the second moment", z2)
    assert abs(z1) <= 5.0 and abs(z2) <= 5.0, (z1, z2)
