"""Shared drivers of tests/test_history_cpu.py (the C-ABI's CPU mirror) and tests/test_history_gpu.py (the HIP
library): BootstrapSweep(history=True), gmx_history_record and gmx_lineage against the CPU oracle and numpy loops.
Comparisons are bit for bit (float arrays through their int32 views)."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import genjax_oracle as O

KINDS = {"systematic": O.SYSTEMATIC, "stratified": O.STRATIFIED, "multinomial_tiled": O.MULTINOMIAL_TILED,
         "multinomial_sorted": O.MULTINOMIAL_SORTED}
LGSSM_N, LGSSM_T, LGSSM_SEED = 2051, 5, 2718        # two full 1024-particle tiles + a 3-particle one; n % 4 = 3


def bits(a):
    """an array's words: torch or numpy, float32 or int32"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.int32), a.dtype
    return a.view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


@functools.lru_cache(maxsize=None)
def lgssm_oracle(resample, n=LGSSM_N, T=LGSSM_T, seed=LGSSM_SEED):
    """the oracle's sweep, once per resampler kind (shared by every test that needs it; never modified)"""
    from genjax_amd import workloads
    from tests import parity
    oi, os_ = workloads.make_lgssm(O)
    return parity.oracle_bootstrap_sweep(oi, os_, n, T, workloads.lgssm_data(T), O.key(seed), kind=KINDS[resample])


def run_lgssm(history, fuse, noise_ahead, capture, specialize, resample, n=LGSSM_N, T=LGSSM_T, seed=LGSSM_SEED):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T, specialize=specialize, resample=resample, noise_ahead=noise_ahead,
                        fuse_resample=fuse, history=history).prepare(G.key(seed), torch.from_numpy(workloads.lgssm_data(T)))
    assert sw.fuse == fuse, "the sweep did not take the requested (one- / two-launch) form"
    assert sw.noise_ahead == noise_ahead, "the sweep did not take the requested (one- / two-stream) form"
    if capture:
        sw.capture()
        sw.launch()              # two replays: the second must record the same history
    sw.launch()
    return sw


def check_lgssm_record(fuse, noise_ahead, capture, specialize, resample):
    """every step of the record equals the oracle's; log_ml() and state() equal those of the same sweep without history"""
    ref = lgssm_oracle(resample)
    sw = run_lgssm(True, fuse, noise_ahead, capture, specialize, resample)
    h = sw.history()
    assert tuple(h.x.shape) == tuple(h.log_weights.shape) == tuple(h.ancestors.shape) == (LGSSM_T, LGSSM_N)
    assert h.ancestors.dtype == torch.int32
    for t, r in enumerate(ref["hist"]):
        assert same_bits(h.x[t], r["x"]), ("x", t)
        assert same_bits(h.log_weights[t], r["lw"]), ("lw", t)
        assert same_bits(h.ancestors[t], np.asarray(r["anc"]).astype(np.int32)), ("anc", t)
    plain = run_lgssm(False, fuse, noise_ahead, capture, specialize, resample)
    assert plain.hist_xs is None and plain.hist_status is None          # nothing allocated
    assert sw.log_ml() == plain.log_ml()
    for a, b in zip(sw.state(), plain.state()):
        assert same_bits(a, b.cpu().numpy())
    assert same_bits(h.ancestors[LGSSM_T - 1], sw.state()[2].cpu().numpy())
    return sw, h


# --- the vector-state and tuple-state models of tests/parity.py (check_vector_state_sweep, check_tuple_state_sweep) ---
def make_tracker(g, stack):
    @g.gen
    def init():
        p = g.normal(0.0, 1.0) @ "p"
        v = g.normal(0.0, 0.5) @ "v"
        g.normal(p, 0.3) @ "y"
        return stack(p, v)

    @g.gen
    def step(s):
        p = g.normal(s[..., 0] + 0.1 * s[..., 1], 0.05) @ "p"
        v = g.normal(s[..., 1], 0.1) @ "v"
        g.normal(p, 0.3) @ "y"
        return stack(p, v)
    return init, step


def make_pair(g):
    @g.gen
    def init():
        a = g.normal(0.0, 1.0) @ "a"
        b = g.normal(a, 1.0) @ "b"
        g.normal(a + b, 1.0) @ "y"
        return (a, b)

    @g.gen
    def step(s):
        a0, b0 = s
        a = g.normal(0.9 * a0, 0.5) @ "a"
        b = g.normal(0.5 * b0 + 0.1 * a, 0.5) @ "b"
        c = g.normal(0.0, 1.0) @ "c"
        g.normal((a + b) + 0.1 * c, 1.0) @ "y"
        return (a, b)
    return init, step


STATE_N, STATE_T, STATE_SEED = 1027, 4, 17


@functools.lru_cache(maxsize=None)
def state_oracle(which):
    """step-by-step oracle loop (the style of parity.check_tuple_state_sweep) keeping every step: x as [D, n] rows"""
    n, T, seed = STATE_N, STATE_T, STATE_SEED
    ys = state_data()
    oi, os_ = make_pair(O) if which == "tuple" else make_tracker(O, lambda a, b: np.stack([a, b], axis=-1))
    hist, x, anc = [], None, None
    for t in range(T):
        ks = O.split(O.fold_in(O.key(seed), t), 3)
        keys = O.split(ks[0], n)
        obs = O.C.d({"y": np.float32(ys[t])})
        if t == 0:
            tr, w = oi.importance(keys, obs, ())
        elif which == "tuple":
            tr, w = os_.importance(keys, obs, (tuple(v[anc] for v in x),))
        else:
            tr, w = os_.importance(keys, obs, (x[anc],))
        rv = tr.get_retval()
        x = tuple(np.asarray(v, np.float32) for v in rv) if which == "tuple" else np.asarray(rv, np.float32)
        lw = np.asarray(w, np.float32)
        cdf, total, M, shift = O.weight_cdf(lw)
        anc = O.ancestors(O.SYSTEMATIC, ks[1], cdf)
        rows = np.stack(x) if which == "tuple" else np.ascontiguousarray(x.T)
        hist.append(dict(rows=rows, lw=lw, anc=np.asarray(anc).astype(np.int32)))
    return hist


def state_data():
    return np.random.default_rng(STATE_SEED).normal(size=STATE_T).astype(np.float32)


def check_state_record(which, capture=False, **kw):
    """a vector [n, 2] state / a tuple of two scalars: the record and the trajectories against the oracle loop"""
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd.inference.smc import BootstrapSweep
    n, T = STATE_N, STATE_T
    init, step = make_pair(G) if which == "tuple" else make_tracker(G, lambda a, b: jnp.stack([a, b]))
    sw = BootstrapSweep(init, step, n, T, history=True, **kw).prepare(G.key(STATE_SEED), torch.from_numpy(state_data()))
    if capture:
        sw.capture()
        sw.launch()
    sw.launch()
    h, ref = sw.history(), state_oracle(which)
    if which == "tuple":
        assert isinstance(h.x, tuple) and len(h.x) == 2 and all(tuple(v.shape) == (T, n) for v in h.x)
        got = lambda t, d: h.x[d][t]
    else:
        assert tuple(h.x.shape) == (T, n, 2)
        got = lambda t, d: h.x[t, :, d]
    for t, r in enumerate(ref):
        for d in range(2):
            assert same_bits(got(t, d), r["rows"][d]), ("x", t, d)
        assert same_bits(h.log_weights[t], r["lw"]) and same_bits(h.ancestors[t], r["anc"]), t
    # trajectories of the survivors: a numpy walk over the oracle's steps
    paths, traj = numpy_lineage(np.stack([r["anc"] for r in ref]), np.stack([r["rows"] for r in ref]), ref[-1]["anc"])
    assert same_bits(h.lineage(), paths)
    tj = h.trajectories()
    if which == "tuple":
        assert isinstance(tj, tuple) and all(tuple(v.shape) == (n, T) for v in tj)
        for d in range(2):
            assert same_bits(tj[d], traj[:, d, :].T)
    else:
        assert tuple(tj.shape) == (n, T, 2)
        assert same_bits(tj, traj.transpose(2, 0, 1))
    fm = h.filter_mean()
    assert fm.dtype == torch.float64 and tuple(fm.shape) == (T, 2)
    return sw


# --- gmx_history_record alone ------------------------------------------------------------------------------------------
def check_record_alone(be, D, n, mode):
    """one call on made-up rows; every destination row starts ONE element into its buffer (misaligned for 16-byte
    stores) and the words before and after each row must stay as they were"""
    dev = be.device
    rng = np.random.default_rng(1000 * D + n)
    x = rng.normal(size=(D, n)).astype(np.float32)
    lw = rng.normal(size=n).astype(np.float32)
    idx = rng.integers(0, n, size=n).astype(np.int32)
    tag, expect = {"plain": (0, 0), "tagged": (7, 7), "stale": (7, 8)}[mode]
    words = (idx.astype(np.uint32) | np.uint32(tag << 24)).view(np.int32)
    GUARD = 0x5A5A5A5A
    x_buf = torch.full((D * n + 2,), GUARD, dtype=torch.int32, device=dev)
    lw_buf = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
    anc_buf = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    src = [torch.from_numpy(a).to(dev) for a in (x, lw, words)]
    rc = be.c.gmx_history_record(be.ptr(src[0]), D, be.ptr(src[1]), be.ptr(src[2]), n, expect,
                                 be.ptr(x_buf[1:]), be.ptr(lw_buf[1:]), be.ptr(anc_buf[1:]), be.ptr(status), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    for buf in (x_buf, lw_buf, anc_buf):
        assert int(buf[0]) == GUARD and int(buf[-1]) == GUARD
    assert same_bits(x_buf[1:-1].reshape(D, n), x)
    assert same_bits(lw_buf[1:-1], lw)
    assert same_bits(anc_buf[1:-1], idx)             # plain: as they were; tagged: stripped to the index
    assert int(status.item()) == (n if mode == "stale" else 0)


# --- gmx_lineage against a numpy loop ------------------------------------------------------------------------------------
def numpy_lineage(anc, xs, start):
    """anc [T, n], xs [T, D, n], start [m] -> paths [T, m], traj [T, D, m]"""
    T, D, _ = xs.shape
    m = len(start)
    paths = np.zeros((T, m), np.int32)
    traj = np.zeros((T, D, m), np.float32)
    p = np.asarray(start).astype(np.int64)
    for t in range(T - 1, -1, -1):
        paths[t] = p
        traj[t] = xs[t][:, p]
        if t:
            p = anc[t - 1][p].astype(np.int64)
    return paths, traj


def lineage_inputs(T, D, n, m):
    rng = np.random.default_rng(T * 1000003 + D * 10007 + n * 31 + m)
    anc = rng.integers(0, n, size=(T, n)).astype(np.int32)          # uniform, NOT sorted: nothing leans on monotone rows
    xs = rng.normal(size=(T, D, n)).astype(np.float32)
    mark = rng.random(size=xs.shape)
    xs[mark < 0.1] = np.float32("nan")                              # a tenth NaN, a tenth -0.0: they must come through
    xs[mark > 0.9] = np.float32(-0.0)                               # with their bits
    start = rng.integers(0, n, size=m).astype(np.int32)
    start[0], start[-1] = 0, n - 1                                  # (m = 1: n - 1)
    xs[T - 1, 0, start[0]] = np.float32("nan")
    return anc, xs, start


def call_lineage(be, anc, xs, start, want_paths=True, want_traj=True):
    dev = be.device
    T, D, n = xs.shape
    m = len(start)
    a_d, x_d, s_d = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (anc, xs, start))
    paths = torch.full((T, m), -7, dtype=torch.int32, device=dev) if want_paths else None
    traj = torch.full((T, D, m), 7.0, dtype=torch.float32, device=dev) if want_traj else None
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_lineage(be.ptr(a_d), be.ptr(x_d) if want_traj else None, T, D, n, be.ptr(s_d), m, be.ptr(paths),
                          be.ptr(traj), be.ptr(status), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return paths, traj, int(status.item())


def check_lineage(be, T, D, n, m):
    anc, xs, start = lineage_inputs(T, D, n, m)
    ref_p, ref_t = numpy_lineage(anc, xs, start)
    paths, traj, st = call_lineage(be, anc, xs, start)
    assert st == 0 and same_bits(paths, ref_p) and same_bits(traj, ref_t)
    paths, traj, st = call_lineage(be, anc, xs, start, want_traj=False)
    assert st == 0 and traj is None and same_bits(paths, ref_p)
    paths, traj, st = call_lineage(be, anc, xs, start, want_paths=False)
    assert st == 0 and paths is None and same_bits(traj, ref_t)
    assert np.isnan(ref_t).any()                       # (the inputs do carry what the test is about)
    if ref_t.size > 100:
        assert (np.signbit(ref_t) & (ref_t == 0)).any()


def check_lineage_out_of_range(be):
    """start holds n and -1: clamped before any read (status 2 from the C call, IndexError from Python); the clamped
    walks are those of n - 1 and 0"""
    import pytest
    from genjax_amd.inference.smc import SweepHistory
    T, D, n, m = 5, 2, 1027, 6
    anc, xs, start = lineage_inputs(T, D, n, m)
    start[2], start[4] = n, -1
    fixed = start.copy()
    fixed[2], fixed[4] = n - 1, 0
    ref_p, ref_t = numpy_lineage(anc, xs, fixed)
    paths, traj, st = call_lineage(be, anc, xs, start)
    assert st == 2 and same_bits(paths, ref_p) and same_bits(traj, ref_t)
    dev = be.device
    h = SweepHistory(torch.from_numpy(xs).to(dev), torch.zeros((T, n), device=dev), torch.from_numpy(anc).to(dev), (D,))
    with pytest.raises(IndexError):
        h.lineage(torch.from_numpy(start))
    with pytest.raises(IndexError):
        h.trajectories(torch.from_numpy(start).long())
    assert same_bits(h.lineage(torch.from_numpy(fixed).long()), ref_p)          # any int tensor


def check_end_to_end(sw, h, resample="systematic"):
    """trajectories() of the LGSSM sweep = a numpy walk over the oracle's steps; its last column is x[T-1][anc[T-1]]"""
    ref = lgssm_oracle(resample)["hist"]
    anc = np.stack([np.asarray(r["anc"]).astype(np.int32) for r in ref])
    xs = np.stack([r["x"][None, :] for r in ref])
    paths, traj = numpy_lineage(anc, xs, anc[-1])
    assert same_bits(h.lineage(), paths)
    tj = h.trajectories()
    assert tuple(tj.shape) == (LGSSM_N, LGSSM_T)
    assert same_bits(tj, traj[:, 0, :].T)
    last = h.x[LGSSM_T - 1][h.ancestors[LGSSM_T - 1].long()]
    assert same_bits(tj[:, LGSSM_T - 1], last)
    some = torch.tensor([0, 5, LGSSM_N - 1, 5])
    assert same_bits(h.trajectories(some), numpy_lineage(anc, xs, some.numpy())[1][:, 0, :].T)


def check_filter_mean(h):
    """filter_mean() against numpy float64 on the same float32 arrays.

    Both sides compute sum_i w_i x_i with w = softmax(lw) in float64 from identical inputs, so they differ by rounding
    only: the weights are non-negative and sum to 1 (each to a few units of 2^-53 relative), every product w_i x_i is
    rounded once, and a float64 sum of n terms in ANY order is within (n - 1) * 2^-53 * sum_i |w_i x_i| of the exact one
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order).  With sum_i |w_i x_i| <= max|x_t|
    the two results are each within about (n + 5) * 2^-53 * max|x_t| of the exact mean, hence within
    n * 2^-52 * max|x_t| of each other for n >= 5."""
    lw = h.log_weights.cpu().numpy().astype(np.float64)
    xs = h._xs.cpu().numpy().astype(np.float64)          # [T, D, n]
    T, D, n = xs.shape
    e = np.exp(lw - lw.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    ref = np.einsum("tn,tdn->td", w, xs)
    got = h.filter_mean().cpu().numpy().reshape(T, D)
    bound = n * 2.0 ** -52 * np.abs(xs).max(axis=(1, 2))
    err = np.abs(got - ref).max(axis=1)
    print("filter_mean: max |torch - numpy| per step", err, "bound", bound)
    assert np.all(err <= bound), (err, bound)


def history_refusal_calls():
    """(entry point, argument tuple, what the message has to name): what gmx_history_record and gmx_lineage refuse before
    any launch"""
    import ctypes
    N, i64, i32, u32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    buf = (ctypes.c_int64 * 8)()
    B = ctypes.cast(buf, ctypes.c_void_p)
    calls = [
        ("gmx_history_record", (N, i32(1), N, N, i64(10), u32(0), N, N, N, N, N), b"null argument"),
        ("gmx_history_record", (B, i32(0), B, B, i64(10), u32(0), B, B, B, B, N), b"D = 0"),
        ("gmx_history_record", (B, i32(1), B, B, i64(0), u32(0), B, B, B, B, N), b"n = 0"),
        ("gmx_history_record", (B, i32(1), B, B, i64(4), u32(3), B, B, B, N, N), b"needs status_d"),      # a tag check without status
        ("gmx_history_record", (B, i32(1), B, B, i64(4), u32(256), B, B, B, B, N), b"expect_tag = 256"),    # no such tag
        ("gmx_lineage", (N, N, i32(3), i32(1), i64(10), N, i64(4), N, N, N, N), b"null argument"),
        ("gmx_lineage", (B, B, i32(3), i32(1), i64(10), B, i64(4), N, N, B, N), b"paths_d and traj_d"),     # neither output
        ("gmx_lineage", (B, N, i32(3), i32(1), i64(10), B, i64(4), N, B, B, N), b"xs_d with traj_d"),       # traj without xs
        ("gmx_lineage", (B, B, i32(0), i32(1), i64(10), B, i64(4), B, B, B, N), b"must be positive"),       # T = 0
        ("gmx_lineage", (B, B, i32(3), i32(1), i64(10), B, i64(-1), B, B, B, N), b"must be positive"),      # m < 0
        ("gmx_lineage", (B, B, i32(3), i32(1), i64(10), B, i64(4), B, B, N, N), b"null argument"),          # no status word
    ]
    return calls, buf
