"""Shared drivers of tests/test_backward_cpu.py (the C-ABI's CPU mirror) and tests/test_backward_gpu.py (the HIP
library): gmx_pick_rows against the oracle's per-row path, SweepHistory.backward_sample against an oracle loop (bit for
bit) and against the exact particle-FFBS marginals of the same history."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import genjax_oracle as O
from tests import history_checks as H

POISON = np.float32(1e30)          # what the padding between rows holds: read as a logit it would take all the mass


# --- gmx_pick_rows alone ---------------------------------------------------------------------------------------------------
def pick_rows(be, rows, keys, pad=0, poison=True):
    """rows: [R, n] float32, keys: [R, 2] uint32 -> (out int32 [R], status); rows are n + pad elements apart"""
    dev = be.device
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    R, n = rows.shape
    ld = n + pad
    host = np.full((R, ld), POISON if poison else 0.0, dtype=np.float32)
    host[:, :n] = rows
    logits = torch.from_numpy(host).to(dev)
    k_d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(R, 2)).to(dev)
    out = torch.full((R,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_pick_rows_workspace(R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_pick_rows(be.ptr(k_d), be.ptr(logits), R, n, ld, be.ptr(out), be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return out.cpu().numpy(), int(status.item())


def oracle_pick(row, key):
    return int(O.ancestors(O.MULTINOMIAL, key, O.weight_cdf(np.asarray(row, np.float32))[0], n_out=1)[0])


def pick_keys(rows=4):
    return O.split(O.key(7), rows)


@functools.lru_cache(maxsize=None)
def pick_case(name):
    """the rows of one case, [4, n] (never modified)"""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("normal"):
        n = int(name[6:])
        rows = rng.normal(size=(4, n))
    elif name == "gap":                 # the first tile lowered by 100: its exponent is more than 64 below the row's
        rows = rng.normal(size=(4, 2051))
        rows[:, :1024] -= 100.0
    elif name == "hole":                # columns 5 .. 1999 carry nothing
        rows = rng.normal(size=(4, 2051))
        rows[:, 5:2000] = -np.inf
    elif name == "last":                # all the mass on the last column
        rows = np.full((4, 2051), -np.inf)
        rows[:, -1] = rng.normal(size=4)
    elif name == "first":
        rows = np.full((4, 2051), -np.inf)
        rows[:, 0] = rng.normal(size=4)
    elif name == "mixed":               # four different rows in one call: each its own key and statistics
        rows = rng.normal(size=(4, 2051))
        rows[1, :1024] -= 100.0
        rows[2, 5:2000] = -np.inf
        rows[3] = -np.inf
        rows[3, 1500] = 0.0
    else:
        raise KeyError(name)
    rows = rows.astype(np.float32)
    rows.setflags(write=False)
    return rows


PICK_CASES = ["normal1", "normal5", "normal1024", "normal1025", "normal2051", "gap", "hole", "last", "first", "mixed"]


def check_pick_case(be, name, pad=0):
    rows, keys = pick_case(name), pick_keys()
    want = [oracle_pick(rows[r], keys[r]) for r in range(4)]
    got, status = pick_rows(be, rows, keys, pad=pad)
    print(name, "pad", pad, "oracle", want, "got", got.tolist(), "status", status)
    assert status == 0
    assert got.tolist() == want
    if name == "last":
        assert want == [rows.shape[1] - 1] * 4
    if name == "first":
        assert want == [0] * 4


def check_pick_no_mass(be):
    """a row that is all -inf returns n - 1 and is counted; its neighbours are drawn as usual"""
    rows = pick_case("normal2051").copy()
    rows[2] = -np.inf
    keys = pick_keys()
    got, status = pick_rows(be, rows, keys, pad=3)
    want = [oracle_pick(rows[r], keys[r]) for r in range(4)]
    assert want[2] == 2050                     # (the oracle's per-row path answers the same)
    assert got.tolist() == want and status == 1


# --- backward_sample against an oracle loop -------------------------------------------------------------------------------
def oracle_backward(os_, LW, X, ys, key, m, sites, n):
    """The definition of SweepHistory.backward_sample, with the oracle: LW[t] float32 [n]; X[t] the step's states ([n]
    or [n, D]); the row of trajectory k at step t is LW[t] + the weight os_.importance returns under the FULL constraint
    {sites: x~_{t+1}[k], "y": ys[t+1]} with args (X[t],) (no randomness is left: the keys are arbitrary)."""
    T = len(LW)
    paths = np.zeros((T, m), np.int32)
    cdf = O.weight_cdf(LW[T - 1])[0]
    paths[T - 1] = np.asarray(O.ancestors(O.MULTINOMIAL, O.fold_in(key, T - 1), cdf, n_out=m)).astype(np.int32)
    any_keys = O.split(O.key(0), n)
    empty_rows = 0
    for t in range(T - 2, -1, -1):
        rk = O.split(O.fold_in(key, t), m)
        for k in range(m):
            xn = np.atleast_1d(X[t + 1][paths[t + 1, k]])
            con = {a: np.float32(xn[d]) for d, a in enumerate(sites)}
            con["y"] = np.float32(ys[t + 1])
            _, w = os_.importance(any_keys, O.C.d(con), (X[t],))
            row = (LW[t] + np.asarray(w, np.float32)).astype(np.float32)
            cdf, total = O.weight_cdf(row)[:2]
            empty_rows += int(total) == 0
            paths[t, k] = int(O.ancestors(O.MULTINOMIAL, rk[k], cdf, n_out=1)[0])
    assert empty_rows == 0
    return paths


LGSSM_M, BACK_KEY = 37, 99


@functools.lru_cache(maxsize=None)
def lgssm_backward_oracle():
    """n = 2051, T = 5, m = 37 on the oracle's own sweep (history_checks.lgssm_oracle): shared, never modified"""
    from genjax_amd import workloads
    ref = H.lgssm_oracle("systematic")["hist"]
    _, os_ = workloads.make_lgssm(O)
    LW = [np.asarray(r["lw"], np.float32) for r in ref]
    X = [np.asarray(r["x"], np.float32) for r in ref]
    paths = oracle_backward(os_, LW, X, workloads.lgssm_data(H.LGSSM_T), O.key(BACK_KEY), LGSSM_M, ("x",), H.LGSSM_N)
    paths.setflags(write=False)
    return paths, X


def check_backward_lgssm(capture):
    """m = 37 is no multiple of the rows per density launch: the last chunk is partial"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    assert LGSSM_M % smc.BACKWARD_ROWS_MAX not in (0, LGSSM_M)
    want, X = lgssm_backward_oracle()
    sw = H.run_lgssm(True, False, False, capture, False, "systematic")
    h = sw.history()
    paths, traj = h.backward_sample(G.key(BACK_KEY), LGSSM_M, return_paths=True)
    assert paths.dtype == torch.int32 and tuple(paths.shape) == (H.LGSSM_T, LGSSM_M)
    assert tuple(traj.shape) == (LGSSM_M, H.LGSSM_T)
    assert np.array_equal(paths.cpu().numpy(), want), np.argwhere(paths.cpu().numpy() != want)[:5]
    assert H.same_bits(traj, np.stack([X[t][want[t]] for t in range(H.LGSSM_T)], axis=1))
    only = h.backward_sample(G.key(BACK_KEY), LGSSM_M)
    assert H.same_bits(only, traj.cpu().numpy())
    return h


TRACKER_M = 5


@functools.lru_cache(maxsize=None)
def tracker_backward_oracle():
    ref = H.state_oracle("vector")
    _, os_ = H.make_tracker(O, lambda a, b: np.stack([a, b], axis=-1))
    LW = [r["lw"] for r in ref]
    X = [np.ascontiguousarray(r["rows"].T) for r in ref]          # [n, 2]
    paths = oracle_backward(os_, LW, X, H.state_data(), O.key(BACK_KEY), TRACKER_M, ("p", "v"), H.STATE_N)
    paths.setflags(write=False)
    return paths, X


def tracker_history(**kw):
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd.inference.smc import BootstrapSweep
    init, step = H.make_tracker(G, lambda a, b: jnp.stack([a, b]))
    sw = BootstrapSweep(init, step, H.STATE_N, H.STATE_T, history=True, **kw).prepare(G.key(H.STATE_SEED),
                                                                                         torch.from_numpy(H.state_data()))
    sw.launch()
    return sw.history()


def check_backward_tracker(**kw):
    """the vector-state tracker, n = 1027, T = 4, m = 5, state_sites = ("p", "v")"""
    import genjax_amd as G
    want, X = tracker_backward_oracle()
    h = tracker_history(**kw)
    paths, traj = h.backward_sample(G.key(BACK_KEY), TRACKER_M, state_sites=("p", "v"), return_paths=True)
    assert np.array_equal(paths.cpu().numpy(), want), np.argwhere(paths.cpu().numpy() != want)[:5]
    assert tuple(traj.shape) == (TRACKER_M, H.STATE_T, 2)
    assert H.same_bits(traj, np.stack([X[t][want[t]] for t in range(H.STATE_T)], axis=1))
    return h


# --- the law of the draws --------------------------------------------------------------------------------------------------
LAW_N, LAW_T, LAW_M, LAW_SEED = 300, 6, 2048, 2718


def ffbs_marginals(lw, x):
    """the exact smoothing marginals of particle FFBS on one history, float64, O(n^2 T):
    S_{T-1} = W_{T-1};  S_t = ((W_t (.) F) / colsum) S_{t+1},  F[i, j] = N(x_{t+1}[j]; a x_t[i], sx^2),  W_t = softmax(lw_t)"""
    from genjax_amd import workloads
    a, sx = workloads.LGSSM["a"], workloads.LGSSM["sx"]
    lw, x = np.asarray(lw, np.float64), np.asarray(x, np.float64)
    T = lw.shape[0]
    W = np.exp(lw - lw.max(axis=1, keepdims=True))
    W /= W.sum(axis=1, keepdims=True)
    S = [None] * T
    S[T - 1] = W[T - 1]
    for t in range(T - 2, -1, -1):
        F = np.exp(-0.5 * ((x[t + 1][None, :] - a * x[t][:, None]) / sx) ** 2)      # (the normalising constant cancels)
        B = W[t][:, None] * F
        S[t] = (B / B.sum(axis=0, keepdims=True)) @ S[t + 1]
    return np.stack(S)


def check_law():
    """LGSSM, n = 300, T = 6, m = 2048: given the history the m trajectories are independent draws from the particle-FFBS
    law, so mean_k x_t[paths[t, k]] has mean mu_t and standard deviation sigma_t / sqrt(m) under the exact marginal S_t:
    5 standard errors, per step (the bound is derived, not measured; the oracle loop alone sits at z <= 1.73 here)"""
    import genjax_amd as G
    sw = H.run_lgssm(True, False, False, False, False, "systematic", n=LAW_N, T=LAW_T, seed=LAW_SEED)
    h = sw.history()
    paths = h.backward_sample(G.key(BACK_KEY), LAW_M, return_paths=True)[0].cpu().numpy()
    x = h.x.cpu().numpy().astype(np.float64)
    S = ffbs_marginals(h.log_weights.cpu().numpy(), x)
    mu = (S * x).sum(axis=1)
    sigma = np.sqrt((S * x * x).sum(axis=1) - mu * mu)
    got = np.stack([x[t][paths[t]].mean() for t in range(LAW_T)])
    z = np.abs(got - mu) / (sigma / np.sqrt(LAW_M))
    distinct0 = len(np.unique(paths[0]))
    lineage0 = len(np.unique(h.lineage()[0].cpu().numpy()))
    print("law: z per step", np.round(z, 2), "distinct step-0 particles: backward", distinct0, "lineage", lineage0)
    assert np.all(np.abs(got - mu) <= 5.0 * sigma / np.sqrt(LAW_M)), z


# --- refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals():
    import pytest
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapSweep, SweepHistory
    h = tracker_history(specialize=False, fuse_resample=False)
    with pytest.raises(NotImplementedError, match="state_sites"):
        h.backward_sample(G.key(1), 3)
    init, step = H.make_pair(G)
    sw = BootstrapSweep(init, step, 64, 3, history=True, specialize=False).prepare(G.key(2), torch.from_numpy(H.state_data()))
    sw.launch()
    with pytest.raises(NotImplementedError, match="'c'"):
        sw.history().backward_sample(G.key(1), 3, state_sites=("a", "b"))
    bare = SweepHistory(h._xs, h.log_weights, h.ancestors, (2,))
    with pytest.raises(RuntimeError, match="backward_sample"):
        bare.backward_sample(G.key(1), 3, state_sites=("p", "v"))
    # m = 0: empty tensors in the same layouts
    paths, traj = h.backward_sample(G.key(1), 0, state_sites=("p", "v"), return_paths=True)
    assert tuple(paths.shape) == (H.STATE_T, 0) and tuple(traj.shape) == (0, H.STATE_T, 2)


def check_no_mass_is_an_error(be):
    """a history whose step-0 particles all carry log-weight -inf: every row of step 0 is -inf, no mass — FloatingPointError
    naming step 0"""
    import pytest
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import SweepHistory
    _, step = workloads.make_lgssm(G)
    dev = be.device
    n, T = 64, 2
    xs = torch.zeros((T, 1, n), dtype=torch.float32, device=dev)
    lws = torch.zeros((T, n), dtype=torch.float32, device=dev)
    lws[0] = float("-inf")
    h = SweepHistory(xs, lws, torch.zeros((T, n), dtype=torch.int32, device=dev), step=step,
                     ys=torch.zeros((T,), device=dev), step_extra=None, obs_addr="y", state_addr="x")
    with pytest.raises(FloatingPointError, match="step 0"):
        h.backward_sample(G.key(3), 4)
