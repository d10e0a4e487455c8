"""Drivers of tests/test_smooth_cpu.py (the CPU mirror) and tests/test_smooth_gpu.py (the HIP library): gmx_smooth_back against
numpy float64 on the same float32 logits, its refusals, and smc.SweepHistory.marginal_smooth against the FFBSm recursion in
numpy float64 on the logits of smc._backward_logits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import history_checks as H
from tests.moments_checks import library

SIZES = [1, 5, 63, 64, 65, 255, 257, 1023, 1025, 4099]      # strip edges, ragged 16-byte loads, several strips; the row kernels' 1024
KS = [1, 3, 4, 5, 67, 260]                                   # a ragged k-step, past one wave's share of a chunk, past one run of rows
CS = [1, 2, 4, 16]
KINDS = ["normal", "dominant", "holes", "norow", "mixed", "slabs"]
SENTINEL, POISON = -7.5, np.float32(1e30)                    # POISON between the rows of A: read as a logit it would take all the mass
# The largest deviation of the restatement — subtraction and exp in float32 as numpy does them, everything after in float64 — from
# reference(), by deviation()'s metric, MEASURED over exactly check_size's cases.  Its printed maxima per n:
#   1: 0, 5: 2.86e-7, 63: 5.42e-7, 64: 1.01e-6, 65: 5.31e-7, 255: 9.73e-7, 257: 1.05e-6, 1023: 1.04e-6, 1025: 1.04e-6, 4099: 1.05e-6
# (the float32 subtraction: half an ulp of a difference of 16 .. 32 is 9.5e-7 of that weight, and with K = 1 nothing averages it).
# Both backends are held to 4 x it and at least 8 * 2^-23 (DESIGN.md section 3's rule): the factor covers gmx_expf_nonpos against
# np.exp and the order of summation.
MEASURED = 1.05e-6
TOL = max(4.0 * MEASURED, 8.0 * 2.0 ** -23)


def case(n, K, C, kind):
    """(A [K, n] float32, U [C, K] float64, G0 [C, n] float64 or None), never modified"""
    rng = np.random.default_rng(100000 * n + 100 * K + C + 7 * len(kind))
    A, U = (3.0 * rng.normal(size=(K, n))).astype(np.float32), rng.random(size=(C, K)) + 0.01
    if kind == "dominant":
        A[np.arange(K), rng.integers(n, size=K)] += np.float32(1e4)
    elif kind == "holes":
        A[:, n // 4:n // 4 + max(1, n // 3)] = -np.inf
        A[K // 2, n // 2] = np.nan
    elif kind == "norow":
        A[K // 2] = -np.inf
    elif kind in ("mixed", "slabs"):
        U = rng.normal(size=(C, K))
    return A, U, (rng.normal(size=(C, n)) if kind == "slabs" else None)


def softmax_rows(A, dtype):
    """(P [K, n] float64, rows without mass): the weights exp(A - row max) taken in `dtype` (0 for a NaN difference), then float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = A.astype(dtype)
        d = a - np.fmax.reduce(a, axis=1, initial=-np.inf, keepdims=True)
        e = np.where(np.isnan(d), 0.0, np.exp(d)).astype(np.float64)
        S = e.sum(axis=1, keepdims=True)
        return np.where(S > 0, e / S, 0.0), int(np.sum(S == 0))


def reference(A, U, G0):
    """(G64, the metric's denominator, the rows without mass)"""
    P, dead = softmax_rows(A, np.float64)
    return U @ P + (0.0 if G0 is None else G0), np.abs(U) @ P + (0.0 if G0 is None else np.abs(G0)), dead


def deviation(G, G64, den, what=()):
    """max |G - G64| / den; where den is 0, G is exactly 0"""
    assert np.all(G[den == 0] == 0.0), (what, "mass where the reference has none")
    return float(np.max(np.abs(G - G64)[den > 0] / den[den > 0], initial=0.0))


def smooth_back(be, A, U, G0=None, pad=0, rows=None):
    """the raw C call over rows `rows` of A (all by default): A's rows n + pad apart, G inside a band of sentinels, accumulate iff G0
    -> (G, status); what lies round G, and the inputs, keep their words"""
    (K, n), C, (lo, hi) = A.shape, U.shape[0], rows or (0, A.shape[0])
    host_a, host_u = np.full((K, n + pad), POISON, np.float32), np.full((C, K + 1), SENTINEL)
    host_a[:, :n], host_u[:, :K] = A, U
    host_g = np.full((C + 1, n + 2), SENTINEL)
    host_g[:C, :n] = SENTINEL if G0 is None else G0
    ta, tu, tg = (torch.from_numpy(a.copy()).to(be.device) for a in (host_a, host_u, host_g))
    status = torch.zeros((1,), dtype=torch.int64, device=be.device)
    ws = torch.zeros(((int(be.c.gmx_smooth_back_workspace(hi - lo, n, C)) + 7) // 8,), dtype=torch.int64, device=be.device)
    rc = be.c.gmx_smooth_back(be.ptr(ta[lo:]), hi - lo, n, n + pad, be.ptr(tu[:, lo:]), C, K + 1, be.ptr(tg), n + 2,
                              int(G0 is not None), be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    got = tg.cpu().numpy()
    assert np.all(got[C] == SENTINEL) and np.all(got[:C, n:] == SENTINEL), "written past G"
    assert H.same_bits(ta, host_a) and np.array_equal(tu.cpu().numpy(), host_u), "an input was written"
    return got[:C, :n], int(status.item())


def check_size(be, n):
    """every K and kind at this n, C and ld going round their values: within TOL of the reference (the restatement's and the
    library's largest deviations are printed first: MEASURED); on the device a second call gives the same bits"""
    devs = []
    for ik, K in enumerate(KS):
        C, pad = CS[(SIZES.index(n) + ik) % 4], 3 * ((SIZES.index(n) + ik) // 4 % 2)
        for kind in KINDS:
            A, U, G0 = case(n, K, C, kind)
            G64, den, dead = reference(A, U, G0)
            assert kind != "norow" or dead == 1
            got, status = smooth_back(be, A, U, G0, pad)
            assert status == dead, (n, K, C, kind, status, dead)
            restated = U @ softmax_rows(A, np.float32)[0] + (0.0 if G0 is None else G0)
            devs.append(((n, K, C, kind), deviation(got, G64, den), deviation(restated, G64, den)))
            if kind == "slabs" and K > 1:                        # two slabs onto G0 against one call over all rows
                half, s1 = smooth_back(be, A, U, G0, pad, rows=(0, K // 2))
                both, s2 = smooth_back(be, A, U, half, pad, rows=(K // 2, K))
                assert s1 + s2 == dead
                devs.append(((n, K, C, "two slabs"), deviation(both, G64, den), 0.0))
                assert deviation(both, got, den) <= TOL
            if be.device.type == "cuda":
                assert np.array_equal(smooth_back(be, A, U, G0, pad)[0].view(np.int64), got.view(np.int64)), (n, K, C, kind)
    print("n", n, "library", max(d[1] for d in devs), "restatement", max(d[2] for d in devs), "allowed", TOL)
    for what, dev, _ in devs:
        assert dev <= TOL, (what, dev, TOL)


def check_refusals_of(hip, mirror):
    buf = (ctypes.c_int64 * 8)()
    P, P4, N = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(ctypes.addressof(buf) + 4), None
    def call(A=P, K=4, n=10, ld=10, u=P, C=2, u_ld=4, G=P, g_ld=10, status=P, ws=P):
        return A, K, n, ld, u, C, u_ld, G, g_ld, 0, status, ws, N
    calls = [(call(A=N), b"null"), (call(u=N), b"null"), (call(G=N), b"null"), (call(status=N), b"null"), (call(ws=N), b"null"),
             (call(K=0), b"K = 0"), (call(n=0), b"n = 0"), (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, g_ld=2 ** 21 + 1), b"n = 2097153"),
             (call(C=0), b"C = 0"), (call(C=17), b"C = 17"), (call(ld=9), b"ld = 9"), (call(u_ld=3), b"u_ld = 3"),
             (call(g_ld=9), b"g_ld = 9"), (call(u=P4), b"8-byte aligned"), (call(G=P4), b"8-byte aligned")]
    for args, names in calls:
        said = []
        for lib in (mirror, hip):                                # (the mirror first: the device library only sees a refused call)
            lib.gmx_last_error.restype = ctypes.c_char_p
            assert lib.gmx_smooth_back(*args) != 0, names
            said.append(lib.gmx_last_error())
        assert said[0].startswith(b"gmx_smooth_back:") and names in said[0] and said[0] == said[1], (said, names)


# --- SweepHistory.marginal_smooth ------------------------------------------------------------------------------------------------
SMOOTH_T, SMOOTH_SEED = 5, 31


def ffbsm(h, sites):
    """the recursion in numpy float64 on smc._backward_logits' rows, fetched 16 rows a launch as the method fetches them"""
    from genjax_amd.inference import smc
    T, D, n, x = h.T, h.D, h.n, h._xs.cpu().numpy().astype(np.float64)
    w, second = np.empty((T, n)), np.empty((T - 1, D, D))
    w[T - 1] = softmax_rows(h.log_weights[T - 1:].cpu().numpy(), np.float64)[0][0]
    R = min(smc.BACKWARD_ROWS_MAX, n, 40 // D)
    A = torch.empty((n, n), dtype=torch.float32, device=h._xs.device)
    for t in range(T - 2, -1, -1):
        for r0 in range(0, n, R):
            smc._backward_logits(h._step, sites or (h._state_addr,), h._obs_addr, h._step_state(t), (),
                                 [h._xs[t + 1, d, r0:r0 + R] for d in range(D)], h._ys[t + 1], h.log_weights[t], A[r0:r0 + R])
        P = softmax_rows(A.cpu().numpy(), np.float64)[0]
        w[t] = w[t + 1] @ P
        second[t] = x[t] @ ((w[t + 1] * x[t + 1]) @ P).T
    mean = np.einsum("tn,tdn->td", w, x)
    cov = np.einsum("tn,tan,tbn->tab", w, x, x) - mean[:, :, None] * mean[:, None, :]
    return w, mean, cov, second - mean[:-1, :, None] * mean[1:, None, :]


def check_marginal(be, model, n, specialize):
    """weights elementwise, moments relative to max |x| and max x^2, within (T - 1) TOL of the recursion: a step's error feeds the next"""
    import genjax_amd as G
    from genjax_amd import numpy as jnp, workloads
    from genjax_amd.inference.smc import BootstrapSweep, SweepHistory
    if model == "lgssm":
        (init, step), ys, sites = workloads.make_lgssm(G), workloads.lgssm_data(SMOOTH_T), None
    else:
        init, step = H.make_tracker(G, lambda a, b: jnp.stack([a, b]))
        ys, sites = np.random.default_rng(SMOOTH_SEED).normal(size=SMOOTH_T).astype(np.float32), ("p", "v")
    sw = BootstrapSweep(init, step, n, SMOOTH_T, history=True, specialize=specialize).prepare(G.key(SMOOTH_SEED), torch.from_numpy(ys))
    sw.launch()
    h = sw.history()
    got = h.marginal_smooth(state_sites=sites)
    w, mean, cov, cross = ffbsm(h, sites)
    D, tol, top = h.D, (SMOOTH_T - 1) * TOL, float(np.abs(h._xs.cpu().numpy()).max())
    gw, gm, gv, gc, gx = (v.cpu().numpy() for v in got)
    assert gw.dtype == np.float64 and gw.shape == (SMOOTH_T, n) and gm.shape == h.filter_mean().shape == gv.shape
    floor = (SMOOTH_T - 1) * 2.0 ** -126 / tol       # a float32 weight below the smallest normal is off by up to 2^-126; S_k >= 1
    devs = {"weights": float(np.max(np.abs(gw - w) / (w + floor))), "mean": float(np.abs(gm.reshape(SMOOTH_T, D) - mean).max()) / top,
            "cov": float(np.abs(gc - cov).max()) / top ** 2, "cross": float(np.abs(gx - cross).max()) / top ** 2}
    print(model, n, devs, "allowed", tol)
    assert all(v <= tol for v in devs.values()), (devs, tol)
    assert np.array_equal(gv.reshape(SMOOTH_T, D), np.diagonal(gc, axis1=1, axis2=2))
    assert np.all(np.abs(gw.sum(axis=1) - 1.0) <= 1e-12)
    assert np.all(np.abs(gm[SMOOTH_T - 1] - h.filter_mean()[SMOOTH_T - 1].cpu().numpy()) <= 1e-12)
    init, step = H.make_pair(G)
    sw = BootstrapSweep(init, step, 64, 3, history=True, specialize=False).prepare(G.key(2), torch.from_numpy(H.state_data()))
    sw.launch()
    with pytest.raises(NotImplementedError, match="SweepHistory.marginal_smooth: the step model samples 'c'"):
        sw.history().marginal_smooth(state_sites=("a", "b"))
    for D_, n_, why in ((16, 8, "D = 16"), (1, 16385, "n = 16385")):
        wide = SweepHistory(torch.zeros((2, D_, n_)), torch.zeros((2, n_)), torch.zeros((2, n_), dtype=torch.int32), (D_,),
                            step=h._step, ys=h._ys, obs_addr="y", state_addr="x")
        with pytest.raises(NotImplementedError, match=why):
            wide.marginal_smooth(state_sites=tuple("abcdefghijklmnop"[:D_]))
