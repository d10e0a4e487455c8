"""Drivers of tests/test_lag_pairs_cpu.py and tests/test_lag_pairs_gpu.py: gmx_rows_lag_pairs step by step behind the recording
gmx_rows_lag_moments against numpy float64, its refusals and sizes, and smc.BootstrapBank(smooth_lag=L, smooth_pairs=True)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bank_checks as K, history_checks as H, lag_checks as C, moments_checks as M
from tests.lag_checks import BANKS, DEVICE_VS_MIRROR, LAGS, SENTINEL, steps_of
from tests.moments_checks import library

SIZES = C.SIZES + [16, 17]             # ... and the first full block of a matrix instruction, and one column past it
# The mirror's largest deviations from the reference, MEASURED over exactly the cases of this file — check_size's (mean 5.39e-9,
# second 8.43e-10, both at n = 5) and check_bank's plain lgssm rows (4.08e-9, 1.64e-9): a mean relative to the row's max |x| at its
# time, a second moment to the product of the two times' max |x|.  Both backends are held to 4 x these (another summation tree).
MEASURED = {"mean": 5.4e-9, "second": 1.7e-9}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
width = lambda D: 2 * D + 3 * D * D    # [mean_s][mean_next][cov_s][cross][cov_next]


def reference(steps, t, l, with_carry):
    """[R, 2 D + 3 D^2] float64 of the pair (x_{t-l}, x_{t-l+1}) along the composed ancestor tables under w = exp(a - max a),
    a = lw_t (+ carry_t, the add in float32), a NaN weight 0; and the rows' max |x| at both times"""
    lw, carry, _, _ = steps[t]
    with np.errstate(invalid="ignore"):
        a = ((lw + carry).astype(np.float32) if with_carry else lw).astype(np.float64)
    (R, n), xu, xv = a.shape, steps[t - l][2].astype(np.float64), steps[t - l + 1][2].astype(np.float64)
    b = [np.tile(np.arange(n), (R, 1))]
    for j in range(l):
        b.append(np.take_along_axis(steps[t - j][3].astype(np.int64), b[-1], axis=1))
    D = xu.shape[0]
    out = np.full((R, width(D)), np.nan)
    for r in range(R):
        m = np.fmax.reduce(a[r])
        with np.errstate(invalid="ignore"):
            w = np.where(np.isnan(a[r]), 0.0, np.exp(a[r] - m)) if np.isfinite(m) else np.zeros(n)
        S0, u, v = w.sum(), xu[:, r, b[l][r]], xv[:, r, b[l - 1][r]]
        if S0 > 0:
            mu, mv = (w * u).sum(axis=1) / S0, (w * v).sum(axis=1) / S0
            cs, cx, cn = ((w * p) @ q.T / S0 - np.outer(mp, mq) for p, q, mp, mq in ((u, u, mu, mu), (u, v, mu, mv), (v, v, mv, mv)))
            for c in (cs, cn):
                np.fill_diagonal(c, np.maximum(np.diagonal(c), 0.0))
            out[r] = np.concatenate([mu, mv, cs.ravel(), cx.ravel(), cn.ravel()])
    return out, np.abs(xu).max(axis=(0, 2)), np.abs(xv).max(axis=(0, 2))


def deviations(got, want, top_s, top_n, dev, bound=None, what=()):
    """the (mean, second) deviations of one lag, scaled as MEASURED is, folded into dev and held to `bound`; no mass: NaN everywhere"""
    D = int(round((np.sqrt(1 + 3 * want.shape[1]) - 1) / 3))
    DD = D * D
    for r in range(want.shape[0]):
        if np.isnan(want[r, 0]):
            assert np.all(np.isnan(got[r])), (what, r, got[r])
            continue
        d = np.abs(got[r] - want[r])
        err = {"mean": max(float(d[:D].max()) / top_s[r], float(d[D:2 * D].max()) / top_n[r]),
               "second": max(float(d[2 * D + k * DD:2 * D + (k + 1) * DD].max()) / s
                             for k, s in enumerate((top_s[r] ** 2, top_s[r] * top_n[r], top_n[r] ** 2)))}
        assert bound is None or all(err[k] <= (bound[k] if isinstance(bound, dict) else bound) for k in err), (what, r, err, bound)
        dev.update({k: max(dev[k], err[k]) for k in err})


def run(be, n, R, D, L, k, with_carry, stride):
    """steps_of's steps through the C-ABI on padded rows: gmx_rows_lag_moments records step t, then every lag 1 .. min(L, t) of
    gmx_rows_lag_pairs -> [t][lag - 1] = [R, 2 D + 3 D^2], and the bit-exact properties asserted below"""
    steps, ld, rs, W = steps_of(n, R, D, L, k), n + 3, n + 5, width(D)
    x_ld, dev, c = R * rs, be.device, be.c
    hx = torch.full(((L + 1) * D * x_ld + 8,), SENTINEL, dtype=torch.float32, device=dev)
    ha = torch.full(((L + 1) * R * ld + 8,), -7, dtype=torch.int32, device=dev)
    ws = [torch.zeros(((int(f(R, n, D, L)) + 7) // 8,), dtype=torch.int64, device=dev)
          for f in (c.gmx_rows_lag_moments_workspace, c.gmx_rows_lag_pairs_workspace)]
    got, none = [], torch.zeros((2 * D + 2,), dtype=torch.float64, device=dev)
    for t, (lw, carry, x, anc) in enumerate(steps):
        host = [np.full((R, ld), np.float32(SENTINEL)), np.full((R, ld), np.float32(SENTINEL)), np.full((D, x_ld), np.float32(SENTINEL)),
                np.full((R, ld), np.int32(-7))]
        host[0][:, :n], host[1][:, :n] = lw, carry
        host[2].reshape(D, R, rs)[:, :, :n] = x
        if t:
            host[3][:, :n] = anc + stride * np.arange(R, dtype=np.int32)[:, None]
        tl, tc, tx, ta = (torch.from_numpy(a.copy()).to(dev) for a in host)
        head = (be.ptr(tl), be.ptr(tc) if with_carry else None, R, n, ld, be.ptr(tx), D, x_ld, rs)
        rc = c.gmx_rows_lag_moments(*head, be.ptr(ta) if t else None, ld, stride, t, L, 0, -1, be.ptr(hx), x_ld, be.ptr(ha), ld,
                                    be.ptr(none), 2 * D, 0, be.ptr(ws[0]), be.stream())
        assert rc == 0, c.gmx_last_error()
        rings, hi = (hx.cpu().numpy().copy(), ha.cpu().numpy().copy()), min(L, t)

        def call(lo, hi):
            out = torch.full((L + 2, R + 1, W + 2), SENTINEL, dtype=torch.float64, device=dev)
            rc = c.gmx_rows_lag_pairs(*head[:5], None, D, x_ld, rs, stride, t, L, lo, hi, be.ptr(hx), x_ld, be.ptr(ha), ld,
                                      be.ptr(out), W + 2, (R + 1) * (W + 2), be.ptr(ws[1]), be.stream())
            assert rc == 0, c.gmx_last_error()
            return out.cpu().numpy()
        assert np.all(call(1, 0) == SENTINEL), "the empty range wrote an output"
        full = call(1, hi)
        assert np.all(full[0] == SENTINEL) and np.all(full[hi + 1:] == SENTINEL) and np.all(full[:, R] == SENTINEL) and \
            np.all(full[:, :, W:] == SENTINEL), "written past the outputs"
        if t >= L:
            one = call(L, L)
            assert np.all(one[:L] == SENTINEL) and np.array_equal(one[L].view(np.int64), full[L].view(np.int64)), "the range (L, L) is not lag L of the full range"
        assert all(H.same_bits(d, h) for d, h in zip((tl, tc, tx, ta, hx, ha), host + list(rings))), "an input or a ring was written"
        for k3 in (0, 2):                                # cov_s and cov_next
            m = full[1:hi + 1, :R, 2 * D + k3 * D * D:2 * D + (k3 + 1) * D * D].reshape(-1, D, D).view(np.int64)
            assert np.array_equal(m, m.transpose(0, 2, 1)), "a covariance is not symmetric bit for bit"
        got.append(full[1:hi + 1, :R, :W].copy())
    return got


def check_size(be, n):
    """per L and R = 1, 3, 5 one run, D = 1, 3, 15, carry and index_stride in turn: within TOL of the reference (the size's largest
    deviations are printed first: MEASURED) and, one tile, within DEVICE_VS_MIRROR of the mirror"""
    dev, checks = {"mean": 0.0, "second": 0.0}, []
    for k, (L, R) in enumerate((L, R) for L in LAGS if n <= 1024 or L <= 5 for R in (1, 3, 5)):
        D, with_carry, stride = (1, 3, 15)[(k + k // 3 + 2) % 3], bool(k % 2), (0, n)[(k // 2) % 2]
        got = run(be, n, R, D, L, k, with_carry, stride)
        mirror = run(library("mirror"), n, R, D, L, k, with_carry, stride) if be.device.type == "cuda" and n <= 1024 else None
        for t, lags in enumerate(got):
            for l, g in enumerate(lags, start=1):
                want = reference(steps_of(n, R, D, L, k), t, l, with_carry)
                deviations(g, *want, dev)
                checks.append(((n, R, D, L, t, l), g) + want)
                if mirror is not None:
                    deviations(g, mirror[t][l - 1], *want[1:], dict(dev), DEVICE_VS_MIRROR, ("device against mirror", n, R, D, L, t, l))
    print("n", n, dev, "allowed", TOL)
    for what, g, want, top_s, top_n in checks:
        deviations(g, want, top_s, top_n, dict(dev), TOL, what)


def check_refusals_of(lib):
    buf = (ctypes.c_int64 * 8)()
    P, N = ctypes.cast(buf, ctypes.c_void_p), None
    def call(lw=P, rows=2, n=10, ld=10, D=2, x_ld=20, x_rs=10, stride=10, t=3, L=2, lo=2, hi=2, hx=P, hx_ld=20, ha=P, ha_ld=10, out=P,
             out_ld=16, ws=P):
        return lw, N, rows, n, ld, N, D, x_ld, x_rs, stride, t, L, lo, hi, hx, hx_ld, ha, ha_ld, out, out_ld, 8, ws, N
    calls = [(call(lw=N), b"null"), (call(hx=N), b"null"), (call(ha=N), b"null"), (call(out=N), b"null"), (call(ws=N), b"null"),
             (call(D=0), b"D = 0"), (call(D=16, out_ld=800), b"D = 16"), (call(n=0), b"n = 0"),
             (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, x_ld=2 ** 23), b"n = 2097153"), (call(rows=-1), b"rows = -1"), (call(ld=9), b"ld = 9"),
             (call(x_ld=19), b"x_ld = 19"), (call(stride=2 ** 31), b"index_stride = 2147483648"), (call(L=0), b"L = 0"),
             (call(L=33), b"L = 33"), (call(t=-1), b"t = -1"), (call(lo=0), b"lag_lo = 0"), (call(hi=3, t=5), b"lag_hi = 3"),
             (call(t=1), b"lag_hi = 2"), (call(ha_ld=9), b"hist_a_ld = 9"), (call(hx_ld=19), b"hist_x_ld = 19"),
             (call(out_ld=15), b"out_ld = 15")]
    for args, names in calls:
        assert lib.gmx_rows_lag_pairs(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_rows_lag_pairs" in msg and names in msg, (msg, names)
    sizes = [int(lib.gmx_rows_lag_pairs_workspace(*a)) for a in ((3, 1024, 2, 8), (3, 1025, 2, 8), (3, 1025, 2, 33))]
    assert sizes == [16, (6 * (8 * (136 + 136 + 256) * 8 + 4) + 15) // 16 * 16, 16]      # 6 cells x (8 lags x 528 doubles + a float)


def check_bank(be, specialize, capture=False, model="lgssm", n=64, T=5, smooth_lag=2, **kw):
    """(a) the bank without smooth_pairs bit for bit; (b) mean_s, cov_s' diagonal and the last cov_next against smoothed_mean(),
    smoothed_var() and a covariance=True bank; (c) plain lgssm: the reference on each key's BootstrapSweep history; (d) two captured
    replays are the eager bits; (e) the named refusals raise"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    init, step = K._models(model)
    keys, ys, R = G.split(G.key(M.BK_SEED), M.BK_R), K._data(T), M.BK_R
    lag, bank, cov = (smc.BootstrapBank(init, step, n, R, T, specialize=specialize, **kw, **m).prepare(keys, ys)
                      for m in (dict(smooth_lag=smooth_lag), dict(smooth_lag=smooth_lag, smooth_pairs=True), dict(covariance=True)))
    for b in (lag, bank, cov):
        b.launch()
    assert all(H.same_bits(a, b) for a, b in zip(K._np_state(bank.state()), K._np_state(lag.state())))
    assert np.array_equal(bank.log_ml(), lag.log_ml()) and torch.equal(bank.smo.view(torch.int64), lag.smo.view(torch.int64))
    for bad in (lag.smoothed_pairs, lag.smoothed_cov):
        with pytest.raises(ValueError, match="smooth_pairs=True"):
            bad()
    for bad in (dict(smooth_pairs=True), dict(smooth_lag=1, smooth_pairs=True, T=1)):
        with pytest.raises(ValueError, match="smooth_pairs=True"):
            smc.BootstrapBank(init, step, n, R, **{"T": T, **bad})
    with pytest.raises(NotImplementedError, match="smooth_pairs=True"):
        smc.ConditionalBank(init, step, n, R, T, smooth_pairs=True)
    with pytest.raises(NotImplementedError, match="D = 16"):
        smc._refuse_wide_pairs(bank, 16, None)
    pairs, scov, rec = bank.smoothed_pairs(), bank.smoothed_cov(), bank.smp.cpu().numpy().copy()
    D = pairs.mean_s.shape[2]
    assert pairs.cross.shape == (T - 1, R, D, D) and scov.shape == (T, R, D, D) and scov.dtype == torch.float64
    close = lambda a, b: np.all(np.abs(a.numpy() - b.numpy()) <= 1e-12 * np.abs(b.numpy()))
    assert close(pairs.mean_s, bank.smoothed_mean()[:T - 1].reshape(T - 1, R, D))
    assert close(pairs.cov_s.diagonal(dim1=2, dim2=3), bank.smoothed_var()[:T - 1].reshape(T - 1, R, D))
    assert close(scov[T - 1], cov.filter_cov()[T - 1])
    if model == "lgssm" and not kw:
        for r in range(R):
            sw = smc.BootstrapSweep(init, step, n, T, specialize=specialize, history=True).prepare(keys[r], ys)
            sw.launch()
            h = sw.history()
            hx, hlw, ha = (v.cpu().numpy() for v in (h.x, h.log_weights, h.ancestors))
            steps = [(hlw[t][None], None, hx[t][None, None], ha[t - 1][None] if t else None) for t in range(T)]
            dev, checks = {"mean": 0.0, "second": 0.0}, []
            for s in range(T - 1):
                t = min(s + smooth_lag, T - 1)
                checks.append((rec[s, r][None],) + reference(steps, t, t - s, False))
                deviations(*checks[-1], dev)
            print("bank row", r, dev, "allowed", TOL)
            for s, c in enumerate(checks):
                deviations(*c, dict(dev), TOL, ("bank", r, s))
    if capture:
        bank.smp.zero_()
        bank.capture()
        bank.launch()
        bank.launch()                    # two replays
        assert np.array_equal(bank.smp.cpu().numpy().view(np.int64), rec.view(np.int64))
