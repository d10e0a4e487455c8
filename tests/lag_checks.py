"""Drivers of tests/test_lag_cpu.py (the CPU mirror) and tests/test_lag_gpu.py (the HIP library): gmx_rows_lag_moments driven step by
step against numpy float64 on the same float32 inputs, its refusals and sizes, and smc.BootstrapBank(smooth_lag=L)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import bank_checks as K
from tests import history_checks as H
from tests import moments_checks as M
from tests.moments_checks import library

SIZES = [1, 5, 255, 256, 257, 512, 513, 1023, 1024,      # one tile: the packing changes at 256 and 512, a ragged last thread
         1025, 2049, 3000]                               # a 1-column tail tile, three tiles, a ragged last tile
LAGS = [1, 2, 5, 32]                                     # L; a run is L + 3 steps: the ring of L + 1 slots wraps
ANCESTORS = ["uniform", "identity", "one", "reverse"]    # one per step, in turn
WEIGHTS = ["normal", "block", "dominant", "norow"]       # one per step, in turn
SENTINEL = -7.5
# The mirror's largest deviations from the reference, MEASURED over exactly the cases of this file — check_size's (its printed
# maxima on the mirror: mean 4.53e-9, var 8.42e-10, both at n = 5) and check_bank's plain lgssm rows (mean 4.08e-9, var 1.64e-9: 64
# particles within 2.4 of 0 average the float32 exp of each weight less than the wide rows do): the mean relative to max |x| of the
# row at the lag's time, the variance to max x^2.  Both backends are held to 4 x these (the device adds in another tree; past one
# tile it rescales).
MEASURED = {"mean": 4.6e-9, "var": 1.7e-9}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
DEVICE_VS_MIRROR = 1e-12               # n <= 1024: the same e_i bit for bit and an exact gather, only the summation order differs


@functools.lru_cache(maxsize=None)
def steps_of(n, R, D, L, k):
    """the L + 3 steps of run k, never modified: per step (lw [R, n], carry [R, n], x [D, R, n], row-local ancestors [R, n] or None)"""
    rng, out = np.random.default_rng(100000 * n + 1000 * R + 100 * D + 10 * L + k), []
    for t in range(L + 3):
        lw, shape = rng.normal(size=(R, n)).astype(np.float32), WEIGHTS[(t + k) % 4]
        if shape == "block":                             # a -inf block with a NaN beside it
            lw[:, n // 4:n // 4 + max(1, n // 3)] = -np.inf
            lw[:, n // 2] = np.nan
        elif shape == "dominant":
            lw[:, :n // 2] -= np.float32(1e4)
            lw[:, n // 2 + 1:] -= np.float32(1e4)
        elif shape == "norow":
            lw[R // 2] = -np.inf
        carry = (0.5 * rng.normal(size=(R, n))).astype(np.float32)
        carry[::2] = 0.0
        anc = {"uniform": rng.integers(0, n, size=(R, n)), "identity": np.tile(np.arange(n), (R, 1)),
               "one": np.full((R, n), n // 3), "reverse": np.tile(np.arange(n)[::-1], (R, 1))}[ANCESTORS[(t + k // 4) % 4]]
        out.append((lw, carry, (10.0 * rng.normal(size=(D, R, n)) + 100.0).astype(np.float32), anc.astype(np.int32) if t else None))
        for a in out[-1][:3]:
            a.setflags(write=False)
    return out


def reference(steps, t, l, with_carry):
    """[R, 2 D] float64: x_{t-l} along the composed ancestor tables under w = exp(a - max a) in float64, a = lw_t (+ carry_t, the add
    in float32), a NaN weight 0; and the row's max |x| at time t - l"""
    lw, carry, _, _ = steps[t]
    with np.errstate(invalid="ignore"):
        a = ((lw + carry).astype(np.float32) if with_carry else lw).astype(np.float64)
    (R, n), xs = a.shape, steps[t - l][2].astype(np.float64)
    b = np.tile(np.arange(n), (R, 1))
    for j in range(l):
        b = np.take_along_axis(steps[t - j][3].astype(np.int64), b, axis=1)
    out = np.full((R, 2 * xs.shape[0]), np.nan)
    for r in range(R):
        m = np.fmax.reduce(a[r])
        with np.errstate(invalid="ignore"):
            w = np.where(np.isnan(a[r]), 0.0, np.exp(a[r] - m)) if np.isfinite(m) else np.zeros(n)
        S0, z = w.sum(), xs[:, r, b[r]]
        if S0 > 0:
            mean = (w * z).sum(axis=1) / S0
            out[r] = np.concatenate([mean, np.maximum((w * z * z).sum(axis=1) / S0 - mean ** 2, 0.0)])
    return out, np.abs(xs).max(axis=(0, 2))


def deviations(got, want, top, dev, bound=None, what=()):
    """the (mean, var) deviations of one lag, scaled as MEASURED is, folded into dev and held to `bound`; no mass: NaN everywhere"""
    D = want.shape[1] // 2
    for r in range(want.shape[0]):
        if np.isnan(want[r, 0]):
            assert np.all(np.isnan(got[r])), (what, r, got[r])
            continue
        err = {"mean": float(np.abs(got[r, :D] - want[r, :D]).max()) / top[r], "var": float(np.abs(got[r, D:] - want[r, D:]).max()) / top[r] ** 2}
        assert bound is None or all(err[k] <= (bound[k] if isinstance(bound, dict) else bound) for k in err), (what, r, err, bound)
        dev.update({k: max(dev[k], err[k]) for k in err})


def run(be, n, R, D, L, k, with_carry, stride):
    """the steps of steps_of through the C-ABI on padded rows (ld = n + 3, x_row_stride = n + 5): at step t every lag 0 .. min(L, t)
    -> [t][lag] = [R, 2 D].  Nothing past an output or a ring slot is written, the rings hold what was recorded, the inputs keep
    their bits, the range (L, L) alone gives lag L's bits."""
    steps, ld, rs, W = steps_of(n, R, D, L, k), n + 3, n + 5, 2 * D
    x_ld, dev, c = R * rs, be.device, be.c
    ring_x, ring_a = np.full(((L + 1) * D * x_ld + 8,), np.float32(SENTINEL)), np.full(((L + 1) * R * ld + 8,), np.int32(-7))
    hx, ha = torch.from_numpy(ring_x.copy()).to(dev), torch.from_numpy(ring_a.copy()).to(dev)
    ws = torch.zeros(((int(c.gmx_rows_lag_moments_workspace(R, n, D, L)) + 7) // 8,), dtype=torch.int64, device=dev)
    got = []
    for t, (lw, carry, x, anc) in enumerate(steps):
        host = [np.full((R, ld), np.float32(SENTINEL)), np.full((R, ld), np.float32(SENTINEL)), np.full((D, x_ld), np.float32(SENTINEL)),
                np.full((R, ld), np.int32(-7))]
        host[0][:, :n], host[1][:, :n] = lw, carry
        host[2].reshape(D, R, rs)[:, :, :n] = x
        if t:
            host[3][:, :n] = anc + stride * np.arange(R, dtype=np.int32)[:, None]
        tl, tc, tx, ta = (torch.from_numpy(a.copy()).to(dev) for a in host)
        hi = min(L, t)

        def call(lo, hi, out):
            rc = c.gmx_rows_lag_moments(be.ptr(tl), be.ptr(tc) if with_carry else None, R, n, ld, be.ptr(tx), D, x_ld, rs,
                                        be.ptr(ta) if t else None, ld, stride, t, L, lo, hi, be.ptr(hx), x_ld, be.ptr(ha), ld,
                                        be.ptr(out), W + 2, (R + 1) * (W + 2), be.ptr(ws), be.stream())
            assert rc == 0, c.gmx_last_error()
            return out.cpu().numpy()
        out = torch.full((L + 2, R + 1, W + 2), SENTINEL, dtype=torch.float64, device=dev)
        if t == 0:
            assert np.all(call(0, -1, out) == SENTINEL), "the empty range wrote an output"
        full = call(0, hi, out)
        assert np.all(full[hi + 1:] == SENTINEL) and np.all(full[:, R] == SENTINEL) and np.all(full[:, :, W:] == SENTINEL), "written past the outputs"
        if t >= L:
            one = call(L, L, torch.full_like(out, SENTINEL))
            assert np.all(one[:L] == SENTINEL) and np.array_equal(one[L].view(np.int64), full[L].view(np.int64)), "the range (L, L) is not lag L of the full range"
        assert all(H.same_bits(d, h) for d, h in zip((tl, tc, tx, ta), host)), "an input was written"
        s = t % (L + 1)
        ring_x[:-8].reshape(L + 1, D, R, rs)[s, :, :, :n] = x
        if t:
            ring_a[:-8].reshape(L + 1, R, ld)[s, :, :n] = host[3][:, :n]
        assert H.same_bits(hx, ring_x) and H.same_bits(ha, ring_a), "the rings do not hold exactly what was recorded"
        got.append(full[:hi + 1, :R, :W].copy())
    return got


def check_size(be, n):
    """per L and R = 1, 3, 5 (3 and 5 leave a partly filled workgroup) one run, D, carry and index_stride in turn over the runs, the
    ancestor and weight shapes in turn over a run's steps: within TOL of the reference (the size's largest deviations are printed
    first: MEASURED) and, one tile, of the mirror"""
    dev, checks = {"mean": 0.0, "var": 0.0}, []
    for k, (L, R) in enumerate((L, R) for L in LAGS if n <= 1024 or L <= 5 for R in (1, 3, 5)):
        D, with_carry, stride = (1, 3)[k % 2], bool((k // 2) % 2), (0, n)[(k // 4) % 2]
        got = run(be, n, R, D, L, k, with_carry, stride)
        mirror = run(library("mirror"), n, R, D, L, k, with_carry, stride) if be.device.type == "cuda" and n <= 1024 else None
        for t, lags in enumerate(got):
            for l, g in enumerate(lags):
                want, top = reference(steps_of(n, R, D, L, k), t, l, with_carry)
                deviations(g, want, top, dev)
                checks.append(((n, R, D, L, t, l), g, want, top))
                if mirror is not None:
                    deviations(g, mirror[t][l], top, dict(dev), DEVICE_VS_MIRROR, ("device against mirror", n, R, D, L, t, l))
    print("n", n, dev, "allowed", TOL)
    for what, g, want, top in checks:
        deviations(g, want, top, dict(dev), TOL, what)


def check_refusals_of(lib):
    buf = (ctypes.c_int64 * 8)()
    P, N = ctypes.cast(buf, ctypes.c_void_p), None
    def call(lw=P, rows=2, n=10, ld=10, x=P, D=2, x_ld=20, x_rs=10, anc=P, a_ld=10, stride=10, t=3, L=2, lo=2, hi=2, hx=P, hx_ld=20,
             ha=P, ha_ld=10, out=P, out_ld=4, ws=P):
        return lw, N, rows, n, ld, x, D, x_ld, x_rs, anc, a_ld, stride, t, L, lo, hi, hx, hx_ld, ha, ha_ld, out, out_ld, 8, ws, N
    calls = [(call(lw=N), b"null"), (call(hx=N), b"null"), (call(ha=N), b"null"), (call(out=N), b"null"), (call(ws=N), b"null"),
             (call(x=N), b"x_d"), (call(D=0), b"D = 0"), (call(n=0), b"n = 0"), (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, x_ld=2 ** 23), b"n = 2097153"),
             (call(rows=-1), b"rows = -1"), (call(ld=9), b"ld = 9"), (call(x_ld=19), b"x_ld = 19"), (call(stride=2 ** 31), b"index_stride = 2147483648"),
             (call(L=0, lo=0, hi=0), b"L = 0"), (call(L=33), b"L = 33"), (call(t=-1), b"t = -1"), (call(lo=-1), b"lag_lo = -1"),
             (call(lo=2, hi=1), b"lag_lo = 2"), (call(hi=3, t=5), b"lag_hi = 3"), (call(t=1), b"lag_hi = 2"), (call(a_ld=9), b"a_ld = 9"),
             (call(ha_ld=9), b"hist_a_ld = 9"), (call(hx_ld=19), b"hist_x_ld = 19"), (call(out_ld=3), b"out_ld = 3"),
             (call(anc=N), b"ancestors_d with t = 3")]
    for args, names in calls:
        assert lib.gmx_rows_lag_moments(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_rows_lag_moments" in msg and names in msg, (msg, names)
    sizes = [int(lib.gmx_rows_lag_moments_workspace(*a)) for a in ((3, 1024, 2, 8), (3, 1025, 2, 8), (3, 1025, 2, 33))]
    assert sizes == [16, (6 * ((1 + 2 * 9) * 16 + 4) + 15) // 16 * 16, 16]         # 6 cells x (19 pairs of doubles + a float)


# --- BootstrapBank(smooth_lag=L): R = 3 filters ----------------------------------------------------------------------------
BANKS = [dict(), dict(ess_threshold=0.5), dict(model="tracker"), dict(T=2, smooth_lag=5)]      # the last: a flush shorter than the lag


def check_bank(be, specialize, capture=False, model="lgssm", n=64, T=5, smooth_lag=2, **kw):
    """(a) log_ml, state and ancestors are the plain bank's bits; (b) row T - 1 is filter_mean() / filter_var() of a moments=True
    bank; (c) plain lgssm: every row meets the reference on that key's BootstrapSweep history; (d) two captured replays are the
    eager bits; the named refusals raise"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    init, step = K._models(model)
    keys, ys, R = G.split(G.key(M.BK_SEED), M.BK_R), K._data(T), M.BK_R
    plain, bank, mom = (smc.BootstrapBank(init, step, n, R, T, specialize=specialize, **kw, **m).prepare(keys, ys)
                        for m in (dict(), dict(smooth_lag=smooth_lag), dict(moments=True)))
    for b in (plain, bank, mom):
        b.launch()
    (x, lw, anc), (px, plw, panc) = K._np_state(bank.state()), K._np_state(plain.state())
    assert H.same_bits(x, px) and H.same_bits(lw, plw) and np.array_equal(anc, panc) and np.array_equal(bank.log_ml(), plain.log_ml())
    for bad in (plain.smoothed_mean, plain.smoothed_var):
        with pytest.raises(ValueError, match="smooth_lag=L"):
            bad()
    with pytest.raises(NotImplementedError, match="smooth_lag"):
        smc.ConditionalBank(init, step, n, R, T, smooth_lag=2)
    for bad in (0, 33, 1.5):
        with pytest.raises(ValueError, match="smooth_lag"):
            smc.BootstrapBank(init, step, n, R, T, smooth_lag=bad)
    mean, var, rec = bank.smoothed_mean(), bank.smoothed_var(), bank.smo.cpu().numpy().copy()
    D = rec.shape[2] // 2
    assert mean.shape == ((T, R) if D == 1 else (T, R, D)) and var.shape == mean.shape and mean.dtype == torch.float64
    for a, b in ((mean, mom.filter_mean()), (var, mom.filter_var())):
        assert np.all(np.abs(a[T - 1].numpy() - b[T - 1].numpy()) <= 1e-12 * np.abs(b[T - 1].numpy())), (a[T - 1], b[T - 1])
    if model == "lgssm" and not kw:
        for r in range(R):
            sw = smc.BootstrapSweep(init, step, n, T, specialize=specialize, history=True).prepare(keys[r], ys)
            sw.launch()
            h = sw.history()
            hx, hlw, ha = (v.cpu().numpy() for v in (h.x, h.log_weights, h.ancestors))
            steps = [(hlw[t][None], None, hx[t][None, None], ha[t - 1][None] if t else None) for t in range(T)]
            dev, checks = {"mean": 0.0, "var": 0.0}, []
            for s in range(T):
                t = min(s + smooth_lag, T - 1)
                checks.append((rec[s, r][None],) + reference(steps, t, t - s, False))
                deviations(*checks[-1], dev)
            print("bank row", r, dev, "allowed", TOL)
            for s, c in enumerate(checks):
                deviations(*c, dict(dev), TOL, ("bank", r, s))
    if capture:
        bank.smo.zero_()
        bank.capture()
        bank.launch()
        bank.launch()                    # two replays
        assert np.array_equal(bank.smo.cpu().numpy().view(np.int64), rec.view(np.int64))
