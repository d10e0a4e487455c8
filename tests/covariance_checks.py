"""Drivers of tests/test_covariance_cpu.py (the CPU mirror) and tests/test_covariance_gpu.py (the HIP library): gmx_rows_covariance
against numpy float64 on the same float32 inputs, its refusals and sizes, and smc.BootstrapBank(covariance=True)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bank_checks as K
from tests import history_checks as H
from tests import moments_checks as M
from tests.moments_checks import case, library

SIZES = [1, 5, 17, 255, 256, 257, 513, 1024,             # the 4-column k-step, the 16-column block, the packing changes at 256 and 512
         1025, 2049, 3000]                               # a 1-column tail tile, three tiles, a ragged last tile
SENTINEL = -7.5
# The mirror's largest deviations from the reference, MEASURED over exactly check_size's cases (its printed maxima on the mirror:
# mean 3.94e-9, cov 7.19e-10): the mean relative to max |x| of the row, the covariance to max x^2 — the float32 exp of each weight.
# Both backends are held to 4 x these (the device adds in another tree; past one tile it rescales).
MEASURED = {"mean": 4.0e-9, "cov": 7.2e-10}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
DEVICE_VS_MIRROR = 1e-12               # n <= 1024: the same e_i bit for bit, only the float64 summation order differs


def reference(lw, carry, x):
    """[R, D + D^2] float64: a = lw (+ carry, the add in float32), w = exp(a - max) in float64; x is [D, R, n]"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = (lw if carry is None else (lw + carry).astype(np.float32)).astype(np.float64)
    D = x.shape[0]
    out = np.full((a.shape[0], D + D * D), np.nan)
    for r, row in enumerate(a):
        w = np.exp(row - row.max()) if np.isfinite(row.max()) else np.zeros_like(row)
        S0, x64 = w.sum(), x[:, r].astype(np.float64)
        if S0 > 0:
            mean = (w * x64).sum(axis=1) / S0
            cov = (w * x64) @ x64.T / S0 - np.outer(mean, mean)
            cov[np.diag_indices(D)] = np.maximum(np.diag(cov), 0.0)
            out[r] = np.concatenate([mean, cov.reshape(-1)])
    return out


def deviations(got, want, x, bound=None, what=()):
    """the (mean, cov) deviations, scaled as MEASURED is, held to `bound` (one, or one per name); cov symmetric bit for bit; no mass:
    NaN everywhere"""
    D, dev = x.shape[0], {"mean": 0.0, "cov": 0.0}
    for r in range(want.shape[0]):
        cov = got[r, D:].reshape(D, D)
        assert np.array_equal(cov.view(np.int64), cov.T.view(np.int64)), (what, r, "cov_jk and cov_kj differ")
        if np.isnan(want[r, 0]):
            assert np.all(np.isnan(got[r])), (what, r, got[r])
            continue
        top, err = float(np.abs(x[:, r].astype(np.float64)).max()), np.abs(got[r] - want[r])
        dev["mean"] = max(dev["mean"], float(err[:D].max()) / top)
        dev["cov"] = max(dev["cov"], float(err[D:].max()) / (top * top))
    assert bound is None or all(v <= (bound[k] if isinstance(bound, dict) else bound) for k, v in dev.items()), (what, dev, bound)
    return dev


def rows_covariance(be, lw, carry, x, pad=0, xpad=0):
    """rows ld = n + pad apart, the store's rows n + xpad apart; outputs past what may be written, and the inputs, keep their words"""
    (R, n), D = lw.shape, x.shape[0]
    ld, rs, x_ld, W = n + pad, n + xpad, R * (n + xpad), D + D * D
    host = [np.full((R, ld), np.float32(SENTINEL)), np.full((R, ld), np.float32(SENTINEL)), np.full((D, x_ld), np.float32(SENTINEL))]
    host[0][:, :n], host[1][:, :n] = lw, (0.0 if carry is None else carry)
    for r in range(R):
        host[2][:, r * rs:r * rs + n] = x[:, r]
    tl, tc, tx = (torch.from_numpy(a.copy()).to(be.device) for a in host)
    out = torch.full((R + 1, W + 2), SENTINEL, dtype=torch.float64, device=be.device)
    ws = torch.zeros(((int(be.c.gmx_rows_covariance_workspace(R, n, D)) + 7) // 8,), dtype=torch.int64, device=be.device)
    rc = be.c.gmx_rows_covariance(be.ptr(tl), be.ptr(tc) if carry is not None else None, R, n, ld, be.ptr(tx), D, x_ld, rs,
                                  be.ptr(out), int(out.shape[1]), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    got = out.cpu().numpy()
    assert np.all(got[R] == SENTINEL) and np.all(got[:R, W:] == SENTINEL), "written past the outputs"
    assert all(H.same_bits(t, h) for t, h in zip((tl, tc, tx), host)), "an input was written"
    return got[:R, :W]


def check_size(be, n):
    """1, 3, 5 rows, D = 1, 3, 15, every shape and carry, ld = n + 3, x_row_stride = n + 5: within TOL of the reference (the size's
    largest deviations are printed first: MEASURED) and, one tile, of the mirror"""
    devs = []
    calls = [(R, D, s, c, 0, 0) for R in (1, 3, 5) for D in (1, 3, 15) for s in M.SHAPES[:(6 if n > 1024 else 4)] for c in (False, True)]
    for R, D, shape, with_carry, pad, xpad in calls + [(3, 1, "normal", True, 3, 0), (3, 3, "block", False, 0, 5)]:
        lw, carry, x = case(n, R, D, shape)
        carry = carry if with_carry else None
        want = reference(lw, carry, x)
        assert shape != "norow" or np.isnan(want[R // 2, 0])
        got = rows_covariance(be, lw, carry, x, pad, xpad)
        devs.append(((n, R, D, shape, with_carry), got, want, x))
        if be.device.type == "cuda" and n <= 1024:
            deviations(got, rows_covariance(library("mirror"), lw, carry, x, pad, xpad), x, DEVICE_VS_MIRROR, "device against mirror")
    print("n", n, {k: max(deviations(*d[1:])[k] for d in devs) for k in TOL}, "allowed", TOL)
    for what, got, want, x in devs:
        deviations(got, want, x, TOL, what)


def check_refusals_of(lib):
    buf = (ctypes.c_int64 * 8)()
    P, N = ctypes.cast(buf, ctypes.c_void_p), None
    def call(lw=P, rows=2, n=10, ld=10, x=P, D=2, x_ld=20, x_rs=10, out=P, out_ld=6, ws=P):
        return lw, N, rows, n, ld, x, D, x_ld, x_rs, out, out_ld, ws, N
    calls = [(call(lw=N), b"null"), (call(out=N), b"null"), (call(ws=N), b"null"), (call(x=N), b"x_d"), (call(D=0), b"D = 0"),
             (call(D=16, out_ld=2 ** 20), b"D = 16"), (call(out_ld=5), b"out_ld = 5"), (call(ld=9), b"ld = 9"), (call(n=0), b"n = 0"),
             (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, x_ld=2 ** 23), b"n = 2097153")]
    for args, names in calls:
        assert lib.gmx_rows_covariance(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_rows_covariance" in msg and names in msg, (msg, names)
    sizes = [int(lib.gmx_rows_covariance_workspace(*a)) for a in ((3, 1024, 2), (3, 1025, 2))]
    assert sizes == [16, (6 * (136 * 8 + 4) + 15) // 16 * 16]            # 6 cells x (136 doubles + a float)


# --- BootstrapBank(covariance=True): R = 3 filters -------------------------------------------------------------------------
BANKS = [dict(model="tracker"), dict(model="tracker", ess_threshold=0.5), dict(model="tracker", n=1030, T=2), dict()]


def check_bank(be, specialize, capture=False, model="lgssm", n=64, T=4, **kw):
    """(a) log_ml, state and ancestors are the plain bank's bits; (b) the last step's record is the reference's on state() and
    smc.row_covariance's bits, its diagonal filter_var() of a moments=True bank; (c) two captured replays are the eager bits"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    init, step = K._models(model)
    keys, ys = G.split(G.key(M.BK_SEED), M.BK_R), K._data(T)
    plain, bank, mom = (smc.BootstrapBank(init, step, n, M.BK_R, T, specialize=specialize, **kw, **m).prepare(keys, ys)
                        for m in (dict(), dict(covariance=True), dict(moments=True)))
    for b in (plain, bank, mom):
        b.launch()
    (x, lw, anc), (px, plw, panc) = K._np_state(bank.state()), K._np_state(plain.state())
    assert H.same_bits(x, px) and H.same_bits(lw, plw) and np.array_equal(anc, panc) and np.array_equal(bank.log_ml(), plain.log_ml())
    with pytest.raises(ValueError, match="covariance=True"):
        plain.filter_cov()
    with pytest.raises(NotImplementedError, match="covariance"):
        smc.ConditionalBank(init, step, n, M.BK_R, T, covariance=True)
    x = x[None] if x.ndim == 2 else np.ascontiguousarray(np.moveaxis(x, 2, 0))
    D = x.shape[0]
    cov, rec = bank.filter_cov(), bank.cov.cpu().numpy().copy()
    assert cov.shape == (T, M.BK_R, D, D) and cov.dtype == torch.float64
    deviations(rec[T - 1], reference(lw, None, x), x, TOL)
    again = smc.row_covariance(bank.state()[1], bank.state()[0])
    assert torch.equal(again[1].cpu(), cov[T - 1]) and torch.equal(again[0].cpu().reshape(M.BK_R, D), bank.cov[T - 1, :, :D].cpu())
    top2 = np.abs(x.astype(np.float64)).max(axis=(0, 2)) ** 2
    diff = np.abs(np.diagonal(cov[T - 1].numpy(), axis1=1, axis2=2) - mom.filter_var()[T - 1].numpy().reshape(M.BK_R, D))
    assert np.all(diff <= (M.TOL["var"] + TOL["cov"]) * top2[:, None]), diff
    if capture:
        bank.cov.zero_()
        bank.capture()
        bank.launch()
        bank.launch()                    # two replays
        assert np.array_equal(bank.cov.cpu().numpy().view(np.int64), rec.view(np.int64))
