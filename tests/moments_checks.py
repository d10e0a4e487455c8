"""Drivers of tests/test_moments_cpu.py (the CPU mirror) and tests/test_moments_gpu.py (the HIP library): gmx_rows_moments against
numpy float64 on the same float32 inputs, its refusals and sizes, and smc.BootstrapBank(moments=True)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genjax_amd import _lib
from tests import bank_checks as K
from tests import history_checks as H

SIZES = [1, 5, 255, 256, 257, 513, 1023, 1024,           # one tile: the packing changes at 256 and 512
         1025, 2049, 3000]                               # a 1-column tail tile, three tiles, a ragged last tile
SHAPES = ["normal", "block", "norow", "dominant", "tile_inf", "max_last"]          # the last two: tiled sizes only
SENTINEL = -7.5
# The mirror's largest deviations from the reference, MEASURED over exactly check_size's cases (its printed maxima on the mirror:
# ess 3.06e-8, mean 3.94e-9, var 3.58e-10): the ESS relative to itself, the mean to max |x| of the row, the variance to max x^2 —
# the float32 exp of each weight.  Both backends are held to 4 x these (the device adds in another tree; past one tile it rescales).
MEASURED = {"ess": 3.1e-8, "mean": 4.0e-9, "var": 3.6e-10}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
DEVICE_VS_MIRROR = 1e-12               # n <= 1024: the same e_i bit for bit, only the float64 summation order differs


@functools.lru_cache(maxsize=None)
def library(which):
    import tests.hostsim as hs
    return _lib.Backend(ctypes.CDLL(hs.build() if which == "mirror" else _lib.LIB_PATH), torch.device("cpu"), uses_streams=False)


def reference(lw, carry, x):
    """[R, 1 + 2 D] float64: a = lw (+ carry, the add in float32), w = exp(a - max) in float64; x is [D, R, n]"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = (lw if carry is None else (lw + carry).astype(np.float32)).astype(np.float64)
    D = x.shape[0]
    out = np.full((a.shape[0], 1 + 2 * D), np.nan)
    for r, row in enumerate(a):
        w = np.exp(row - row.max()) if np.isfinite(row.max()) else np.zeros_like(row)
        S0, x64 = w.sum(), x[:, r].astype(np.float64)
        out[r, 0] = S0 * S0 / np.sum(w * w) if S0 > 0 else 0.0
        if S0 > 0:
            out[r, 1:1 + D] = (w * x64).sum(axis=1) / S0
            out[r, 1 + D:] = np.maximum((w * x64 * x64).sum(axis=1) / S0 - out[r, 1:1 + D] ** 2, 0.0)
    return out


def deviations(got, want, x, bound=None, what=()):
    """the (ess, mean, var) deviations, scaled as MEASURED is, held to `bound` (one, or one per name); no mass: ESS 0, NaN, exactly"""
    D, dev = x.shape[0], {"ess": 0.0, "mean": 0.0, "var": 0.0}
    for r in range(want.shape[0]):
        if want[r, 0] == 0.0:
            assert np.array_equal(got[r], want[r], equal_nan=True), (r, got[r], want[r])
            continue
        top, err = float(np.abs(x[:, r].astype(np.float64)).max()) if D else 1.0, np.abs(got[r] - want[r])
        dev["ess"] = max(dev["ess"], err[0] / want[r, 0])
        dev["mean"] = max(dev["mean"], float(err[1:1 + D].max(initial=0.0)) / top)
        dev["var"] = max(dev["var"], float(err[1 + D:].max(initial=0.0)) / (top * top))
    assert bound is None or all(v <= (bound[k] if isinstance(bound, dict) else bound) for k, v in dev.items()), (what, dev, bound)
    return dev


def rows_moments(be, lw, carry, x, pad=0, xpad=0):
    """rows ld = n + pad apart, the store's rows n + xpad apart; outputs past what may be written, and the inputs, keep their words"""
    (R, n), D = lw.shape, x.shape[0]
    ld, rs, x_ld = n + pad, n + xpad, R * (n + xpad)
    host = [np.full((R, ld), np.float32(SENTINEL)), np.full((R, ld), np.float32(SENTINEL)), np.full((max(D, 1), x_ld), np.float32(SENTINEL))]
    host[0][:, :n], host[1][:, :n] = lw, (0.0 if carry is None else carry)
    for r in range(R):
        host[2][:D, r * rs:r * rs + n] = x[:, r]
    tl, tc, tx = (torch.from_numpy(a.copy()).to(be.device) for a in host)
    out = torch.full((R + 1, 1 + 2 * D + 2), SENTINEL, dtype=torch.float64, device=be.device)
    ws = torch.zeros(((int(be.c.gmx_rows_moments_workspace(R, n, D)) + 7) // 8,), dtype=torch.int64, device=be.device)
    rc = be.c.gmx_rows_moments(be.ptr(tl), be.ptr(tc) if carry is not None else None, R, n, ld, be.ptr(tx) if D else None, D, x_ld,
                               rs, be.ptr(out), int(out.shape[1]), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    got = out.cpu().numpy()
    assert np.all(got[R] == SENTINEL) and np.all(got[:R, 1 + 2 * D:] == SENTINEL), "written past the outputs"
    assert all(H.same_bits(t, h) for t, h in zip((tl, tc, tx), host)), "an input was written"
    return got[:R, :1 + 2 * D]


@functools.lru_cache(maxsize=None)
def case(n, R, D, shape):
    """(lw [R, n], carry [R, n], x [D, R, n]) float32, never modified: states 10 z + 100 (a variance beside a nonzero mean)"""
    rng = np.random.default_rng(1000 * n + 10 * R + D + 7 * len(shape))
    lw = rng.normal(size=(R, n)).astype(np.float32)
    holes = {"block": np.s_[:, n // 4:n // 4 + max(1, n // 3)], "norow": np.s_[R // 2], "tile_inf": np.s_[:, 1024:2048]}
    if shape in holes:
        lw[holes[shape]] = -np.inf
    elif shape == "dominant":                            # ESS ~ 1: every other column 1e4 below
        lw[:, :n // 2] -= np.float32(1e4)
        lw[:, n // 2 + 1:] -= np.float32(1e4)
    elif shape == "max_last":
        lw[:, n - 1] = 9.0
    carry = (0.5 * rng.normal(size=(R, n))).astype(np.float32)
    carry[::2] = 0.0
    out = lw, carry, (10.0 * rng.normal(size=(D, R, n)) + 100.0).astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out


def check_size(be, n):
    """1, 3, 5 rows (3 and 5 leave a partly filled workgroup at W = 1 and 2), every D, shape and carry, ld = n + 3, x_row_stride = n + 5:
    within TOL of the reference (the size's largest deviations are printed first: MEASURED) and, one tile, of the mirror"""
    devs = []
    calls = [(R, D, s, c, 0, 0) for R in (1, 3, 5) for D in (0, 1, 3) for s in SHAPES[:(6 if n > 1024 else 4)] for c in (False, True)]
    for R, D, shape, with_carry, pad, xpad in calls + [(3, 1, "normal", True, 3, 0), (3, 3, "block", False, 0, 5)]:
        lw, carry, x = case(n, R, D, shape)
        carry = carry if with_carry else None
        want = reference(lw, carry, x)
        assert (shape != "norow" or want[R // 2, 0] == 0.0) and (shape != "dominant" or np.all(np.abs(want[:, 0] - 1.0) < 1e-6))
        got = rows_moments(be, lw, carry, x, pad, xpad)
        devs.append(((n, R, D, shape, with_carry), got, want, x))
        if be.device.type == "cuda" and n <= 1024:
            deviations(got, rows_moments(library("mirror"), lw, carry, x, pad, xpad), x, DEVICE_VS_MIRROR, "device against mirror")
    print("n", n, {k: max(deviations(*d[1:])[k] for d in devs) for k in TOL}, "allowed", TOL)
    for what, got, want, x in devs:
        deviations(got, want, x, TOL, what)


def check_refusals_of(lib):
    buf = (ctypes.c_int64 * 8)()
    P, N = ctypes.cast(buf, ctypes.c_void_p), None
    def call(lw=P, rows=2, n=10, ld=10, x=P, D=1, x_ld=20, x_rs=10, out=P, out_ld=3, ws=P):
        return lw, N, rows, n, ld, x, D, x_ld, x_rs, out, out_ld, ws, N
    calls = [(call(lw=N), b"null"), (call(out=N), b"null"), (call(ws=N), b"null"), (call(n=0), b"n = 0"),
             (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, x_ld=2 ** 23), b"n = 2097153"), (call(rows=-1), b"rows = -1"),
             (call(rows=2 ** 21, n=1024, ld=1024, x_ld=2 ** 32, x_rs=1024), b"rows = 2097152"), (call(ld=9), b"ld = 9"),
             (call(D=-1), b"D = -1"), (call(D=65534, out_ld=2 ** 20), b"D = 65534"), (call(out_ld=2), b"out_ld = 2"),
             (call(x=N), b"x_d"), (call(x_ld=19), b"x_ld = 19")]
    for args, names in calls:
        assert lib.gmx_rows_moments(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_rows_moments" in msg and names in msg, (msg, names)
    assert [int(lib.gmx_rows_moments_workspace(*a)) for a in ((3, 1024, 2), (3, 1025, 2), (0, 5, 0))] == [16, 320, 16]      # 6 cells x (6 doubles + a float)


# --- BootstrapBank(moments=True): R = 3 filters ---------------------------------------------------------------------------
BK_R, BK_SEED = 3, 4242
BANKS = [dict(), dict(ess_threshold=0.5), dict(model="tracker", n=1030, T=2)]      # the last: D = 2, the tiled form in the sweep


def check_bank(be, specialize, capture=False, model="lgssm", n=64, T=4, **kw):
    """(a) log_ml, state and ancestors are the plain bank's bits; (b) the last step's moments are the reference's on state() and
    smc.row_moments' bits; (c) plain lgssm: filter_mean() is each key's BootstrapSweep history's, a captured replay the eager bits"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    init, step = K._models(model)
    keys, ys = G.split(G.key(BK_SEED), BK_R), K._data(T)
    plain, bank = (smc.BootstrapBank(init, step, n, BK_R, T, specialize=specialize, **kw, **m).prepare(keys, ys)
                   for m in (dict(), dict(moments=True)))
    plain.launch()
    bank.launch()
    (x, lw, anc), (px, plw, panc) = K._np_state(bank.state()), K._np_state(plain.state())
    assert H.same_bits(x, px) and H.same_bits(lw, plw) and np.array_equal(anc, panc) and np.array_equal(bank.log_ml(), plain.log_ml())
    with pytest.raises(ValueError, match="moments=True"):
        plain.filter_mean()
    with pytest.raises(NotImplementedError, match="moments"):
        smc.ConditionalBank(init, step, n, BK_R, T, moments=True)
    x = x[None] if x.ndim == 2 else np.ascontiguousarray(np.moveaxis(x, 2, 0))
    D = x.shape[0]
    mean, var, ess, mom = bank.filter_mean(), bank.filter_var(), bank.ess(), bank.mom.cpu().numpy().copy()
    assert mean.shape == ((T, BK_R) if D == 1 else (T, BK_R, D)) and var.shape == mean.shape and ess.shape == (T, BK_R)
    got = torch.cat([ess[T - 1][:, None], mean[T - 1].reshape(BK_R, D), var[T - 1].reshape(BK_R, D)], dim=1).numpy()
    deviations(got, reference(lw, None, x), x, TOL)
    again = smc.row_moments(bank.state()[1], bank.state()[0])
    assert all(torch.equal(a.cpu(), b[T - 1]) for a, b in zip(again, (ess, mean, var)))
    if model != "lgssm" or kw:
        return
    for r in range(BK_R):
        sw = smc.BootstrapSweep(init, step, n, T, specialize=specialize, history=True).prepare(keys[r], ys)
        sw.launch()
        want, top = sw.history().filter_mean().cpu().numpy(), float(sw.history().x.abs().max())
        assert np.abs(mean[:, r].numpy() - want).max() <= TOL["mean"] * top, (r, mean[:, r], want)
    if capture:
        bank.mom.zero_()
        bank.capture()
        bank.launch()
        bank.launch()                    # two replays
        assert np.array_equal(bank.mom.cpu().numpy().view(np.int64), mom.view(np.int64))
