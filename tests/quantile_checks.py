"""Drivers of tests/test_quantiles_cpu.py (the CPU mirror) and tests/test_quantiles_gpu.py (the HIP library): gmx_rows_quantiles bit
for bit against a reference in Python integers, the definition against float64, its refusals, smc.BootstrapBank(quantiles=)."""
import bisect
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from tests import bank_checks as K
from tests import history_checks as H
from tests.moments_checks import library

SIZES = [1, 5, 255, 256, 257, 512, 513, 1023, 1024]      # the packing changes at 256 and 512; 1023: a ragged last thread
SHAPES = ["normal", "block", "dominant", "ascending", "descending", "top", "norow", "ties"]
ONE, SENTINEL, NAN_BITS, PROBS = 2 ** 32, -7.5, 0x7FC00000, (0.025, 0.5, 0.975)
LEVELS = [0, 1, round(0.025 * ONE), 2 ** 31, round(0.975 * ONE), ONE]
# The smallest eps the integer reference needs in definition_eps, MEASURED over exactly check_size's tie-free cases: 0.0 at every
# size (printed).  The float32 exp and the truncation move a cumulative weight by some 1e-7 of the total, which changes the particle
# only where a level lies that close to a step of F — none of these cases — and F is summed exactly (math.fsum).  Held to 4 x it.
MEASURED = 0.0
EPS = 4.0 * MEASURED


def fixed_weights(a):
    """the row's fixed-point weights as Python integers: the increments of gmx_weight_cdf (the mirror's) of the row alone"""
    be, n = library("mirror"), a.size
    row, mx = torch.from_numpy(a.copy()), torch.tensor([np.fmax.reduce(a, initial=-np.inf)], dtype=torch.float32)
    cdf, total = torch.zeros(n, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    ws = torch.zeros((int(be.c.gmx_weight_cdf_workspace(n)) + 7) // 8, dtype=torch.int64)
    assert be.c.gmx_weight_cdf(be.ptr(row), n, 62 - (n - 1).bit_length(), None, 0, be.ptr(mx), be.ptr(cdf), be.ptr(total), be.ptr(ws), None) == 0
    return [int(v) for v in np.diff(cdf.numpy().view(np.uint64).astype(object), prepend=0)]


def reference(a, x, levels):
    """uint32 [R, D, Q]: per row of a = lw (+ carry, added in float32) the integer weights, then per component a stable argsort of
    the key, the cumulative sum in Python integers and the first position that reaches T; x is [D, R, n]"""
    D, R, n = x.shape
    out = np.full((R, D, len(levels)), NAN_BITS, dtype=np.uint32)
    for r in range(R):
        q = fixed_weights(a[r])
        total = sum(q)
        for d in range(D if total else 0):
            bits = np.ascontiguousarray(x[d, r]).view(np.uint32)
            order = np.argsort(np.where(bits >> 31, ~bits, bits ^ np.uint32(0x80000000)), kind="stable")
            C = list(itertools.accumulate(q[i] for i in order))
            for j, lv in enumerate(levels):
                out[r, d, j] = bits[order[bisect.bisect_left(C, max(1, (lv * total + ONE - 1) >> 32))]]
    return out


def rows_quantiles(be, lw, carry, x, levels, pad=3, xpad=5):
    """rows ld = n + pad apart, the store's rows n + xpad apart; words past the outputs, and the inputs, keep their bits"""
    (R, n), D, Q = lw.shape, x.shape[0], len(levels)
    ld, rs, x_ld = n + pad, n + xpad, R * (n + xpad)
    host = [np.full((R, ld), np.float32(SENTINEL)), np.full((R, ld), np.float32(SENTINEL)), np.full((D, x_ld), np.float32(SENTINEL))]
    host[0][:, :n], host[1][:, :n] = lw, (0.0 if carry is None else carry)
    for r in range(R):
        host[2][:, r * rs:r * rs + n] = x[:, r]
    tl, tc, tx = (torch.from_numpy(a.copy()).to(be.device) for a in host)
    lv = torch.tensor(levels, dtype=torch.int64, device=be.device)
    out = torch.full((R + 1, D * Q + 2), SENTINEL, dtype=torch.float32, device=be.device)
    assert be.c.gmx_rows_quantiles(be.ptr(tl), be.ptr(tc) if carry is not None else None, R, n, ld, be.ptr(tx), D, x_ld, rs, be.ptr(lv),
                                   Q, be.ptr(out), int(out.shape[1]), be.stream()) == 0, be.c.gmx_last_error()
    got = out.cpu().numpy()
    assert np.all(got[R] == SENTINEL) and np.all(got[:R, D * Q:] == SENTINEL), "written past the outputs"
    assert all(H.same_bits(t, h) for t, h in zip((tl, tc, tx), host)) and lv.tolist() == levels, "an input was written"
    return np.ascontiguousarray(got[:R, :D * Q]).view(np.uint32).reshape(R, D, Q)


def case(n, R, D, shape):
    """(lw [R, n], carry [R, n], x [D, R, n]) float32, a function of its arguments"""
    rng = np.random.default_rng(1000 * n + 10 * R + D + 7 * SHAPES.index(shape))
    lw = rng.normal(size=(R, n)).astype(np.float32)
    x = (10.0 * rng.normal(size=(D, R, n)) + 100.0).astype(np.float32)
    if shape == "block":                                 # a block of -inf, and a NaN weight: both count 0
        lw[:, n // 4:n // 4 + max(1, n // 3)] = -np.inf
        lw[:, n // 2] = np.nan if n > 2 else lw[:, n // 2]
    elif shape == "norow":
        lw[R // 2] = -np.inf
    elif shape == "dominant":
        lw[:, np.arange(n) != n // 2] -= np.float32(1e4)
    elif shape in ("ascending", "descending"):
        x = np.sort(x, axis=2)[:, :, ::(1 if shape == "ascending" else -1)].copy()
    elif shape == "top":                                 # all weight on the column with the largest state of component 0
        lw[:] = -np.inf
        lw[np.arange(R), x[0].argmax(axis=1)] = 1.0
    elif shape == "ties":                                # -1, -0.0, +0.0, 1 and both infinities
        x = np.round(np.clip(rng.normal(size=(D, R, n)), -1, 1)).astype(np.float32)
        x[:, :, ::7], x[:, :, 3::11] = np.inf, -np.inf
    return lw, (0.5 * rng.normal(size=(R, n))).astype(np.float32), x


def definition_eps(a, x, got):
    """the smallest eps with F(v-) <= p + eps and F(v) >= p - eps for every non-NaN output v: w = exp(a - max a) in float64,
    F(v) = sum { w_i : x_i <= v } / sum w, F(v-) the same over x_i < v — no library arithmetic"""
    a, eps = a.astype(np.float64), 0.0
    for (r, d, j), v in np.ndenumerate(got.view(np.float32)):
        if not np.isnan(v):
            w, xs, p = np.nan_to_num(np.exp(a[r] - np.nanmax(a[r])), nan=0.0), x[d, r], LEVELS[j] / ONE
            eps = max(eps, math.fsum(w[xs < v]) / math.fsum(w) - p, p - math.fsum(w[xs <= v]) / math.fsum(w))
    return eps


def check_size(be, n):
    """rows 1, 3, 5 (partly filled workgroups at W = 1, 2), D 1 and 3, carry on and off, every shape, ld = n + 3 and x_row_stride =
    n + 5: the reference's bits; the tie-free shapes also meet the float64 definition within EPS (the size's eps is printed)"""
    worst = 0.0
    for R, D, shape, with_carry in itertools.product((1, 3, 5), (1, 3), SHAPES, (False, True)):
        lw, carry, x = case(n, R, D, shape)
        a = lw + carry if with_carry else lw
        want, got = reference(a, x, LEVELS), rows_quantiles(be, lw, carry if with_carry else None, x, LEVELS)
        assert np.array_equal(got, want) and (shape != "norow" or np.all(got[R // 2] == NAN_BITS)), (n, R, D, shape, with_carry, got, want)
        if shape in SHAPES[:6]:                          # finite, distinct states: what the float64 check takes
            worst = max(worst, definition_eps(a, x, got))
    print("n", n, "eps needed", worst, "allowed", EPS)
    assert worst <= EPS, (n, worst, EPS)


def check_refusals_of(lib):
    buf, big = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 2)(ONE, ONE + 1)
    P, N = ctypes.cast(buf, ctypes.c_void_p), None
    def call(lw=P, n=10, ld=10, x=P, D=1, x_ld=20, lv=P, Q=2, out=P, out_ld=2):
        return lw, N, 2, n, ld, x, D, x_ld, 10, lv, Q, out, out_ld, N
    calls = [(call(lw=N), b"null"), (call(x=N), b"null"), (call(lv=N), b"null"), (call(out=N), b"null"), (call(n=0), b"n = 0"),
             (call(n=1025, ld=1025, x_ld=4096), b"n = 1025"), (call(D=0), b"D = 0"), (call(Q=0), b"Q = 0"), (call(Q=17, out_ld=17), b"Q = 17"),
             (call(lv=ctypes.cast(big, ctypes.c_void_p)), b"level of 4294967297"), (call(ld=9), b"ld = 9"),
             (call(D=2, x_ld=40, out_ld=3), b"out_ld = 3"), (call(x_ld=19), b"x_ld = 19")]
    for args, names in calls:
        rc, msg = lib.gmx_rows_quantiles(*args), lib.gmx_last_error()
        assert rc != 0 and b"gmx_rows_quantiles" in msg and names in msg, (msg, names)


BK_R, BK_SEED, BANKS = 3, 4242, [dict(), dict(ess_threshold=0.5), dict(model="tracker")]       # R = 3 filters; the last bank: D = 2


def check_bank(be, specialize, capture=False, model="lgssm", n=64, T=4, **kw):
    """the plain bank's bits in state and log_ml; the last step's quantiles are smc.row_quantiles' and the reference's on state();
    plain lgssm: every step is the reference on that key's BootstrapSweep history, two captured replays give the eager bits"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    init, step = K._models(model)
    keys, ys, lv = G.split(G.key(BK_SEED), BK_R), K._data(T), [round(p * ONE) for p in PROBS]
    plain, bank = (smc.BootstrapBank(init, step, n, BK_R, T, specialize=specialize, **kw, **m).prepare(keys, ys)
                   for m in (dict(), dict(quantiles=PROBS)))
    plain.launch(), bank.launch()
    (x, lw, anc), (px, plw, panc) = K._np_state(bank.state()), K._np_state(plain.state())
    assert H.same_bits(x, px) and H.same_bits(lw, plw) and np.array_equal(anc, panc) and np.array_equal(bank.log_ml(), plain.log_ml())
    for err, name, f in ((ValueError, "quantiles=", plain.filter_quantiles),
                         (NotImplementedError, "ConditionalBank: quantiles=", lambda: smc.ConditionalBank(init, step, n, BK_R, T, quantiles=PROBS)),
                         (NotImplementedError, "gmx_rows_quantiles", lambda: smc.BootstrapBank(init, step, 1025, BK_R, T, quantiles=PROBS))):
        with pytest.raises(err, match=name):
            f()
    x, got = x[None] if x.ndim == 2 else np.ascontiguousarray(np.moveaxis(x, 2, 0)), bank.filter_quantiles()
    D = x.shape[0]
    assert got.shape == ((T, BK_R, 3) if D == 1 else (T, BK_R, D, 3)) and got.dtype == torch.float32
    eager = got.numpy().reshape(T, BK_R, D, 3).view(np.uint32).copy()
    assert np.array_equal(eager[T - 1], reference(lw, x, lv))           # (ess_threshold=: state()'s lw is the sum the kernel saw)
    again = smc.row_quantiles(bank.state()[1], bank.state()[0], PROBS)
    assert np.array_equal(again.cpu().numpy().reshape(BK_R, D, 3).view(np.uint32), eager[T - 1])
    if model != "lgssm" or kw:
        return
    for r in range(BK_R):
        sw = smc.BootstrapSweep(init, step, n, T, specialize=specialize, history=True).prepare(keys[r], ys)
        sw.launch()
        hx, hlw = sw.history().x.cpu().numpy(), sw.history().log_weights.cpu().numpy()
        assert all(np.array_equal(eager[t, r], reference(hlw[t][None], hx[t][None, None], lv)[0]) for t in range(T)), r
    if capture:
        bank.qnt.zero_()
        bank.capture()
        bank.launch(), bank.launch()     # two replays
        assert np.array_equal(bank.qnt.cpu().numpy().view(np.uint32), eager)
