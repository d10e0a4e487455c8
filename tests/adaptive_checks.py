"""Shared drivers of tests/test_adaptive_cpu.py (the C-ABI's CPU mirror) and tests/test_adaptive_gpu.py (the HIP library):
gmx_resample_rows_ess against its definition composed from existing pieces — the oracle's per-row path on float32(lw +
carry), the fixed-point weights as the differences of the oracle's one-tile CDF, the ESS predicate in Python integers —
with every integer and every bit compared for equality; the integer ESS against float64; and
smc.BootstrapBank(ess_threshold=) against the bank without the argument, against a bank whose resampling step is that
composition, and against the Kalman evidence."""
from __future__ import annotations

import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import torch

from oracle import genjax_oracle as O
from tests import backward_checks as B
from tests import bank_checks as K
from tests import history_checks as H

ESS_SIZES = [1, 5, 64, 255, 256, 257, 512, 513, 1023, 1024]      # the packing changes at 256 and 512
ESS_COUNTS = [1, 7, 130]               # at n = 100: idle groups, a partial last workgroup
KINDS = list(K.ROW_KINDS)
LD_PAD = 3
FLAG_POISON = -7

# What the integer ESS V1^2 / V2 of the truncated fixed-point weights may differ from exp(2 lse(x) - lse(2 x)) in float64
# by, relatively: 4 x the largest relative error MEASURED on the CPU mirror over the rows of SHAPE_CASES plus the sized
# cases (every row with mass; the integer side is exact rational arithmetic on the integers the mirror's decisions were
# held to, bit for bit, by the tests above it).  Measured: 3.19e-8 over 37 rows (check_ess_against_float64 prints it); the
# float32 exp of each weight (about 6e-8 relative, averaging out over a row) dominates, the truncation to 30 bits is
# below 2^-29 on the weights that matter.
ESS_REL_MEASURED = 3.2e-8
ESS_REL_BOUND = 4.0 * ESS_REL_MEASURED


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def same_bits_or_nan(got, want):
    """bit equality, except that where `want` is NaN any NaN will do (an addition's NaN payload is the hardware's)"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and H.same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want))


# --- the entry point -----------------------------------------------------------------------------------------------------------
def resample_rows_ess(be, kind, rows, carry, keys, ess_q8, stride=0, pad=LD_PAD):
    """rows, carry: [R, n] float32; both matrices padded and the padding poisoned; everything the call writes starts poisoned"""
    dev = be.device
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    R, n = rows.shape
    ld = n + pad
    host = np.full((R, ld), B.POISON, dtype=np.float32)
    host[:, :n] = rows
    chost = np.full((R, ld), -B.POISON, dtype=np.float32)
    chost[:, :n] = carry
    lw, cy = torch.from_numpy(host.copy()).to(dev), torch.from_numpy(chost.copy()).to(dev)
    k_d = torch.from_numpy(_i32(keys).reshape(R, 2)).to(dev)
    anc = torch.full((R, n), -7, dtype=torch.int32, device=dev)
    mx = torch.full((R,), 7.0, dtype=torch.float32, device=dev)
    total = torch.full((R,), -7, dtype=torch.int64, device=dev)
    flags = torch.full((R,), FLAG_POISON, dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_resample_rows_ess_workspace(kind, R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_resample_rows_ess(kind, be.ptr(k_d), be.ptr(lw), be.ptr(cy), R, n, ld, stride, int(ess_q8), be.ptr(mx),
                                    be.ptr(total), be.ptr(flags), be.ptr(anc), be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    lw_h, cy_h = lw.cpu().numpy(), cy.cpu().numpy()
    assert H.same_bits(lw_h[:, n:], host[:, n:]) and H.same_bits(cy_h[:, n:], chost[:, n:]), "the padding was written"
    return dict(anc=anc.cpu().numpy(), mx=mx.cpu().numpy(), tot=[int(v) & 0xFFFFFFFFFFFFFFFF for v in total.cpu().tolist()],
                status=int(status.item()), flags=flags.cpu().numpy(), lw=lw_h[:, :n], carry=cy_h[:, :n])


# --- its definition, from existing pieces ------------------------------------------------------------------------------------------
def summed(rows, carry):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(rows, np.float32) + np.asarray(carry, np.float32)).astype(np.float32)


def row_sums(x):
    """(V1, V2) of one row, Python integers: v_i = w_i >> (shift - 30), w_i the differences of the oracle's one-tile CDF"""
    x = np.asarray(x, np.float32)
    assert x.size <= O.CDF_TILE
    cdf, _total, _M, shift = O.weight_cdf(x)
    c = [0] + [int(v) for v in cdf]
    v = [(c[i + 1] - c[i]) >> (shift - 30) for i in range(x.size)]
    return sum(v), sum(a * a for a in v)


def decides(V1, V2, total, ess_q8, n):
    """the definition's predicate, in Python integers"""
    return total != 0 and (ess_q8 > 256 * n or V1 * V1 * 256 < ess_q8 * V2)


def oracle_parts(kind, x, keys):
    """per row of x: (candidate ancestors, total, max, V1, V2) — what does not depend on the threshold"""
    out = []
    for r in range(x.shape[0]):
        a, total, M = K.oracle_row(kind, x[r], keys[r])
        out.append((a, total, M) + row_sums(x[r]))
    return out


def definition(parts, x, ess_q8, stride):
    R, n = x.shape
    anc = np.empty((R, n), np.int32)
    carry = np.zeros((R, n), np.float32)
    flags = np.zeros((R,), np.int32)
    for r, (a, total, _M, V1, V2) in enumerate(parts):
        go = decides(V1, V2, total, ess_q8, n)
        flags[r] = int(go)
        anc[r] = (a if go else np.arange(n, dtype=np.int32)) + r * stride
        if not go:
            carry[r] = x[r]
    return dict(anc=anc, mx=np.array([p[2] for p in parts], np.float32), tot=[p[1] for p in parts],
                status=sum(1 for p in parts if p[1] == 0), flags=flags, lw=x, carry=carry)


def assert_equal(got, want, what):
    assert np.array_equal(got["flags"], want["flags"]), (what, "flags", got["flags"].tolist(), want["flags"].tolist())
    assert np.array_equal(got["anc"], want["anc"]), (what, "ancestors", np.argwhere(got["anc"] != want["anc"])[:5].tolist())
    assert got["tot"] == want["tot"], (what, "total")
    assert H.same_bits(got["mx"], want["mx"]), (what, "max", got["mx"], want["mx"])
    assert got["status"] == want["status"], (what, "status", got["status"], want["status"])
    assert same_bits_or_nan(got["lw"], want["lw"]), (what, "lw written back")
    assert same_bits_or_nan(got["carry"], want["carry"]), (what, "carry")


def ess_of(parts):
    """the integer ESS of every row with mass, as exact fractions"""
    return [Fraction(p[3] * p[3], p[4]) for p in parts if p[1] != 0 and p[4] != 0]


def mid_threshold(parts):
    """an ess_q8 between the two middle ESS values of the rows with mass: both outcomes occur (asserted by the callers)"""
    e = sorted(ess_of(parts))
    assert len(e) >= 2 and e[0] < e[-1], "the case holds rows of one ESS only"
    j = min((i for i in range(1, len(e)) if e[i - 1] < e[i]), key=lambda i: abs(i - len(e) // 2))
    return int(math.floor((e[j - 1] + e[j]) / 2 * 256)) + 1


def both_outcomes(flags):
    return bool(np.any(flags == 1) and np.any(flags == 0))


# --- the cases -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sized_case(n, R=6):
    """(rows, carry, keys) of a size (never modified): half the rows dense normal draws, half with at most 3 finite columns;
    the carry non-zero on every other row"""
    rng = np.random.default_rng(77 * n + R)
    rows = rng.normal(size=(R, n)).astype(np.float32)
    for r in range(R // 2, R):
        keep = rng.choice(n, size=min(n, 1 + r % 3), replace=False)
        sparse = np.full((n,), -np.inf, np.float32)
        sparse[keep] = rows[r, keep]
        rows[r] = sparse
    carry = (0.5 * rng.normal(size=(R, n))).astype(np.float32)
    carry[::2] = 0.0
    rows.setflags(write=False)
    carry.setflags(write=False)
    return rows, carry, O.split(O.key(7), R)


@functools.lru_cache(maxsize=None)
def count_case(R):
    """R rows of 100 columns, each at its own spread (the ESS of a row falls with it), carry on every third row"""
    rng = np.random.default_rng(100)
    rows = (rng.normal(size=(max(ESS_COUNTS), 100)) * rng.uniform(0.2, 3.0, size=(max(ESS_COUNTS), 1))).astype(np.float32)[:R]
    carry = (0.3 * rng.normal(size=(max(ESS_COUNTS), 100))).astype(np.float32)[:R].copy()
    carry[::3] = 0.0
    rows.setflags(write=False)
    carry.setflags(write=False)
    return rows, carry, O.split(O.key(7), max(ESS_COUNTS))[:R]


# backward_checks.pick_case's row shapes, through a window of at most one tile that keeps what the shape is about
SHAPE_CASES = {"normal5": ("normal5", 0, 5), "normal1024": ("normal1024", 0, 1024), "gap": ("gap", 512, 1024),
               "hole": ("hole", 0, 1000), "mixed": ("mixed", 976, 1024)}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    src, lo, n = SHAPE_CASES[name]
    rows = np.ascontiguousarray(B.pick_case(src)[:, lo:lo + n])
    rng = np.random.default_rng(len(name))
    carry = (0.25 * rng.normal(size=rows.shape)).astype(np.float32)
    carry[1] = 0.0
    rows.setflags(write=False)
    carry.setflags(write=False)
    return rows, carry, B.pick_keys(rows.shape[0])


@functools.lru_cache(maxsize=None)
def _parts(which, arg, kind_name):
    rows, carry, keys = {"sized": sized_case, "count": count_case, "shape": shape_case}[which](arg)
    x = summed(rows, carry)
    x.setflags(write=False)
    return x, oracle_parts(K.ROW_KINDS[kind_name], x, keys)


def check_case(be, which, arg, kind_name, need_both=True, strides=(0, None)):
    """the entry point == its definition at a threshold between the rows' ESS values, index_stride 0 and n"""
    rows, carry, keys = {"sized": sized_case, "count": count_case, "shape": shape_case}[which](arg)
    R, n = rows.shape
    x, parts = _parts(which, arg, kind_name)
    qs = [mid_threshold(parts)] if need_both else [256 * n, 256 * n + 1]
    for q in qs:
        for s in strides:
            s = n if s is None else s
            want = definition(parts, x, q, s)
            if need_both:
                assert both_outcomes(want["flags"]), (which, arg, q, want["flags"].tolist())
            got = resample_rows_ess(be, K.ROW_KINDS[kind_name], rows, carry, keys, q, stride=s)
            assert_equal(got, want, (which, arg, kind_name, q, s))


def check_boundary(be, n, k, kind_name):
    """k equal finite weights, the rest -inf: the integer ESS is exactly k — 256 k does not resample, 256 k + 1 does"""
    rng = np.random.default_rng(n + k)
    rows = np.full((2, n), -np.inf, np.float32)
    carry = np.zeros((2, n), np.float32)
    for r in range(2):
        cols = rng.choice(n, size=k, replace=False)
        rows[r, cols] = np.float32(-1.25 - r)
        carry[r, cols] = np.float32(0.5 * r)
    keys = O.split(O.key(3), 2)
    x = summed(rows, carry)
    parts = oracle_parts(K.ROW_KINDS[kind_name], x, keys)
    assert ess_of(parts) == [Fraction(k), Fraction(k)]
    for q, flag in ((256 * k, 0), (256 * k + 1, 1)):
        got = resample_rows_ess(be, K.ROW_KINDS[kind_name], rows, carry, keys, q, stride=n)
        assert got["flags"].tolist() == [flag, flag], (n, k, q, got["flags"].tolist())
        assert_equal(got, definition(parts, x, q, n), ("boundary", n, k, q))


def check_extremes(be, n, kind_name):
    """ess_q8 = 0 resamples no row (identity ancestors, carry = lw + carry); 256 n + 1 every row: gmx_resample_rows'
    ancestors on the sum through the same library, and a zero carry"""
    rows, carry, keys = sized_case(n)
    R = rows.shape[0]
    x, parts = _parts("sized", n, kind_name)
    kind = K.ROW_KINDS[kind_name]
    got = resample_rows_ess(be, kind, rows, carry, keys, 0, stride=n)
    assert_equal(got, definition(parts, x, 0, n), ("never", n))
    assert not got["flags"].any()
    assert np.array_equal(got["anc"], np.arange(R * n, dtype=np.int32).reshape(R, n))
    assert same_bits_or_nan(got["carry"], x)
    got = resample_rows_ess(be, kind, rows, carry, keys, 256 * n + 1, stride=n)
    assert_equal(got, definition(parts, x, 256 * n + 1, n), ("always", n))
    assert got["flags"].all() and H.same_bits(got["carry"], np.zeros((R, n), np.float32))
    anc, mx, tot, status = K.resample_rows(be, kind, x, keys, pad=LD_PAD, stride=n)
    assert np.array_equal(got["anc"], anc) and H.same_bits(got["mx"], mx) and got["tot"] == tot and got["status"] == status


def check_no_mass(be, n, kind_name):
    """row 2 without mass among normal ones: counted once, not resampled whatever the threshold, its neighbours exact"""
    rows, carry, keys = sized_case(n)
    rows = rows.copy()
    rows[2] = -np.inf
    x = summed(rows, carry)
    parts = oracle_parts(K.ROW_KINDS[kind_name], x, keys)
    assert parts[2][1] == 0
    for q in (mid_threshold(parts), 256 * n + 1):
        got = resample_rows_ess(be, K.ROW_KINDS[kind_name], rows, carry, keys, q, stride=n)
        assert_equal(got, definition(parts, x, q, n), ("no mass", n, q))
        assert got["status"] == 1 and got["flags"][2] == 0
        assert np.array_equal(got["anc"][2], 2 * n + np.arange(n, dtype=np.int32))


def check_special_carry(be, n, kind_name):
    """-inf and NaN entries in the carry (and -inf weights under a NaN carry): the definition's answer"""
    rows, carry, keys = sized_case(n)
    carry = carry.copy()
    carry[0, ::3] = -np.inf
    carry[1, 1::4] = np.nan
    carry[3, :] = np.nan                # a sparse row: NaN over -inf and over its finite columns — no mass left
    carry[4, 0] = -np.inf
    x = summed(rows, carry)
    parts = oracle_parts(K.ROW_KINDS[kind_name], x, keys)
    assert parts[3][1] == 0
    for q in (mid_threshold(parts), 256 * n + 1):
        got = resample_rows_ess(be, K.ROW_KINDS[kind_name], rows, carry, keys, q, stride=n)
        assert_equal(got, definition(parts, x, q, n), ("special carry", n, q))
        assert got["flags"][3] == 0


# --- the integer ESS against float64 ------------------------------------------------------------------------------------------------
def float_ess(x):
    """exp(2 lse(x) - lse(2 x)) in float64 over the entries that carry weight (NaN carries none)"""
    x = np.asarray(x, np.float64)
    x = x[~np.isnan(x)]
    m = x.max()
    return float(np.exp(2.0 * (m + np.log(np.sum(np.exp(x - m)))) - (2.0 * m + np.log(np.sum(np.exp(2.0 * (x - m)))))))


def ess_rows():
    """every row with mass of the shape cases and of three sized cases: (x [n], V1, V2)"""
    out = []
    for which, args in (("shape", list(SHAPE_CASES)), ("sized", [64, 257, 1024])):
        for arg in args:
            x, parts = _parts(which, arg, "multinomial")
            out += [(x[r], p[3], p[4]) for r, p in enumerate(parts) if p[1] != 0]
    return out


def ess_relative_errors():
    return [abs(float(Fraction(V1 * V1, V2)) / float_ess(x) - 1.0) for x, V1, V2 in ess_rows()]


def check_ess_against_float64(be):
    """the rows' integer ESS is within ESS_REL_BOUND of float64, as exact fractions — and the entry point's own decision
    says so: at ess_q8 = floor(256 E (1 - b)) a row is NOT resampled (ESS_int >= E (1 - b) >= ess_q8 / 256), at
    ceil(256 E (1 + b)) + 1 it IS (ESS_int <= E (1 + b) < ess_q8 / 256), E the float64 value and b the bound"""
    errs = ess_relative_errors()
    print("integer ESS against float64: largest relative error", max(errs), "over", len(errs), "rows; bound", ESS_REL_BOUND)
    assert max(errs) <= ESS_REL_BOUND, max(errs)
    key = O.split(O.key(5), 1)
    for x, _V1, _V2 in ess_rows():
        n = x.size
        if n < 2:
            continue
        E = float_ess(x)
        lo, hi = int(math.floor(256.0 * E * (1.0 - ESS_REL_BOUND))), int(math.ceil(256.0 * E * (1.0 + ESS_REL_BOUND))) + 1
        for q, flag in ((lo, 0), (min(hi, 256 * n + 1), 1)):
            got = resample_rows_ess(be, O.SYSTEMATIC, x.reshape(1, n), np.zeros((1, n), np.float32), key, q)
            assert got["flags"].tolist() == [flag], (n, E, q, flag)


# --- refusals ------------------------------------------------------------------------------------------------------------------
def ess_refusal_calls():
    """argument tuples gmx_resample_rows_ess must refuse before any launch, with what the message has to name"""
    N, i64, i32, u32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    buf = (ctypes.c_int64 * 8)()
    P = ctypes.cast(buf, ctypes.c_void_p)

    def call(kind=0, keys=P, lw=P, carry=P, rows=2, n=10, ld=10, stride=0, q=128, mx=P, total=P, flags=P, anc=P, status=P, ws=P):
        return (i32(kind), keys, lw, carry, i64(rows), i64(n), i64(ld), i64(stride), u32(q), mx, total, flags, anc, status, ws, N)
    calls = [(call(**{a: N}), b"null") for a in ("keys", "lw", "carry", "mx", "total", "flags", "anc", "status", "ws")]
    calls += [(call(n=0), b"n = 0 is outside [1, 1024]"), (call(n=1025, ld=1025), b"n = 1025 is outside [1, 1024]"),
              (call(n=1025, ld=1025), b"one tile"), (call(n=2 ** 21 + 1, ld=2 ** 21 + 1), b"outside [1, 1024]"),
              (call(kind=O.MULTINOMIAL_TILED), b"GMX_RESAMPLE_MULTINOMIAL_TILED"),
              (call(kind=O.MULTINOMIAL_SORTED), b"GMX_RESAMPLE_MULTINOMIAL_SORTED"),
              (call(kind=O.MULTINOMIAL_TILED, n=2000, ld=2000), b"GMX_RESAMPLE_MULTINOMIAL_TILED"), (call(kind=7), b"kind"),
              (call(ld=9), b"ld = 9"), (call(rows=0), b"rows = 0"), (call(rows=2 ** 31), b"rows = "),
              (call(rows=2 ** 21, n=1024, ld=1024, stride=1024), b"index_stride"), (call(stride=-1), b"index_stride")]
    return calls, buf


def check_refusals_of(lib):
    """lib: a ctypes library (the HIP library without a GPU, or the mirror)"""
    lib.gmx_last_error.restype = ctypes.c_char_p
    calls, _keep = ess_refusal_calls()
    for args, names in calls:
        assert lib.gmx_resample_rows_ess(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_resample_rows_ess" in msg and names in msg, (msg, names)


def workspace_sizes(lib):
    lib.gmx_resample_rows_ess_workspace.restype = ctypes.c_size_t
    lib.gmx_resample_rows_ess_workspace.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
    return [int(lib.gmx_resample_rows_ess_workspace(k, r, n)) for k in (0, 2) for r, n in ((1, 1), (3, 1024), (0, 5), (5, 1025))]


# --- BootstrapBank(ess_threshold=) ----------------------------------------------------------------------------------------------------
SW_R, SW_T, SW_SEED = 8, 8, 4242
SW_SIZES = [64, 300]
SW_MID = 0.5                            # both outcomes fill >= 10 % of the [T, R] cells at n = 64 and 300 (asserted)
SW_HIGH = 0.95                          # some rows are resampled after every step, some are not (asserted)


def make_bank(n, specialize, ess_threshold="plain", kind="systematic", cls=None):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapBank
    init, step = workloads.make_lgssm(G)
    kw = {} if isinstance(ess_threshold, str) else dict(ess_threshold=ess_threshold)
    bank = (cls or BootstrapBank)(init, step, n, SW_R, SW_T, resample=kind, specialize=specialize, **kw)
    return bank.prepare(G.split(G.key(SW_SEED), SW_R), K._data(SW_T))


def composed_bank_class():
    """BootstrapBank(ess_threshold=) whose resampling step is the definition composed call by call: the float32 add, the
    existing gmx_resample_rows, then the predicate in Python integers on host copies and the gating with torch ops"""
    from genjax_amd.inference.smc import BootstrapBank, resample_rows

    class ComposedBank(BootstrapBank):
        def _resample(self, t):
            R, n = self.R, self.n
            lw, carry = self.lw.reshape(R, n), self.carry.reshape(R, n)
            lw.add_(carry)
            resample_rows(self.kind, self.step_keys[t][1], lw, index_stride=n,
                          out=(self.anc, self.totals[t], self.maxs[t], self.status), workspace=self.ws)
            x = lw.cpu().numpy()
            totals = [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.totals[t].cpu().tolist()]
            go = torch.tensor([decides(*row_sums(x[r]), totals[r], self.ess_q8, n) for r in range(R)], device=lw.device)
            ident = torch.arange(R * n, dtype=torch.int32, device=lw.device).reshape(R, n)
            self.anc.copy_(torch.where(go[:, None], self.anc, ident))
            carry.copy_(torch.where(go[:, None], torch.zeros_like(lw), lw))
            self.flags[t].copy_(go.to(torch.int32))
    return ComposedBank


def _snapshot(bank):
    x, lw, anc = K._np_state(bank.state())
    out = dict(x=x, lw=lw, anc=anc, log_ml=bank.log_ml(), maxs=bank.maxs.cpu().numpy(), totals=bank.totals.cpu().numpy())
    if bank.ess_q8 is not None:
        out["flags"] = bank.resampled().numpy()
    return out


def assert_same_sweep(a, b, what, rows=None):
    sel = slice(None) if rows is None else rows
    assert H.same_bits(a["x"][sel], b["x"][sel]), (what, "x")
    assert H.same_bits(a["lw"][sel], b["lw"][sel]), (what, "lw")
    assert np.array_equal(a["anc"][sel], b["anc"][sel]), (what, "ancestors")
    assert np.array_equal(a["log_ml"][sel], b["log_ml"][sel]), (what, "log_ml", a["log_ml"], b["log_ml"])
    if rows is None and "flags" in a and "flags" in b:
        assert np.array_equal(a["flags"], b["flags"]), (what, "flags")


def check_always_is_the_plain_bank(be, n, specialize):
    """ess_threshold=inf (and any value above 1): the bank without the argument, bit for bit"""
    plain = make_bank(n, specialize)
    plain.launch()
    want = _snapshot(plain)
    for tau in (math.inf, 1.5):
        bank = make_bank(n, specialize, tau)
        assert bank.ess_q8 == 256 * n + 1
        bank.launch()
        got = _snapshot(bank)
        assert got["flags"].all() and got["flags"].shape == (SW_T, SW_R) and got["flags"].dtype == np.bool_
        assert_same_sweep(got, want, ("always", n, tau))
        assert H.same_bits(got["maxs"], want["maxs"]) and np.array_equal(got["totals"], want["totals"])
        assert int(bank.status.item()) == 0 and not bank.carry.any()


@functools.lru_cache(maxsize=None)
def composed_sweep(device_type, n, specialize):
    """the composed reference at the middle threshold, once per shape (never modified)"""
    bank = make_bank(n, specialize, SW_MID, cls=composed_bank_class())
    bank.launch()
    return _snapshot(bank)


def check_mid_threshold(be, n, specialize, capture=False):
    """the fused step == the composed one at a threshold where both outcomes fill >= 10 % of the cells; the rows that were
    resampled at every step are the plain bank's"""
    want = composed_sweep(be.device.type, n, specialize)
    frac = float(want["flags"].mean())
    print("mid threshold: resampled fraction of the [T, R] cells", frac, "n", n)
    assert 0.1 <= frac <= 0.9, frac
    bank = make_bank(n, specialize, SW_MID)
    assert bank.ess_q8 == int(math.ceil(SW_MID * n * 256))
    if capture:
        bank.capture()
        assert bank.graph is not None
        bank.launch()                    # two replays
    bank.launch()
    got = _snapshot(bank)
    assert_same_sweep(got, want, ("mid", n, capture))


def check_rows_resampled_at_every_step(be, n, specialize):
    """at a high threshold some rows are resampled after every step and some are not (asserted): the former are the plain
    bank's rows, bit for bit — a row's decisions touch no other row"""
    bank = make_bank(n, specialize, SW_HIGH)
    bank.launch()
    got = _snapshot(bank)
    every = np.nonzero(got["flags"].all(axis=0))[0]
    print("rows resampled at every step:", every.tolist(), "of", SW_R)
    assert 0 < every.size < SW_R, got["flags"].astype(int).tolist()
    plain = make_bank(n, specialize)
    plain.launch()
    assert_same_sweep(got, _snapshot(plain), ("every step", n), rows=every)


def check_never(be, n, specialize):
    """ess_threshold=0: no flag, identity ancestors, log_ml the single term of step T - 1"""
    from genjax_amd.inference.smc import evidence_terms
    bank = make_bank(n, specialize, 0.0)
    assert bank.ess_q8 == 0
    bank.launch()
    got = _snapshot(bank)
    assert not got["flags"].any()
    assert np.array_equal(got["anc"], np.broadcast_to(np.arange(n, dtype=np.int32), (SW_R, n)))
    terms = evidence_terms(got["maxs"], got["totals"], bank.shift, n)
    assert np.array_equal(got["log_ml"], np.array([float(np.sum(terms[SW_T - 1:, r])) for r in range(SW_R)]))
    assert np.all(np.isfinite(got["log_ml"]))


def check_api_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapBank, ConditionalBank
    init, step = workloads.make_lgssm(G)
    for bad in (-0.1, math.nan, -math.inf):
        with pytest.raises(ValueError, match="ess_threshold"):
            BootstrapBank(init, step, 64, 3, 4, ess_threshold=bad)
    with pytest.raises(NotImplementedError, match="1024"):
        BootstrapBank(init, step, 1025, 3, 4, ess_threshold=0.5)
    BootstrapBank(init, step, 1025, 3, 4)
    with pytest.raises(NotImplementedError, match="ess_threshold"):
        ConditionalBank(init, step, 64, 3, 4, ess_threshold=0.5)
    assert BootstrapBank(init, step, 100, 3, 4, ess_threshold=0.5).ess_q8 == 12800
    assert BootstrapBank(init, step, 100, 3, 4, ess_threshold=1.0).ess_q8 == 25600
    assert BootstrapBank(init, step, 3, 3, 4, ess_threshold=1.0 / 3.0).ess_q8 == 256
    with pytest.raises(ValueError, match="ess_threshold"):
        make_bank(64, False).resampled()


# --- the law: E[Z^] = Z under adaptive resampling -----------------------------------------------------------------------------------
def check_law(be, specialize, tau):
    """bank_checks.check_law's set-up and bound with ess_threshold=tau.  A sweep that forgets the carry, or that counts
    a skipped step's term, misses this by many standard errors."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapBank
    init, step = workloads.make_lgssm(G)
    ys = workloads.lgssm_data(K.LAW_T)
    bank = BootstrapBank(init, step, K.LAW_N, K.LAW_R, K.LAW_T, specialize=specialize, ess_threshold=tau)
    bank.prepare(G.split(G.key(2024), K.LAW_R), torch.from_numpy(ys)).launch()
    log_ml = bank.log_ml()
    flags = bank.resampled().numpy()
    assert log_ml.shape == (K.LAW_R,) and np.all(np.isfinite(log_ml))
    if tau == 0:
        assert not flags.any()
    else:
        assert flags.any() and not flags.all()
    ratio = np.exp(log_ml - workloads.kalman_log_ml(ys))
    mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(K.LAW_R)
    print("law: tau", tau, "resampled fraction", flags.mean(), "mean of Z^/Z over", K.LAW_R, "filters", mean,
          "standard error", se, "z", (mean - 1.0) / se)
    assert abs(mean - 1.0) <= 5.0 * se, (mean, se)
