"""Shared drivers of tests/test_abi_kernels_cpu.py (the C-ABI's CPU mirror) and tests/test_abi_kernels_gpu.py (the HIP
library): the small exported kernels of include/genmi.h — gmx_mh_accept, gmx_select, gmx_random_bits, gmx_reduce_max,
gmx_gather, gmx_logsumexp, gmx_sum_rows, gmx_categorical_rows — called through the raw C-ABI and held to exact
references (numpy on the byte view, the oracle bit for bit) or to float64 within a derived bound.

Every output lives in a buffer with GUARD sentinel elements on each side, checked after the call.  Every index handed
to a kernel is in range and every leaf pointer is aligned to its own element size; only 16-byte alignment is broken on
purpose (gmx_gather's choice between k_gather4 and k_gather)."""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch

from oracle import genjax_oracle as O

GUARD = 64            # sentinel elements on each side of every output
SENTINEL = 0xA5       # the byte they hold (as a float32: -2.9e-16, as an int32: negative)


# --- buffers -----------------------------------------------------------------------------------------------------------------
def dev_bytes(be, host, misalign=0):
    """a copy of `host` (any numpy array, taken as bytes) on the backend's device whose address is `misalign` mod 16"""
    raw = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
    t = torch.empty((raw.size + 32,), dtype=torch.uint8, device=be.device)
    off = (-t.data_ptr()) % 16 + misalign
    v = t[off:off + raw.size]
    v.copy_(torch.from_numpy(raw.copy()))
    assert v.data_ptr() % 16 == misalign % 16
    return v


class Out:
    """n elements of `elem` bytes with GUARD sentinel elements before and after; .t is the payload (a byte tensor)"""

    def __init__(self, be, n, elem, misalign=0):
        assert misalign % math.gcd(elem, 16) == 0                # aligned to its own element size, always
        self.n, self.elem = int(n), int(elem)
        self.all = dev_bytes(be, np.full(((2 * GUARD + self.n) * self.elem,), SENTINEL, np.uint8), misalign)
        self.t = self.all[GUARD * self.elem:(GUARD + self.n) * self.elem]
        assert self.t.data_ptr() % 16 == misalign % 16          # (GUARD * elem is a multiple of 16)

    def read(self, dtype=np.uint8):
        """the payload; asserts both guard bands still hold the sentinel"""
        host = self.all.cpu().numpy()
        lo, hi = GUARD * self.elem, (GUARD + self.n) * self.elem
        assert np.all(host[:lo] == SENTINEL), "the guard band BEFORE the output was written"
        assert np.all(host[hi:] == SENTINEL), "the guard band AFTER the output was written"
        return host[lo:hi].copy().view(dtype)

    def untouched(self):
        return bool(np.all(self.all.cpu().numpy() == SENTINEL))


def ptr_table(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def i32_table(values):
    return (ctypes.c_int32 * len(values))(*values)


def keys_dev(be, keys):
    return dev_bytes(be, np.ascontiguousarray(keys, dtype=np.uint32))


def same_bits(a, b):
    a, b = np.atleast_1d(np.ascontiguousarray(a)), np.atleast_1d(np.ascontiguousarray(b))
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# --- gmx_mh_accept -----------------------------------------------------------------------------------------------------------
MH_SIZES = [1, 255, 256, 257, 100_003]
MH_LAW_N = 100_003
MH_LAW_P = [0.01, 0.3, 0.9]


@functools.lru_cache(maxsize=None)
def mh_keys(n):
    k = O.split(O.key(5), n)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def mh_log_u(n):
    """log(uniform.sample(keys, 0, 1)) with the oracle: the left side of the acceptance test (never modified)"""
    lu = O.log(O.uniform.sample(mh_keys(n), np.float32(0.0), np.float32(1.0)))
    lu.setflags(write=False)
    return lu


def mh_accept(be, keys, log_alpha):
    n = len(log_alpha)
    k_d, la_d = keys_dev(be, keys), dev_bytes(be, np.asarray(log_alpha, np.float32))
    out = Out(be, n, 1)
    rc = be.c.gmx_mh_accept(be.ptr(k_d), be.ptr(la_d), n, be.ptr(out.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return out.read(np.uint8)


def check_mh_accept(be, n):
    """bit for bit against log(uniform) < log_alpha for a random N(0, 2) vector and the constants 0, +inf, -inf, NaN"""
    keys, lu = mh_keys(n), mh_log_u(n)
    rng = np.random.default_rng(100 + n)
    cases = [("normal", rng.normal(0, 2, n).astype(np.float32), None),
             ("zero", np.zeros(n, np.float32), 1), ("+inf", np.full(n, np.inf, np.float32), 1),
             ("-inf", np.full(n, -np.inf, np.float32), 0), ("nan", np.full(n, np.nan, np.float32), 0)]
    for name, la, const in cases:
        with np.errstate(invalid="ignore"):
            want = (lu < la).astype(np.uint8)
        got = mh_accept(be, keys, la)
        assert np.array_equal(got, want), (name, n, np.flatnonzero(got != want)[:5])
        if const is not None:
            assert np.all(got == const), (name, n)


def check_mh_accept_frequency(be):
    """the second reference: with log_alpha = log(p) the acceptance frequency over 100_003 fixed keys lies within 4
    binomial standard deviations of p (the oracle alone: z = 1.33, 0.50, -0.02 for p = 0.01, 0.3, 0.9)"""
    n = MH_LAW_N
    for p in MH_LAW_P:
        got = mh_accept(be, mh_keys(n), np.full(n, np.log(p), np.float32))
        assert set(np.unique(got)) <= {0, 1}
        z = (got.mean() - p) / math.sqrt(p * (1 - p) / n)
        print(f"mh_accept frequency: p = {p}, accepted {int(got.sum())} of {n}, z = {z:.2f}")
        assert abs(z) <= 4.0, (p, z)


# --- gmx_select --------------------------------------------------------------------------------------------------------------
SELECT_SIZES = [1, 255, 257, 100_003]
MIXED_ELEMS = [1, 2, 4, 8, 12]         # 12: an array-of-structs [n, 3] int32 leaf, copy_elem's generic byte loop


def select(be, mask, a_leaves, b_leaves, elems):
    """a_leaves / b_leaves: host byte arrays [n * elem] -> the selected leaves as byte arrays"""
    n = len(mask)
    m_d = dev_bytes(be, mask)
    a_d = [dev_bytes(be, a) for a in a_leaves]
    b_d = [dev_bytes(be, b) for b in b_leaves]
    outs = [Out(be, n, e) for e in elems]
    A, _ka = ptr_table(a_d)
    B, _kb = ptr_table(b_d)
    D, _kd = ptr_table([o.t for o in outs])
    rc = be.c.gmx_select(be.ptr(m_d), A, B, D, i32_table(elems), len(elems), n, be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return [o.read() for o in outs]


def check_select(be, n, elems):
    rng = np.random.default_rng(200 + n + len(elems))
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    a = [rng.integers(0, 256, size=n * e, dtype=np.uint8) for e in elems]
    b = [rng.integers(0, 256, size=n * e, dtype=np.uint8) for e in elems]
    got = select(be, mask, a, b, elems)
    for l, e in enumerate(elems):
        want = np.where((mask != 0)[:, None], a[l].reshape(n, e), b[l].reshape(n, e)).reshape(-1)
        assert np.array_equal(got[l], want), (n, l, e, np.flatnonzero(got[l] != want)[:5])


# --- gmx_random_bits ---------------------------------------------------------------------------------------------------------
BITS_SHAPES = [(1, 1), (1, 257), (3, 1000), (1000, 3), (100_003, 1)]


def check_random_bits(be, n, m):
    keys = O.split(O.key(3), n)
    want = O.bits32(keys[:, None, :], np.arange(m, dtype=np.uint64)[None, :])
    out, k_d = Out(be, n * m, 4), keys_dev(be, keys)
    rc = be.c.gmx_random_bits(be.ptr(k_d), n, m, be.ptr(out.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    got = out.read(np.uint32).reshape(n, m)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# --- gmx_reduce_max ----------------------------------------------------------------------------------------------------------
REDUCE_SIZES = [1, 255, 256, 257, 100_003]


def reduce_max(be, x):
    x = np.asarray(x, np.float32)
    out, x_d = Out(be, 1, 4), dev_bytes(be, x)
    rc = be.c.gmx_reduce_max(be.ptr(x_d), len(x), be.ptr(out.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return out.read(np.float32)[0]


def check_reduce_max(be, n):
    rng = np.random.default_rng(300 + n)
    x = rng.normal(0, 5, n).astype(np.float32)
    assert same_bits(reduce_max(be, x), np.fmax.reduce(x))
    holes = x.copy()                                   # scattered NaN is ignored ...
    holes[rng.random(n) < 0.3] = np.nan
    holes[int(np.argmax(x))] = np.nan                  # ... the maximum's own slot included
    want = np.fmax.reduce(holes)
    got = reduce_max(be, holes)
    if np.isnan(want):                                 # (n = 1: nothing is left)
        assert got == -np.inf
    else:
        assert same_bits(got, want)
    assert reduce_max(be, np.full(n, np.nan, np.float32)) == -np.inf
    assert reduce_max(be, np.full(n, -np.inf, np.float32)) == -np.inf
    one = x.copy()
    one[n // 2] = np.inf
    assert reduce_max(be, one) == np.inf
    # max(-0, +0) = +0 wherever the +0 sits
    for pos in sorted({0, n // 2, n - 1}):
        z = np.full(n, -0.0, np.float32)
        z[pos] = 0.0
        assert same_bits(reduce_max(be, z), np.float32(0.0)), (n, pos)
    assert same_bits(reduce_max(be, np.full(n, -0.0, np.float32)), np.float32(-0.0))


def check_reduce_max_signed_zeros(be):
    for pair in ([-0.0, 0.0], [0.0, -0.0]):
        assert same_bits(reduce_max(be, np.array(pair, np.float32)), np.float32(0.0)), pair


# --- gmx_gather --------------------------------------------------------------------------------------------------------------
GATHER_N_OUT = [1, 2, 3, 4, 5, 7, 1023, 100_001]
ANC_FORMS = ["sorted", "random", "equal", "last"]
GATHER_LEAF_COUNTS = [32, 33, 65]       # GMX_MAX_LEAVES = 32 leaves per launch: one, two and three launches


def gather_sources(n_out):
    """n_src above and below n_out (n_out = 1: above and equal)"""
    return [2 * n_out + 3, max(1, (n_out + 1) // 3)]


def ancestors_of(form, rng, n_src, n_out):
    if form == "sorted":
        return np.sort(rng.integers(0, n_src, size=n_out)).astype(np.int32)
    if form == "random":
        return rng.integers(0, n_src, size=n_out).astype(np.int32)
    if form == "equal":
        return np.full(n_out, int(rng.integers(0, n_src)), np.int32)
    if form == "last":
        return np.full(n_out, n_src - 1, np.int32)
    raise KeyError(form)


def gather(be, src_leaves, elems, anc, dst_shift=None, anc_shift=False):
    """src_leaves: host byte arrays [n_src * elem]; dst_shift[l] = True: leaf l's destination starts one ELEMENT past a
    16-byte boundary; anc_shift: the ancestors are handed over as a[1:] of an aligned array (4 bytes past a boundary).
    Sources are always 16-byte aligned."""
    n_out = len(anc)
    dst_shift = dst_shift or [False] * len(elems)
    if anc_shift:
        a_d = dev_bytes(be, np.concatenate([np.zeros(1, np.int32), anc]))[4:]
        assert a_d.data_ptr() % 16 == 4
    else:
        a_d = dev_bytes(be, anc)
    s_d = [dev_bytes(be, s) for s in src_leaves]
    outs = [Out(be, n_out, e, misalign=(e % 16) if sh else 0) for e, sh in zip(elems, dst_shift)]
    for o, e, sh in zip(outs, elems, dst_shift):
        assert o.t.data_ptr() % math.gcd(e, 16) == 0 and (o.t.data_ptr() % 16 != 0) == bool(sh and e % 16)
    S, _ks = ptr_table(s_d)
    D, _kd = ptr_table([o.t for o in outs])
    rc = be.c.gmx_gather(S, D, i32_table(elems), len(elems), be.ptr(a_d), n_out, be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return [o.read() for o in outs]


def gather_reference(src_leaves, elems, anc):
    return [s.reshape(-1, e)[anc].reshape(-1) for s, e in zip(src_leaves, elems)]


def check_gather_mixed(be, n_out):
    """element sizes 1, 2, 4, 8 and 12 bytes in one table (k_gather: every branch of copy_elem)"""
    rng = np.random.default_rng(400 + n_out)
    for n_src in gather_sources(n_out):
        src = [rng.integers(0, 256, size=n_src * e, dtype=np.uint8) for e in MIXED_ELEMS]
        for form in ANC_FORMS:
            anc = ancestors_of(form, rng, n_src, n_out)
            got = gather(be, src, MIXED_ELEMS, anc)
            for l, want in enumerate(gather_reference(src, MIXED_ELEMS, anc)):
                assert np.array_equal(got[l], want), (n_out, n_src, form, MIXED_ELEMS[l], np.flatnonzero(got[l] != want)[:5])


def check_gather_alignment(be, n_out, leaves=3):
    """an all-4-byte table three ways: (a) everything 16-byte aligned (k_gather4), (b) every destination one element
    past a boundary, (c) the ancestors one element past a boundary (both: k_gather) — the same bytes each time"""
    rng = np.random.default_rng(500 + n_out)
    elems = [4] * leaves
    for n_src in gather_sources(n_out):
        src = [rng.integers(0, 256, size=n_src * 4, dtype=np.uint8) for _ in elems]
        for form in ANC_FORMS:
            anc = ancestors_of(form, rng, n_src, n_out)
            want = gather_reference(src, elems, anc)
            ways = {"aligned": gather(be, src, elems, anc),
                    "dst + 1": gather(be, src, elems, anc, dst_shift=[True] * leaves),
                    "anc + 1": gather(be, src, elems, anc, anc_shift=True)}
            for way, got in ways.items():
                for l in range(leaves):
                    assert np.array_equal(got[l], want[l]), (way, n_out, n_src, form, l, np.flatnonzero(got[l] != want[l])[:5])


def check_gather_many_leaves(be, leaves, n_out):
    """more leaves than one launch holds: chunks of 32, each with its own choice of kernel — all aligned, and with only
    the LAST chunk's destinations one element past a boundary (the first chunks stay on k_gather4)"""
    rng = np.random.default_rng(600 + leaves + n_out)
    elems = [4] * leaves
    n_src = n_out + 5
    src = [rng.integers(0, 256, size=n_src * 4, dtype=np.uint8) for _ in elems]
    anc = ancestors_of("random", rng, n_src, n_out)
    want = gather_reference(src, elems, anc)
    last_chunk = ((leaves - 1) // 32) * 32
    for shift in ([False] * leaves, [l >= last_chunk for l in range(leaves)]):
        got = gather(be, src, elems, anc, dst_shift=shift)
        for l in range(leaves):
            assert np.array_equal(got[l], want[l]), (leaves, n_out, shift[l], l, np.flatnonzero(got[l] != want[l])[:5])


# --- gmx_logsumexp -----------------------------------------------------------------------------------------------------------
LSE_TILE = 4096
LSE_SHAPES = [(31, 4096), (32, 4096), (32, 4097), (31, 4097),        # both sides of the one-wave-per-row dispatch
              (1, 1), (5, 63), (5, 64), (5, 65),
              (2, 4095), (2, 8192), (2, 8193), (1, 4096 * 256 + 1),   # the last: stage 2 loops over 257 tile partials
              (70_000, 3)]                                            # more than 65535 rows, short path
LSE_LONG = 4096 * 256 + 1
LSE_DATA = ["normal5", "wide", "third_neginf", "neginf_tile"]
LSE_RTOL = LSE_ATOL = 2e-6             # tests/test_gpu_parity.py::test_logsumexp: f32 tree sum against float64


def lse_cases():
    """(rows, cols, data): "neginf_tile" (the second 4096-tile entirely -inf) needs a row of at least two tiles"""
    return [(r, c, d) for (r, c) in LSE_SHAPES for d in LSE_DATA if d != "neginf_tile" or c >= 2 * LSE_TILE]


def lse_rows_path(rows, cols):
    """include/genmi.h: one wave per row for many short rows, two stages over tiles of 4096 otherwise"""
    return rows >= 32 and cols <= 4096


def lse_workspace_bytes(rows, cols):
    return 16 if lse_rows_path(rows, cols) else rows * ((cols + LSE_TILE - 1) // LSE_TILE) * 8 + 16


@functools.lru_cache(maxsize=None)
def lse_input(rows, cols, data):
    """float32 [rows, cols], every row with a finite maximum (never modified).  The last column repeats the row's maximum:
    a kernel that loses the ragged end of a row (a last tile of one element, the 257th tile partial) loses a term no
    smaller than any other.  The row of a million columns is handed over in ASCENDING order: in random order a
    sequential float32 sum — the oracle's O.logsumexp, the CPU mirror — drops every term below half an ulp of its
    accumulator and misses the bound 6.8-fold, so that input could not be confirmed against the oracle; sorted, the
    small terms are added first and both stay inside the bound."""
    rng = np.random.default_rng(700 + sum(data.encode()) + rows * 7 + cols)
    if data == "wide":                   # most terms underflow
        x = rng.normal(0, 1, (rows, cols)) * 1e4
    else:
        x = rng.normal(0, 5, (rows, cols))
    x = x.astype(np.float32)
    if cols >= LSE_LONG:
        x = np.sort(x, axis=1)
    x[:, -1] = x.max(axis=1)
    if data == "third_neginf":
        hole = rng.random((rows, cols)) < 1.0 / 3.0
        hole[:, -1] = False
        x[hole] = -np.inf
    if data == "neginf_tile":
        x[:, LSE_TILE:2 * LSE_TILE] = -np.inf
    x.setflags(write=False)
    return x


def lse_float64(x):
    x64 = np.asarray(x, np.float64)
    m = x64.max(axis=-1)
    return np.log(np.sum(np.exp(x64 - m[..., None]), axis=-1)) + m


def logsumexp(be, x, want_max=True):
    x = np.asarray(x, np.float32)
    rows, cols = x.shape
    ws_bytes = int(be.c.gmx_logsumexp_workspace(rows, cols))
    assert ws_bytes == lse_workspace_bytes(rows, cols), (rows, cols, ws_bytes)    # which kernel the library picks
    ws = Out(be, (ws_bytes + 3) // 4, 4)
    out, out_max, x_d = Out(be, rows, 4), Out(be, rows, 4), dev_bytes(be, x)
    rc = be.c.gmx_logsumexp(be.ptr(x_d), rows, cols, be.ptr(out.t), be.ptr(out_max.t) if want_max else None,
                            be.ptr(ws.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    ws.read()                                                                      # (its guard bands)
    if not want_max:
        assert out_max.untouched()
    return out.read(np.float32), out_max.read(np.float32)


def check_logsumexp(be, rows, cols, data):
    x = lse_input(rows, cols, data)
    got, got_max = logsumexp(be, x)
    ref = lse_float64(x)
    err = np.abs(got - ref) / (LSE_ATOL + LSE_RTOL * np.abs(ref))
    print(f"logsumexp {rows} x {cols} {data}: worst error / bound = {err.max():.3f}")
    assert same_bits(got_max, x.max(axis=-1))
    np.testing.assert_allclose(got, ref, rtol=LSE_RTOL, atol=LSE_ATOL)
    alone, _ = logsumexp(be, x, want_max=False)
    assert same_bits(alone, got)


LSE_SPECIAL_SHAPES = [(40, 100), (2, 5000)]            # one wave per row; two stages, two tiles per row
LSE_SPECIAL = {                                         # what jax.scipy.special.logsumexp answers (O.logsumexp restates it)
    "all -inf": "-inf",
    "holds +inf": "+inf",
    "all nan": "nan",
    "one nan": "nan",
    # not in the reference's own tests, but what its max-then-sum gives (np.max propagates NaN) and O.logsumexp states:
    "+inf and nan": "nan",
    "-inf and nan": "nan",
}


def klass(v):
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return "finite"


def lse_special_rows(case, cols, rng):
    """the forms of one case: the special entries in the first columns, in the last ones (the last tile of a long row) —
    each a row of `cols`"""
    base = rng.normal(0, 5, cols).astype(np.float32)
    rows = []
    if case == "all -inf":
        rows.append(np.full(cols, -np.inf, np.float32))
    elif case == "all nan":
        rows.append(np.full(cols, np.nan, np.float32))
    elif case in ("holds +inf", "one nan"):
        v = np.float32(np.inf if case == "holds +inf" else np.nan)
        for pos in (0, cols // 2, cols - 1):
            r = base.copy()
            r[pos] = v
            rows.append(r)
    elif case == "+inf and nan":
        for a, b in ((0, cols - 1), (cols - 1, 0), (1, 2)):
            r = base.copy()
            r[a], r[b] = np.inf, np.nan
            rows.append(r)
    elif case == "-inf and nan":
        for pos in (0, cols - 1):
            r = np.full(cols, -np.inf, np.float32)
            r[pos] = np.nan
            rows.append(r)
    else:
        raise KeyError(case)
    return rows


def check_logsumexp_special(be, case, rows, cols):
    """the special rows among finite ones: each answers with its class, the finite rows around them with their value"""
    rng = np.random.default_rng(800 + sum(case.encode()) + cols)
    x = rng.normal(0, 5, (rows, cols)).astype(np.float32)
    special = lse_special_rows(case, cols, rng)
    where = [0, rows - 1, rows // 2][:len(special)] if rows > 2 else [0]
    want = LSE_SPECIAL[case]
    for k in range(0, len(special), len(where)):                  # (2 rows: one special row per call, beside a finite one)
        y = x.copy()
        used = {}
        for r, row in zip(where, special[k:k + len(where)]):
            y[r] = row
            used[r] = row
        got, _ = logsumexp(be, y)
        with np.errstate(all="ignore"):
            ref = lse_float64(y)
        for r in range(rows):
            if r in used:
                with np.errstate(all="ignore"):
                    oracle = klass(O.logsumexp(used[r])[()])
                assert oracle == want, (case, "the oracle says", oracle)
                assert klass(got[r]) == want, (case, rows, cols, r, got[r])
            else:
                assert klass(got[r]) == "finite"
                np.testing.assert_allclose(got[r], ref[r], rtol=LSE_RTOL, atol=LSE_ATOL)


def check_refusal(be, what, rows, cols):
    """more than 65535 rows on a two-stage path: non-zero, the entry point named, nothing written.  The input is allocated
    at full size (never filled, never read)."""
    x = torch.empty((rows * cols,), dtype=torch.float32, device=be.device)
    out = Out(be, rows, 4)
    if what == "gmx_logsumexp":
        ws = Out(be, (int(be.c.gmx_logsumexp_workspace(rows, cols)) + 3) // 4, 4)
        rc = be.c.gmx_logsumexp(be.ptr(x), rows, cols, be.ptr(out.t), None, be.ptr(ws.t), be.stream())
    else:
        ws = Out(be, (int(be.c.gmx_sum_rows_workspace(rows, cols)) + 3) // 4, 4)
        rc = be.c.gmx_sum_rows(be.ptr(x), rows, cols, be.ptr(out.t), be.ptr(ws.t), be.stream())
    assert rc != 0
    assert what.encode() in be.c.gmx_last_error(), be.c.gmx_last_error()
    assert out.untouched() and ws.untouched()


# --- gmx_sum_rows ------------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(1, 1), (3, 255), (3, 256), (3, 257), (2, 4095), (2, 4096), (2, 4097),
              (1, 4096 * 256 + 1),          # 257 tile partials: thread 0 of stage 2 adds two of them
              (65_535, 2)]


@functools.lru_cache(maxsize=None)
def sum_input(rows, cols):
    """normal * exp(normal * 4), as test_rows_summed_in_element_order: any reordering of the adds changes the bits"""
    rng = np.random.default_rng(900 + rows + cols)
    x = (rng.normal(0, 3, (rows, cols)) * np.exp(rng.normal(0, 4, (rows, cols)))).astype(np.float32)
    x.setflags(write=False)
    return x


def oracle_sum_tree(x):
    """O.plate_sum_tree, a few rows at a time (it pads every row to whole tiles)"""
    step = 2048
    return np.concatenate([O.plate_sum_tree(x[i:i + step]) for i in range(0, x.shape[0], step)])


def sum_rows(be, x):
    rows, cols = x.shape
    ws_bytes = int(be.c.gmx_sum_rows_workspace(rows, cols))
    assert ws_bytes == rows * ((cols + 4095) // 4096) * 4 + 16
    ws, out, x_d = Out(be, (ws_bytes + 3) // 4, 4), Out(be, rows, 4), dev_bytes(be, x)
    rc = be.c.gmx_sum_rows(be.ptr(x_d), rows, cols, be.ptr(out.t), be.ptr(ws.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    ws.read()
    return out.read(np.float32)


def check_sum_rows(be, rows, cols):
    x = sum_input(rows, cols)
    got = sum_rows(be, x)
    assert same_bits(got, oracle_sum_tree(x)), np.flatnonzero(got != oracle_sum_tree(x))[:5]
    # float64: 16 sequential adds per thread and a block tree of 8 levels per tile, then ceil(tiles / 256) sequential adds
    # per thread and 8 levels over the partials — each add rounds by at most 2^-24 of a partial sum of |x|
    tiles = (cols + 4095) // 4096
    x64 = x.astype(np.float64)
    bound = (16 + 8 + math.ceil(tiles / 256) + 8) * 2.0 ** -24 * np.abs(x64).sum(axis=1)
    err = np.abs(got.astype(np.float64) - x64.sum(axis=1))
    print(f"sum_rows {rows} x {cols}: worst error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), np.flatnonzero(err > bound)[:5]
    assert same_bits(sum_rows(be, x), got)                           # the same bits on a second call


# --- gmx_categorical_rows ----------------------------------------------------------------------------------------------------
CAT_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (7, 5000), (100_003, 3)]
CAT_LAW_ROWS = 200_000


def categorical_rows(be, keys, logits):
    logits = np.asarray(logits, np.float32)
    rows, cols = logits.shape
    out, k_d, x_d = Out(be, rows, 4), keys_dev(be, keys), dev_bytes(be, logits)
    rc = be.c.gmx_categorical_rows(be.ptr(k_d), be.ptr(x_d), rows, cols, be.ptr(out.t), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return out.read(np.int32)


def check_categorical(be, rows, cols):
    """bit for bit against O.categorical.sample: plain logits; scattered -inf logits (never returned); rows that are
    all -inf (index 0) among ordinary ones"""
    rng = np.random.default_rng(1000 + rows + cols)
    keys = O.split(O.key(11), rows)
    plain = rng.normal(0, 2, (rows, cols)).astype(np.float32)
    holes = plain.copy()
    holes[rng.random((rows, cols)) < 0.3] = -np.inf
    empty = holes.copy()
    empty[sorted({0, rows // 2, rows - 1})] = -np.inf
    for name, logits in (("plain", plain), ("holes", holes), ("empty rows", empty)):
        want = O.categorical.sample(keys, logits)
        got = categorical_rows(be, keys, logits)
        assert got.min() >= 0 and got.max() < cols
        assert np.array_equal(got, want), (name, rows, cols, np.flatnonzero(got != want)[:5])
        picked = logits[np.arange(rows), got]
        dead = np.all(np.isneginf(logits), axis=1)
        assert np.all(np.isfinite(picked[~dead])), name             # a -inf logit is never drawn ...
        assert np.all(got[dead] == 0), name                          # ... unless the row has nothing else: index 0
    assert np.all(np.all(np.isneginf(empty), axis=1)[[0, rows - 1]])


def check_categorical_law(be):
    """200_000 rows of the same 7 logits, entry 3 -inf, against the float64 softmax: category 3 is never drawn and
    Pearson's chi-square over the other six stays below 25 (about the 99.99 % point at 5 degrees of freedom; the
    oracle alone gives 5.23 with these keys)"""
    logits = np.random.default_rng(0).normal(0, 1.5, 7)
    logits[3] = -np.inf
    p = np.exp(logits - logits.max())
    p /= p.sum()
    keys = O.split(O.key(11), CAT_LAW_ROWS)
    got = categorical_rows(be, keys, np.broadcast_to(logits.astype(np.float32), (CAT_LAW_ROWS, 7)))
    counts = np.bincount(got, minlength=7)
    live = [0, 1, 2, 4, 5, 6]
    chi2 = float(np.sum((counts[live] - CAT_LAW_ROWS * p[live]) ** 2 / (CAT_LAW_ROWS * p[live])))
    print("categorical law: counts", counts.tolist(), "chi-square", round(chi2, 2))
    assert counts.sum() == CAT_LAW_ROWS and counts[3] == 0
    assert chi2 < 25.0, chi2
