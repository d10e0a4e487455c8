"""Shared drivers of tests/test_ancestor_cpu.py (the C-ABI's CPU mirror) and tests/test_ancestor_gpu.py (the HIP library):
gmx_rows_pin and gmx_resample_rows_as against the composition of the entry points the same library already has (integers
and bits compared for equality) and against the oracle's per-row path, smc.ConditionalBank(ancestor_sampling=True) against
the ancestor_sampling=False bank, an oracle replay and BootstrapBank, bit for bit, its law against the exact smoother of
the LGSSM, and how far one iteration moves the start of a trajectory."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from oracle import genjax_oracle as O
from tests import backward_checks as B
from tests import bank_checks as K
from tests import conditional_checks as C
from tests import history_checks as H

# either side of the 1 / 2 / 4-wave packing and of the one-tile boundary; past 1024 the five-launch form
AS_SIZES = [1, 2, 3, 5, 64, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2049, 3000]
AS_COUNTS = [1, 3, 4, 5, 7, 9]          # around the 4 / 2 / 1 rows per workgroup
AS_COUNT_SIZES = [200, 400, 1000, 1500]  # four, two, one row(s) per workgroup; the tiled form
LD_PAD, AS_LD_PAD = 3, 5               # rows that start at any 4-byte boundary, the two matrices differently
NEXT_POISON = np.float32(7.25e29)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def as_case(n, R):
    """(weights [R, n], ancestor logits [R, n], keys [R, 2], ancestor keys [R, 2]) of a size (never modified)"""
    rng = np.random.default_rng(31 * n + R)
    out = (rng.normal(size=(R, n)).astype(np.float32), (2.0 * rng.normal(size=(R, n))).astype(np.float32),
           O.split(O.key(7), R), O.split(O.key(11), R))
    for a in out[:2]:
        a.setflags(write=False)
    return out


# --- gmx_rows_pin ------------------------------------------------------------------------------------------------------------
def rows_pin(be, rows, pin_lw, pin_x, next_x=None, pad=LD_PAD):
    """the matrix (with its padding), the state store and the broadcast store as gmx_rows_pin left them; everything the
    call may not write is poisoned"""
    dev = be.device
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    R, n = rows.shape
    D = int(pin_x.shape[0])
    ld = n + pad
    host = np.full((R, ld), B.POISON, dtype=np.float32)
    host[:, :n] = rows
    lw = torch.from_numpy(host.copy()).to(dev)
    x_ld = R * n + 5
    x0 = np.full((max(D, 1), x_ld), C.X_POISON, dtype=np.float32)
    x = torch.from_numpy(x0.copy()).to(dev)
    next_ld = R * n + 3                  # (row d > 0 of the broadcast store starts off a 16-byte boundary)
    nx0 = np.full((max(D, 1), next_ld), NEXT_POISON, dtype=np.float32)
    nx = torch.from_numpy(nx0.copy()).to(dev)
    p_lw = torch.from_numpy(np.array(pin_lw, dtype=np.float32)).to(dev)
    p_x = torch.from_numpy(np.array(pin_x, dtype=np.float32)).to(dev) if D else None
    n_x = torch.from_numpy(np.array(next_x, dtype=np.float32)).to(dev) if next_x is not None and D else None
    rc = be.c.gmx_rows_pin(be.ptr(lw), R, n, ld, be.ptr(p_lw), be.ptr(p_x), be.ptr(x) if D else None, D, x_ld, n,
                           be.ptr(n_x), be.ptr(nx) if n_x is not None else None, next_ld, be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return dict(lw_t=lw, lw=lw.cpu().numpy(), lw0=host, x=x.cpu().numpy(), x0=x0, next=nx.cpu().numpy(), next0=nx0, ld=ld)


def check_pin_composition(be, n, R, D, stride):
    """gmx_rows_pin + gmx_resample_rows(MULTINOMIAL) + forcing slot n - 1 == gmx_resample_rows_pinned: ancestors, the matrix,
    the store, max, total and status; and the broadcast is exactly next_x over every particle of its row"""
    rows, _, keys, _ = as_case(n, R)
    rng = np.random.default_rng(1000 * D + n + R)
    pin_lw = rng.normal(size=R).astype(np.float32)
    pin_x = rng.normal(size=(D, R)).astype(np.float32)
    next_x = rng.normal(size=(D, R)).astype(np.float32)
    s = n if stride else 0
    want = C.pinned(be, rows, keys, pin_lw, pin_x, pad=LD_PAD, stride=s)
    for nxt in (None, next_x):
        got = rows_pin(be, rows, pin_lw, pin_x, nxt)
        assert H.same_bits(got["lw"], want["lw"]) and H.same_bits(got["x"], want["x"]), (n, R, D)
        ex = got["next0"].copy()
        if nxt is not None:
            for d in range(D):
                ex[d, :R * n] = np.repeat(next_x[d], n)
        assert H.same_bits(got["next"], ex), (n, R, D, np.argwhere(H.bits(got["next"]) != H.bits(ex))[:5].tolist())
    # ... then the unconditional draw on the matrix the call left, the pinned slot forced on the host
    dev = be.device
    k_d = torch.from_numpy(_i32(keys).reshape(R, 2)).to(dev)
    anc = torch.full((R, n), -7, dtype=torch.int32, device=dev)
    mx = torch.full((R,), 7.0, dtype=torch.float32, device=dev)
    total = torch.full((R,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_resample_rows_workspace(O.MULTINOMIAL, R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_resample_rows(O.MULTINOMIAL, be.ptr(k_d), be.ptr(got["lw_t"]), R, n, got["ld"], s, be.ptr(mx), be.ptr(total),
                                be.ptr(anc), be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    a = anc.cpu().numpy()
    a[:, n - 1] = n - 1 + np.arange(R) * s
    assert np.array_equal(a, want["anc"]), (n, R, D)
    assert H.same_bits(mx, want["mx"]) and int(status.item()) == want["status"]
    assert [int(v) & 0xFFFFFFFFFFFFFFFF for v in total.cpu().tolist()] == want["total"]


# --- gmx_resample_rows_as ------------------------------------------------------------------------------------------------------
def resample_rows_as(be, rows, as_rows, keys, as_keys, stride=0, pad=LD_PAD, as_pad=AS_LD_PAD):
    """(ancestors int32 [R, n], max [R], total [R] python ints, status [2]); both matrices padded and poisoned"""
    dev = be.device
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    R, n = rows.shape
    ld, as_ld = n + pad, n + as_pad
    host = np.full((R, ld), B.POISON, dtype=np.float32)
    host[:, :n] = rows
    ahost = np.full((R, as_ld), B.POISON, dtype=np.float32)
    ahost[:, :n] = as_rows
    lw, alw = torch.from_numpy(host).to(dev), torch.from_numpy(ahost).to(dev)
    k_d = torch.from_numpy(_i32(keys).reshape(R, 2)).to(dev)
    ak_d = torch.from_numpy(_i32(as_keys).reshape(R, 2)).to(dev)
    anc = torch.full((R, n), -7, dtype=torch.int32, device=dev)
    mx = torch.full((R,), 7.0, dtype=torch.float32, device=dev)
    total = torch.full((R,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros((2,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_resample_rows_as_workspace(R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_resample_rows_as(be.ptr(k_d), be.ptr(lw), R, n, ld, stride, be.ptr(ak_d), be.ptr(alw), as_ld, be.ptr(mx),
                                   be.ptr(total), be.ptr(anc), be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    assert H.same_bits(lw, host) and H.same_bits(alw, ahost)            # (both matrices are only read)
    tot = [int(v) & 0xFFFFFFFFFFFFFFFF for v in total.cpu().tolist()]
    return anc.cpu().numpy(), mx.cpu().numpy(), tot, status.cpu().tolist()


def definition(be, rows, as_rows, keys, as_keys, stride):
    """the three steps of gmx_resample_rows_as' definition through the library's own gmx_resample_rows and gmx_pick_rows"""
    R, n = rows.shape
    anc, mx, tot, st0 = K.resample_rows(be, O.MULTINOMIAL, rows, keys, pad=LD_PAD, stride=stride)
    tmp, st1 = B.pick_rows(be, as_rows, as_keys, pad=AS_LD_PAD)
    anc = anc.copy()
    anc[:, n - 1] = tmp + np.arange(R, dtype=np.int32) * stride
    return anc, mx, tot, [st0, st1]


def assert_as_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5].tolist())
    assert H.same_bits(got[1], want[1]), (what, "max")
    assert got[2] == want[2], (what, "total")
    assert list(got[3]) == list(want[3]), (what, "status", got[3], want[3])


def check_as_case(be, n, R, oracle=True):
    """gmx_resample_rows_as == its definition, index_stride 0 and n; every row also the oracle's per-row path with slot
    n - 1 replaced by the oracle's one draw from the ancestor logits"""
    rows, as_rows, keys, as_keys = as_case(n, R)
    for s in (0, n):
        got = resample_rows_as(be, rows, as_rows, keys, as_keys, stride=s)
        assert_as_equal(got, definition(be, rows, as_rows, keys, as_keys, s), (n, R, s))
        assert got[3] == [0, 0]
    if oracle:
        for r in range(R):
            a, total, M = K.oracle_row(O.MULTINOMIAL, rows[r], keys[r])
            a = a.copy()
            a[-1] = B.oracle_pick(as_rows[r], as_keys[r])
            assert np.array_equal(got[0][r] - r * n, a), (n, R, r, np.argwhere(got[0][r] - r * n != a)[:5].tolist())
            assert got[2][r] == total and H.same_bits(got[1][r:r + 1], np.array([M], np.float32))


SPECIAL_SIZES = [257, 600, 1000, 1500]


def check_as_specials(be, n):
    """special ancestor logits, each in one row among ordinary neighbours: all -inf (answers n - 1, counted in status word
    1); a single finite column at 0, 63, 64, 255, 256, n - 1 (the answer); all equal; one column 200 above the rest"""
    singles = [0, 63, 64, 255, 256, n - 1]
    R = 6 + len(singles)
    rows, as_rows, keys, as_keys = as_case(n, R)
    as_rows = as_rows.copy()
    as_rows[1] = -np.inf
    for k, col in enumerate(singles):
        as_rows[3 + k] = -np.inf
        as_rows[3 + k, col] = np.float32(0.5 * k - 1.0)
    r_eq, r_hi = 3 + len(singles), 4 + len(singles)
    as_rows[r_eq] = np.float32(-3.25)
    hi_col = n // 3
    as_rows[r_hi, hi_col] = as_rows[r_hi].max() + np.float32(200.0)
    got = resample_rows_as(be, rows, as_rows, keys, as_keys, stride=n)
    want = definition(be, rows, as_rows, keys, as_keys, n)
    assert_as_equal(got, want, (n, "specials"))
    assert got[3] == [0, 1]
    last = got[0][:, n - 1] - np.arange(R) * n
    assert last[1] == n - 1
    assert [int(last[3 + k]) for k in range(len(singles))] == singles
    assert last[r_hi] == hi_col
    for r in (0, 2, r_eq, R - 1):        # the ordinary neighbours and the flat row: the oracle's draw
        assert last[r] == B.oracle_pick(as_rows[r], as_keys[r]), r
    for r in range(R):                   # no other slot knows about the ancestor logits
        assert np.array_equal(got[0][r, :n - 1] - r * n, K.oracle_row(O.MULTINOMIAL, rows[r], keys[r])[0][:n - 1]), r


def check_as_no_weight_mass(be, n):
    """a row whose WEIGHTS carry no mass (word 0) keeps its ancestor draw; a row with neither is counted in both words"""
    R = 4
    rows, as_rows, keys, as_keys = as_case(n, R)
    rows, as_rows = rows.copy(), as_rows.copy()
    rows[1] = -np.inf
    rows[2] = -np.inf
    as_rows[2] = -np.inf
    got = resample_rows_as(be, rows, as_rows, keys, as_keys, stride=n)
    assert_as_equal(got, definition(be, rows, as_rows, keys, as_keys, n), (n, "no mass"))
    assert got[3] == [2, 1]
    assert got[0][1, n - 1] - n == B.oracle_pick(as_rows[1], as_keys[1]) and got[0][2, n - 1] - 2 * n == n - 1


def _refusal_env():
    N, i64, i32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32
    buf = (ctypes.c_int64 * 8)()
    return N, i64, i32, buf, ctypes.cast(buf, ctypes.c_void_p)


def pin_refusal_calls():
    """argument tuples gmx_rows_pin must refuse before any launch, with what the message has to name"""
    N, i64, i32, buf, P = _refusal_env()

    def call(lw=P, rows=2, n=10, ld=10, pin_lw=P, pin_x=P, x=P, D=1, x_ld=20, x_rs=10, next_x=P, nxt=P, next_ld=20):
        return (lw, i64(rows), i64(n), i64(ld), pin_lw, pin_x, x, i32(D), i64(x_ld), i64(x_rs), next_x, nxt, i64(next_ld), N)
    calls = [(call(**{a: N}), b"null") for a in ("lw", "pin_lw")]
    calls += [(call(n=0), b"n = 0"), (call(rows=0), b"rows = 0"), (call(ld=9), b"ld = 9"), (call(D=-1), b"D = -1"),
              (call(D=65534), b"D = 65534"), (call(x=N), b"x_d"), (call(pin_x=N), b"pin_x_d"), (call(x_ld=19), b"x_ld = 19"),
              (call(x_rs=-1), b"x_row_stride"), (call(next_ld=19), b"next_ld = 19"), (call(nxt=N), b"next_d")]
    return calls, buf


def as_refusal_calls():
    """argument tuples gmx_resample_rows_as must refuse before any launch, with what the message has to name"""
    N, i64, i32, buf, P = _refusal_env()

    def call(keys=P, lw=P, rows=2, n=10, ld=10, stride=0, as_keys=P, as_lw=P, as_ld=10, mx=P, total=P, anc=P, status=P, ws=P):
        return (keys, lw, i64(rows), i64(n), i64(ld), i64(stride), as_keys, as_lw, i64(as_ld), mx, total, anc, status, ws, N)
    calls = [(call(**{a: N}), b"null") for a in ("keys", "lw", "as_keys", "as_lw", "mx", "total", "anc", "status", "ws")]
    calls += [(call(n=0), b"n = 0"), (call(n=2 ** 21 + 1, ld=2 ** 21 + 1, as_ld=2 ** 21 + 1), b"n = "), (call(rows=0), b"rows = 0"),
              (call(rows=2 ** 31), b"rows = "), (call(ld=9), b"ld = 9"), (call(as_ld=9), b"as_ld = 9"),
              (call(rows=2 ** 21, n=1024, ld=1024, as_ld=1024, stride=1024), b"index_stride"), (call(stride=-1), b"index_stride")]
    return calls, buf


def check_refusals_of(lib, messages=True):
    """lib: a ctypes library (the HIP library without a GPU, or the mirror)"""
    lib.gmx_last_error.restype = ctypes.c_char_p
    for fn, (calls, _keep) in (("gmx_rows_pin", pin_refusal_calls()), ("gmx_resample_rows_as", as_refusal_calls())):
        for args, names in calls:
            assert getattr(lib, fn)(*args) != 0, (fn, names)
            msg = lib.gmx_last_error()
            if messages:
                assert fn.encode() in msg and names in msg, (msg, names)


WORKSPACE_SHAPES = [(1, 1), (3, 1024), (3, 1025), (9, 3000), (64, 16384), (5, 2 ** 21), (0, 5), (5, 2 ** 21 + 1)]


def workspace_sizes(lib):
    lib.gmx_resample_rows_as_workspace.restype = ctypes.c_size_t
    lib.gmx_resample_rows_as_workspace.argtypes = [ctypes.c_int64, ctypes.c_int64]
    return [int(lib.gmx_resample_rows_as_workspace(r, n)) for r, n in WORKSPACE_SHAPES]


# --- ConditionalBank(ancestor_sampling=True) ---------------------------------------------------------------------------------
AB_R, AB_T = 3, 4
AB_SIZES = [4, 200, 1500]               # a handful of particles; one launch per resampling; the tiled form
MODELS = ["lgssm", "pair"]             # a scalar state; a two-component tuple state


def make_pair(g):
    """history_checks.make_pair without the site the step samples besides its state: a tuple state (a, b)"""
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
        g.normal(a + b, 1.0) @ "y"
        return (a, b)
    return init, step


@functools.lru_cache(maxsize=None)
def _models(name):
    import genjax_amd as G
    return make_pair(G) if name == "pair" else K._models(name)


def make_bank(model, n, specialize, ancestors, R=AB_R, T=AB_T, keys=None, seed=C.CB_SEED):
    import genjax_amd as G
    from genjax_amd.inference.smc import ConditionalBank
    init, step = _models(model)
    kw = dict(state_sites=("a", "b")) if model == "pair" else {}
    cb = ConditionalBank(init, step, n, R, T, specialize=specialize, ancestor_sampling=ancestors, **kw)
    return cb.prepare(G.split(G.key(seed), R) if keys is None else keys, K._data(T))


@functools.lru_cache(maxsize=None)
def some_paths(model, R, T):
    """retained paths that come from nowhere, in draw()'s layout (never modified)"""
    rng = np.random.default_rng(R * 100 + T + 1)
    if model == "pair":
        return tuple(torch.from_numpy((0.5 * rng.normal(size=(R, T))).astype(np.float32)) for _ in range(2))
    return torch.from_numpy((0.5 * rng.normal(size=(R, T))).astype(np.float32))


def check_only_the_pinned_ancestor_moves(be, model, n, specialize):
    """under the same keys, ys and retained paths the recorded particles and weights are those of ancestor_sampling=False,
    and so is every ancestor but slot n - 1 of each chain at t < T - 1"""
    R, T = AB_R, AB_T
    banks = []
    for flag in (False, True):
        cb = make_bank(model, n, specialize, flag)
        cb.set_retained(some_paths(model, R, T))
        cb.launch()
        banks.append(cb)
    plain, anc = banks
    assert H.same_bits(anc.hist_xs, plain.hist_xs) and H.same_bits(anc.hist_lws, plain.hist_lws)
    assert H.same_bits(anc.maxs, plain.maxs) and torch.equal(anc.totals.cpu(), plain.totals.cpu())
    a, p = anc.hist_ancs.cpu().numpy(), plain.hist_ancs.cpu().numpy()
    last = np.arange(R) * n + n - 1
    keep = np.ones(R * n, bool)
    keep[last] = False
    assert np.array_equal(a[:, keep], p[:, keep])
    assert np.array_equal(a[T - 1], p[T - 1])
    assert np.array_equal(p[:, last], np.broadcast_to(last.astype(np.int32), (T, R)))
    local = a[:T - 1, last] - (np.arange(R) * n)[None, :]
    assert np.all((local >= 0) & (local < n)), local
    if n >= 200:
        assert np.any(local != n - 1), local          # (9 draws among >= 200 particles)
    assert anc.status.cpu().tolist() == [0, 0]
    # the ancestor logits of the last conditional step, as the bank left them: lw + a finite density, the pin included
    assert np.all(np.isfinite(anc.as_lw.cpu().numpy()))
    nx = anc.next_x.cpu().numpy().reshape(anc.D, R, n)
    assert H.same_bits(nx, np.broadcast_to(anc.ref_x[T - 1].cpu().numpy()[:, :, None], nx.shape))


def check_oracle_replay(be, specialize, n, R=2, T=4):
    """every step of an ancestor-sampling LGSSM sweep against an oracle loop per chain: conditional_checks.check_oracle_replay
    with slot n - 1's ancestor at t < T - 1 the oracle's one draw, under the step key's third child, from
    lw_t + the weight os_.importance returns under {x: ref_x[t + 1], y: ys[t + 1]} with args (x_t,)"""
    from genjax_amd import workloads
    cb = make_bank("lgssm", n, specialize, True, R=R, T=T)
    cb.set_retained(some_paths("lgssm", R, T))
    cb.launch()
    ref_x, ref_lw = cb.ref_x.cpu().numpy(), cb.ref_lw.cpu().numpy()
    oi, os_ = workloads.make_lgssm(O)
    ys = workloads.lgssm_data(T)
    keys = C.oracle_keys(R)
    any_keys = O.split(O.key(0), n)
    moved = 0
    for r in range(R):
        x = anc = None
        for t in range(T):
            ks = O.split(O.fold_in(keys[r], t), 3)
            obs = O.C.d({"y": np.float32(ys[t])})
            tr, w = oi.importance(O.split(ks[0], n), obs, ()) if t == 0 else os_.importance(O.split(ks[0], n), obs, (x[anc],))
            x, lw = np.array(tr.get_retval(), np.float32), np.array(w, np.float32)
            x[-1], lw[-1] = ref_x[t, 0, r], ref_lw[t, r]
            anc = C.pinned_oracle_row(lw, lw[-1], ks[1])[0]
            if t < T - 1:
                con = O.C.d({"x": np.float32(ref_x[t + 1, 0, r]), "y": np.float32(ys[t + 1])})
                _, wn = os_.importance(any_keys, con, (x,))
                logits = (lw + np.asarray(wn, np.float32)).astype(np.float32)
                anc = anc.copy()
                anc[-1] = B.oracle_pick(logits, ks[2])
                moved += int(anc[-1] != n - 1)
            sl = slice(r * n, (r + 1) * n)
            assert H.same_bits(cb.hist_xs[t, 0, sl], x), ("x", r, t)
            assert H.same_bits(cb.hist_lws[t, sl], lw), ("lw", r, t)
            assert np.array_equal(cb.hist_ancs[t, sl].cpu().numpy() - r * n, anc), ("anc", r, t, anc[-1])
    assert moved > 0


def check_unconditional(be, model, n, specialize):
    """nothing retained: BootstrapBank(resample="multinomial") under the same keys, bit for bit"""
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapBank
    R, T = AB_R, AB_T
    cb = make_bank(model, n, specialize, True)
    cb.launch()
    init, step = _models(model)
    bb = BootstrapBank(init, step, n, R, T, resample="multinomial", specialize=specialize)
    bb.prepare(G.split(G.key(C.CB_SEED), R), K._data(T)).launch()
    for a, b in zip(K._np_state(cb.state()), K._np_state(bb.state())):
        assert H.same_bits(a, b)
    assert np.array_equal(cb.log_ml(), bb.log_ml())
    assert cb.status.cpu().tolist() == [0, 0]


def check_captured(be, model, n):
    """GPU: a captured ancestor-sampling sweep, replayed; then rekey + retain and replayed again — every replay equals an
    eager bank given the same keys and retained path"""
    import genjax_amd as G
    R, T = AB_R, AB_T
    cap = make_bank(model, n, True, True)
    cap.set_retained(some_paths(model, R, T))
    cap.capture()
    assert cap.graph is not None
    cap.launch()

    def eager(keys, paths):
        e = make_bank(model, n, True, True, keys=keys)
        e.set_retained(paths)
        e.launch()
        return e

    def same(a, b):
        assert H.same_bits(a.hist_xs, b.hist_xs) and H.same_bits(a.hist_lws, b.hist_lws) and H.same_bits(a.hist_ancs, b.hist_ancs)
        assert np.array_equal(a.log_ml(), b.log_ml())
        assert a.status.cpu().tolist() == [0, 0]
    same(cap, eager(G.split(G.key(C.CB_SEED), R), some_paths(model, R, T)))
    drawn = cap.draw(G.key(8))
    drawn = tuple(v.clone() for v in drawn) if isinstance(drawn, tuple) else drawn.clone()
    keys2 = G.split(G.key(123), R)
    cap.rekey(keys2)
    cap.retain()
    assert cap.graph is not None                    # (only buffer contents changed)
    cap.launch()
    same(cap, eager(keys2, drawn))


def check_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    R, T = 3, 4
    keys, ys = G.split(G.key(1), R), K._data(T)
    ti, ts = H.make_tracker(G, lambda a, b: jnp.stack([a, b]))
    with pytest.raises(NotImplementedError, match="state_sites"):
        ConditionalBank(ti, ts, 64, R, T, specialize=False, ancestor_sampling=True).prepare(keys, ys)
    ConditionalBank(ti, ts, 64, R, T, specialize=False, ancestor_sampling=True, state_sites=("p", "v")).prepare(keys, ys)
    pi, ps = H.make_pair(G)                             # the step model samples "c" besides the state and the observation
    with pytest.raises(NotImplementedError, match="'c'"):
        ConditionalBank(pi, ps, 64, R, T, specialize=False, ancestor_sampling=True, state_sites=("a", "b")).prepare(keys, ys)
    with pytest.raises(ValueError, match="1 addresses for a state of 2"):
        ConditionalBank(pi, ps, 64, R, T, specialize=False, ancestor_sampling=True, state_sites=("a",)).prepare(keys, ys)
    # T = 1: there is no ancestor step; the sweep runs, conditional or not
    init, step = workloads.make_lgssm(G)
    one = ConditionalBank(init, step, 64, R, 1, specialize=False, ancestor_sampling=True).prepare(keys, K._data(1))
    one.launch()
    one.set_retained(torch.zeros((R, 1)))
    one.launch()
    assert tuple(one.draw(G.key(3)).shape) == (R, 1)
    # a counted ancestor fallback is an error of the draw, naming the count
    cb = make_bank("lgssm", 64, False, True)
    cb.set_retained(some_paths("lgssm", AB_R, AB_T))
    cb.launch()
    cb.draw(G.key(3))
    cb.status[1] = 3
    with pytest.raises(FloatingPointError, match="3 ancestor"):
        cb.draw(G.key(3))


# --- the law and the mixing, against the exact smoother of the LGSSM ------------------------------------------------------------
def check_law(be, specialize):
    """conditional_checks.check_law's recipe, unchanged, with ancestor sampling: R = 16384 chains of n = 4 particles started
    from exact draws of the smoothing distribution; after 3 iterations of run() the across-chain mean of x_t is the RTS
    mean and the mean of (x_t - RTS mean)^2 the RTS variance, each within 5 standard errors taken from the R values
    themselves.  A float64 numpy restatement scored <= 3.2 over four seeds for the correct kernel, 15 .. 17 when the logits
    omit lw, and 30 .. 31 when column n - 1's logit comes from the proposed state and not the pinned one."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    ms, Ps, x_ref = C.exact_smoother()
    init, step = workloads.make_lgssm(G)
    cb = ConditionalBank(init, step, C.LAW_N, C.LAW_R, C.LAW_T, specialize=specialize, ancestor_sampling=True)
    out = cb.run(G.key(2718), torch.from_numpy(workloads.lgssm_data(C.LAW_T)), C.LAW_ITERS,
                 retained=torch.from_numpy(x_ref.astype(np.float32)))
    x = out[C.LAW_ITERS - 1].cpu().numpy().astype(np.float64)              # [R, T]
    assert x.shape == (C.LAW_R, C.LAW_T) and np.all(np.isfinite(x))
    z = []
    for t in range(C.LAW_T):
        v = x[:, t]
        z.append((v.mean() - ms[t]) / (v.std(ddof=1) / np.sqrt(C.LAW_R)))
        s = (v - ms[t]) ** 2
        z.append((s.mean() - Ps[t]) / (s.std(ddof=1) / np.sqrt(C.LAW_R)))
    print("law: z of the means and of the second moments per step", np.round(z, 2).tolist())
    assert np.max(np.abs(z)) <= 5.0, z


MIX_R, MIX_N, MIX_T = 2048, 8, 32


@functools.lru_cache(maxsize=None)
def smoother_draws(T, R, seed=20241):
    """float64, numpy: R trajectories drawn EXACTLY from p(x_0..T-1 | y) of the LGSSM on lgssm_data(T) — the Kalman filter,
    then backward sampling (conditional_checks.exact_smoother, for any T)"""
    from genjax_amd import workloads
    p = workloads.LGSSM
    a, q, r = p["a"], p["sx"] ** 2, p["sy"] ** 2
    ys = workloads.lgssm_data(T).astype(np.float64)
    mf, Pf = np.zeros(T), np.zeros(T)
    m, P = 0.0, p["s0"] ** 2
    for t in range(T):
        if t > 0:
            m, P = a * m, a * a * P + q
        Kg = P / (P + r)
        m, P = m + Kg * (ys[t] - m), (1 - Kg) * P
        mf[t], Pf[t] = m, P
    rng = np.random.default_rng(seed)
    x = np.zeros((R, T))
    x[:, T - 1] = mf[T - 1] + np.sqrt(Pf[T - 1]) * rng.normal(size=R)
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + q
        J = Pf[t] * a / Pp
        x[:, t] = mf[t] + J * (x[:, t + 1] - a * mf[t]) + np.sqrt(Pf[t] - J * J * Pp) * rng.normal(size=R)
    x.setflags(write=False)
    return x


def check_mixing(be, specialize):
    """R = 2048 chains of n = 8 particles over T = 32 steps, retained paths drawn exactly from the smoother, ONE iteration of
    run(): with ancestor sampling x_0 leaves the retained value in at least 0.4 of the chains (a float64 numpy restatement:
    0.61, standard error 0.011), and in at least 10 times as many chains as without (the restatement: 0.001)"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    start = torch.from_numpy(smoother_draws(MIX_T, MIX_R).astype(np.float32))
    init, step = workloads.make_lgssm(G)
    frac = {}
    for flag in (False, True):
        cb = ConditionalBank(init, step, MIX_N, MIX_R, MIX_T, specialize=specialize, ancestor_sampling=flag)
        out = cb.run(G.key(1618), torch.from_numpy(workloads.lgssm_data(MIX_T)), 1, retained=start)
        x0 = out[0].cpu().numpy()[:, 0]
        frac[flag] = float(np.mean(H.bits(x0) != H.bits(start.numpy()[:, 0])))
    print("mixing: the fraction of chains whose x_0 moved, without / with ancestor sampling", frac[False], frac[True])
    assert frac[True] >= 0.4, frac
    assert frac[True] >= 10.0 * frac[False], frac
