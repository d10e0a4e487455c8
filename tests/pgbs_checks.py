"""Shared drivers of tests/test_pgbs_cpu.py (the C-ABI's CPU mirror) and tests/test_pgbs_gpu.py (the HIP library):
gmx_pick_rows_take against its definition composed from the same library's gmx_pick_rows plus numpy indexing and against
the oracle's per-row pick (integers and bits compared for equality), smc.ConditionalBank.draw(key, backward=True) against
an oracle replay of the bank's own record, draw(key), retain() and a captured bank, its law against the exact smoother of
the LGSSM, and how far one iteration moves the start of a trajectory."""
from __future__ import annotations

import ctypes
import functools
import itertools

import numpy as np
import torch

from oracle import genjax_oracle as O
from tests import ancestor_checks as A
from tests import backward_checks as B
from tests import conditional_checks as C
from tests import history_checks as H

# either side of the 1 / 2 / 4-wave packing and of the one-tile boundary; past 1024 the three-launch form
TAKE_SIZES = [1, 2, 3, 5, 64, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2049, 3000]
TAKE_COUNTS = [1, 3, 4, 5, 7, 9]        # around the 4 / 2 / 1 rows per workgroup
TAKE_COUNT_SIZES = [200, 400, 1000, 1500]  # four, two, one row(s) per workgroup; the tiled form
TAKE_DEPTHS = [0, 1, 3]
SPECIAL_SIZES = [257, 600, 1000, 1500]
LD_PAD, LW_LD_PAD = 3, 5                # odd row strides: rows that start at any 4-byte boundary, the two matrices differently
LW_POISON = np.float32(-2.5e30)
OUT_POISON = np.float32(6.5e29)
TAIL = 3                                # canary words after the last element of every output


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def take_case(n, R):
    """(logits [R, n], weights [R, n], states [3, R, n], keys [R, 2]) of a size (never modified)"""
    rng = np.random.default_rng(77 * n + R)
    out = ((2.0 * rng.normal(size=(R, n))).astype(np.float32), rng.normal(size=(R, n)).astype(np.float32),
           rng.normal(size=(3, R, n)).astype(np.float32), O.split(O.key(13), R))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def take(be, logits, keys, lw=None, x=None, stride=0, spread=True, pad=LD_PAD, lw_pad=LW_LD_PAD):
    """gmx_pick_rows_take on padded, poisoned buffers.  lw = None: lw_d IS logits_d.  x: [D, R, n] or None (D = 0), laid
    out as rows of n columns inside a wider [D, x_ld] store.  Returns what the call wrote; asserts that every input, every
    padding word and the words after the last element of each output are what they were."""
    dev = be.device
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    R, n = logits.shape
    D = 0 if x is None else int(x.shape[0])
    ld = n + pad
    host = np.full((R, ld), B.POISON, dtype=np.float32)
    host[:, :n] = logits
    lg = torch.from_numpy(host.copy()).to(dev)
    if lw is None:
        lw_t, lw_host, lw_ld = lg, host, ld
    else:
        lw_ld = n + lw_pad
        lw_host = np.full((R, lw_ld), LW_POISON, dtype=np.float32)
        lw_host[:, :n] = lw
        lw_t = torch.from_numpy(lw_host.copy()).to(dev)
    x_ld = R * n + 5
    x_host = np.full((max(D, 1), x_ld), C.X_POISON, dtype=np.float32)
    for d in range(D):
        x_host[d, :R * n] = np.asarray(x[d], np.float32).reshape(R * n)
    x_t = torch.from_numpy(x_host.copy()).to(dev)
    next_ld = R * n + 3                  # (row d > 0 of the broadcast store starts off a 16-byte boundary)
    nx0 = np.full((max(D, 1), next_ld), A.NEXT_POISON, dtype=np.float32)
    nx = torch.from_numpy(nx0.copy()).to(dev)
    k_d = torch.from_numpy(_i32(keys).reshape(R, 2)).to(dev)
    idx = torch.full((R + TAIL,), -7, dtype=torch.int32, device=dev)
    lw_out = torch.full((R + TAIL,), float(OUT_POISON), dtype=torch.float32, device=dev)
    x_out = torch.full((D * R + TAIL,), float(OUT_POISON), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_pick_rows_take_workspace(R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_pick_rows_take(be.ptr(k_d), be.ptr(lg), R, n, ld, be.ptr(lw_t), lw_ld, be.ptr(x_t) if D else None, D, x_ld, n,
                                 stride, be.ptr(idx), be.ptr(lw_out), be.ptr(x_out) if D else None,
                                 be.ptr(nx) if spread else None, next_ld, be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    assert H.same_bits(lg, host) and H.same_bits(lw_t, lw_host) and H.same_bits(x_t, x_host)      # (inputs are only read)
    idx, lw_out, x_out, nx = idx.cpu().numpy(), lw_out.cpu().numpy(), x_out.cpu().numpy(), nx.cpu().numpy()
    assert np.all(idx[R:] == -7), "idx_out: written past its end"
    assert H.same_bits(lw_out[R:], np.full(TAIL, OUT_POISON)), "lw_out: written past its end"
    assert H.same_bits(x_out[D * R:], np.full(TAIL, OUT_POISON)), "x_out: written past its end"
    assert H.same_bits(nx[:, R * n:], nx0[:, R * n:]), "next: written past rows * n"
    if not spread or D == 0:
        assert H.same_bits(nx, nx0), "next: written without a broadcast"
    return dict(idx=idx[:R], lw=lw_out[:R], x=x_out[:D * R].reshape(D, R), next=nx[:D, :R * n].reshape(D, R, n),
                status=int(status.item()))


def definition(be, logits, keys, lw, x, stride):
    """the three steps of gmx_pick_rows_take's definition: the library's own gmx_pick_rows, then numpy"""
    R, n = logits.shape
    k, status = B.pick_rows(be, logits, keys, pad=LD_PAD)
    return composed(k, status, logits, lw, x, stride)


def composed(k, status, logits, lw, x, stride):
    R, n = logits.shape
    rows = np.arange(R)
    src = logits if lw is None else lw
    D = 0 if x is None else int(x.shape[0])
    x_out = np.zeros((D, R), np.float32)
    for d in range(D):
        x_out[d] = x[d][rows, k]
    return dict(idx=(k + rows * stride).astype(np.int32), lw=np.asarray(src, np.float32)[rows, k], x=x_out,
                next=np.repeat(x_out[:, :, None], n, axis=2), status=status)


def assert_take_equal(got, want, what, spread=True):
    assert np.array_equal(got["idx"], want["idx"]), (what, got["idx"].tolist(), want["idx"].tolist())
    assert H.same_bits(got["lw"], want["lw"]), (what, "lw_out")
    assert H.same_bits(got["x"], want["x"]), (what, "x_out")
    if spread and got["x"].shape[0]:
        assert H.same_bits(got["next"], want["next"]), (what, "next", np.argwhere(H.bits(got["next"]) != H.bits(want["next"]))[:5].tolist())
    assert got["status"] == want["status"], (what, "status", got["status"], want["status"])


def check_take_case(be, n, R, oracle=True, full=True):
    """gmx_pick_rows_take == its definition for D in {0, 1, 3}, lw aliasing the logits or not, with and without the
    broadcast, index_stride 0 and n; the pick of every row also the oracle's"""
    logits, lw, x, keys = take_case(n, R)
    k, status = B.pick_rows(be, logits, keys, pad=LD_PAD)
    assert status == 0
    if oracle:
        assert k.tolist() == [B.oracle_pick(logits[r], keys[r]) for r in range(R)], n
    combos = itertools.product(TAKE_DEPTHS, (False, True), (False, True), (0, n)) if full else \
        [(1, False, True, n), (3, True, True, 0), (0, False, False, n)]
    for D, alias, spread, s in combos:
        xs = x[:D] if D else None
        got = take(be, logits, keys, lw=None if alias else lw, x=xs, stride=s, spread=spread)
        assert_take_equal(got, composed(k, 0, logits, None if alias else lw, xs, s), (n, R, D, alias, spread, s), spread)


def check_take_specials(be, n):
    """special logits, each in one row among ordinary neighbours: a row of all -inf between two live rows (answers n - 1, its
    state and weight still taken, counted once, its neighbours bitwise what they are beside a live row); -inf and NaN
    columns; all the mass in column 0, and in column n - 1; equal logits"""
    R = 8
    logits0, lw, x, keys = take_case(n, R)
    logits = logits0.copy()
    logits[1] = -np.inf
    logits[3, ::3] = -np.inf
    logits[3, 1::7] = np.nan
    logits[4] = -np.inf
    logits[4, 0] = np.float32(-1.5)
    logits[5] = -np.inf
    logits[5, n - 1] = np.float32(0.25)
    logits[6] = np.float32(-3.25)
    for alias in (False, True):
        src = None if alias else lw
        got = take(be, logits, keys, lw=src, x=x, stride=n)
        assert_take_equal(got, definition(be, logits, keys, src, x, n), (n, "specials", alias))
        assert got["status"] == 1
        local = got["idx"] - np.arange(R) * n
        assert local[1] == n - 1 and local[4] == 0 and local[5] == n - 1
        assert H.same_bits(got["x"][:, 1], x[:, 1, n - 1])
        assert H.same_bits(got["lw"][1:2], (logits if alias else lw)[1, n - 1:n])
        live = np.isfinite(logits[3])
        assert live[local[3]]                                # (a column without mass is never drawn)
        for r in (0, 2, 6, 7):                               # the ordinary neighbours and the flat row: the oracle's draw
            assert local[r] == B.oracle_pick(logits[r], keys[r]), r
        plain = take(be, logits0, keys, lw=None if alias else lw, x=x, stride=n)      # row 1 live: rows 0 and 2 do not notice
        assert plain["status"] == 0
        for r in (0, 2):
            for name in ("idx", "lw"):
                assert H.same_bits(got[name][r:r + 1], plain[name][r:r + 1]), (name, r)
            assert H.same_bits(got["x"][:, r], plain["x"][:, r]) and H.same_bits(got["next"][:, r], plain["next"][:, r]), r


# --- refusals and sizes ----------------------------------------------------------------------------------------------------
def take_refusal_calls():
    """argument tuples gmx_pick_rows_take must refuse before any launch, with what the message has to name"""
    N, i64, i32, buf, P = A._refusal_env()

    def call(keys=P, logits=P, rows=2, n=10, ld=10, lw=P, lw_ld=10, x=P, D=1, x_ld=20, x_rs=10, stride=0, idx=P, lw_out=P,
             x_out=P, nxt=P, next_ld=20, status=P, ws=P):
        return (keys, logits, i64(rows), i64(n), i64(ld), lw, i64(lw_ld), x, i32(D), i64(x_ld), i64(x_rs), i64(stride), idx,
                lw_out, x_out, nxt, i64(next_ld), status, ws, N)
    calls = [(call(**{a: N}), b"null") for a in ("keys", "logits", "lw", "idx", "lw_out", "status", "ws")]
    calls += [(call(x=N), b"x_d"), (call(x_out=N), b"x_out_d"), (call(n=0), b"n = 0"), (call(rows=0), b"rows = 0"),
              (call(rows=2 ** 31), b"rows = "), (call(ld=9), b"ld = 9"), (call(lw_ld=9), b"lw_ld = 9"),
              (call(next_ld=19), b"next_ld = 19"), (call(next_ld=2 ** 46), b"next_ld = "), (call(D=-1), b"D = -1"),
              (call(D=65534), b"D = 65534"), (call(x_ld=19), b"x_ld = 19"), (call(x_rs=-1), b"x_row_stride"),
              (call(rows=2 ** 21, n=1024, ld=1024, lw_ld=1024, stride=1024, x_ld=2 ** 31, x_rs=1024, next_ld=2 ** 31),
               b"index_stride"), (call(stride=-1), b"index_stride")]
    return calls, buf


def check_refusals_of(lib):
    """lib: a ctypes library (the HIP library without a GPU, or the mirror)"""
    lib.gmx_last_error.restype = ctypes.c_char_p
    calls, _keep = take_refusal_calls()
    for args, names in calls:
        assert lib.gmx_pick_rows_take(*args) != 0, names
        msg = lib.gmx_last_error()
        assert b"gmx_pick_rows_take" in msg and names in msg, (msg, names)


def workspace_sizes(lib):
    lib.gmx_pick_rows_take_workspace.restype = ctypes.c_size_t
    lib.gmx_pick_rows_take_workspace.argtypes = [ctypes.c_int64, ctypes.c_int64]
    return [int(lib.gmx_pick_rows_take_workspace(r, n)) for r, n in A.WORKSPACE_SHAPES]


# --- ConditionalBank.draw(key, backward=True) ------------------------------------------------------------------------------------
PB_SIZES = [4, 200, 1500]               # a handful of particles; one launch per pick; the tiled form
DRAW_SEED = 61


def _clone(v):
    return tuple(u.clone() for u in v) if isinstance(v, (tuple, list)) else v.clone()


def _record(cb):
    return [v.clone() for v in (cb.hist_xs, cb.hist_lws, cb.hist_ancs, cb.anc, cb.status)]


def check_oracle_replay(be, specialize, n, retained, ancestors, R=2, T=4):
    """every step of a backward draw from the bank's OWN recorded slabs: the logits recomputed with the oracle — lw_t + the
    weight os_.importance returns under {x: the chosen next state, y: ys[t + 1]} with args (x_t,), in float32 — and the
    pick B.oracle_pick under the documented keys; paths, trajectory and recorded weights bit for bit.  At least one pick
    is not the lineage's (n = 4: over six draw keys)."""
    import genjax_amd as G
    from genjax_amd import workloads
    cb = A.make_bank("lgssm", n, specialize, ancestors, R=R, T=T)
    if retained:
        cb.set_retained(A.some_paths("lgssm", R, T))
    cb.launch()
    xs, lws, ancs = (v.cpu().numpy() for v in (cb.hist_xs, cb.hist_lws, cb.hist_ancs))
    _oi, os_ = workloads.make_lgssm(O)
    ys = workloads.lgssm_data(T)
    any_keys = O.split(O.key(0), n)
    moved = 0
    for seed in range(DRAW_SEED, DRAW_SEED + (6 if n < 200 else 1)):
        out = cb.draw(G.key(seed), backward=True)
        traj, lw_path, paths, k_last = (v.cpu().numpy() for v in cb._last)
        assert H.same_bits(out, traj[:, 0].T)
        dk = O.key(seed)
        for r in range(R):
            sl = slice(r * n, (r + 1) * n)
            nxt = None
            for t in range(T - 1, -1, -1):
                key = (O.split(dk, R) if t == T - 1 else O.split(O.fold_in(dk, t), R))[r]
                x, lw = xs[t, 0, sl], lws[t, sl]
                if t == T - 1:
                    logits = lw
                else:
                    con = O.C.d({"x": np.float32(nxt), "y": np.float32(ys[t + 1])})
                    _, wn = os_.importance(any_keys, con, (x,))
                    logits = (lw + np.asarray(wn, np.float32)).astype(np.float32)
                k = B.oracle_pick(logits, key)
                assert paths[t, r] == k + r * n, ("paths", seed, r, t, int(paths[t, r]) - r * n, k)
                assert H.same_bits(traj[t, 0, r:r + 1], x[k:k + 1]), ("traj", seed, r, t)
                assert H.same_bits(lw_path[t, r:r + 1], lw[k:k + 1]), ("lw_path", seed, r, t)
                nxt = x[k]
        assert np.array_equal(k_last, paths[T - 1] - np.arange(R) * n)
        walked, _ = H.numpy_lineage(ancs, xs, paths[T - 1])
        moved += int(np.sum(walked != paths))
    assert moved > 0


def check_last_state(be, model, n, specialize):
    """the last state of draw(key, backward=True) is draw(key)'s, bit for bit; at T = 1 the whole draw is"""
    import genjax_amd as G
    R, T = A.AB_R, A.AB_T
    cb = A.make_bank(model, n, specialize, False)
    cb.set_retained(A.some_paths(model, R, T))
    cb.launch()
    before = _record(cb)
    a = cb.draw(G.key(17))
    last_a = [v.clone() for v in cb._last]
    b = cb.draw(G.key(17), backward=True)
    last_b = cb._last
    assert H.same_bits(last_a[0][T - 1], last_b[0][T - 1]) and H.same_bits(last_a[1][T - 1], last_b[1][T - 1])
    assert H.same_bits(last_a[2][T - 1], last_b[2][T - 1]) and H.same_bits(last_a[3], last_b[3])
    if model == "pair":
        assert isinstance(b, tuple) and len(b) == 2 and all(tuple(v.shape) == (R, T) for v in b)
        assert all(H.same_bits(u[:, T - 1], v[:, T - 1]) for u, v in zip(a, b))
    else:
        assert tuple(b.shape) == (R, T) and H.same_bits(a[:, T - 1], b[:, T - 1])
    for u, v in zip(before, _record(cb)):                   # a draw touches nothing of the sweep's
        assert H.same_bits(u, v) if u.dtype != torch.int64 else torch.equal(u, v)


def check_one_step(be):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    from tests import bank_checks as K
    R = 3
    init, step = workloads.make_lgssm(G)
    one = ConditionalBank(init, step, 64, R, 1, specialize=False).prepare(G.split(G.key(1), R), K._data(1))
    one.launch()
    a = one.draw(G.key(3)).clone()
    last = [v.clone() for v in one._last]
    b = one.draw(G.key(3), backward=True)
    assert tuple(b.shape) == (R, 1) and H.same_bits(a, b)
    assert all(H.same_bits(u, v) for u, v in zip(last, one._last))


def check_pair_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd.inference.smc import ConditionalBank
    from tests import bank_checks as K
    R, T = 3, 4
    keys, ys = G.split(G.key(1), R), K._data(T)
    init, step = A.make_pair(G)
    cb = ConditionalBank(init, step, 64, R, T, specialize=False).prepare(keys, ys)
    cb.launch()
    with pytest.raises(NotImplementedError, match="state_sites"):
        cb.draw(G.key(2), backward=True)
    ok = ConditionalBank(init, step, 64, R, T, specialize=False, state_sites=("a", "b")).prepare(keys, ys)
    ok.launch()
    out = ok.draw(G.key(2), backward=True)
    assert isinstance(out, tuple) and len(out) == 2 and all(tuple(v.shape) == (R, T) for v in out)
    pi, ps = H.make_pair(G)                             # the step model samples "c" besides the state and the observation
    pb = ConditionalBank(pi, ps, 64, R, T, specialize=False, state_sites=("a", "b")).prepare(keys, ys)
    pb.launch()
    pb.draw(G.key(2))
    with pytest.raises(NotImplementedError, match="'c'") as e:
        pb.draw(G.key(2), backward=True)
    assert "draw(backward=True)" in str(e.value)
    with pytest.raises(ValueError, match="ONE key"):
        ok.draw(keys, backward=True)


def check_retain(be, model, n, specialize):
    """retain() after a backward draw: ref_x / ref_lw are the drawn states and the recorded weights along paths; after the
    next launch() slot n - 1 of every step holds them"""
    import genjax_amd as G
    R, T = A.AB_R, A.AB_T
    cb = A.make_bank(model, n, specialize, False)
    cb.launch()                                             # the unconditional first sweep: one FFBS draw per chain
    cb.draw(G.key(23), backward=True)
    traj, lw_path, paths, _k = (v.cpu().numpy().copy() for v in cb._last)
    xs, lws = cb.hist_xs.cpu().numpy(), cb.hist_lws.cpu().numpy()
    assert H.same_bits(traj, np.stack([xs[t][:, paths[t]] for t in range(T)]))
    assert H.same_bits(lw_path, np.take_along_axis(lws, paths.astype(np.int64), axis=1))
    assert np.all(paths // n == np.arange(R)[None, :])
    cb.retain()
    assert cb.conditional
    assert H.same_bits(cb.ref_x, traj) and H.same_bits(cb.ref_lw, lw_path)
    cb.launch()
    last = np.arange(R) * n + n - 1
    assert H.same_bits(cb.hist_xs[:, :, last], traj) and H.same_bits(cb.hist_lws[:, last], lw_path)


def check_captured(be, model, n):
    """GPU: the graph survives a backward draw, rekey and retain; the replay equals an eager bank under the same keys and
    path; the slabs, anc and status are what they were before the draw"""
    import genjax_amd as G
    R, T = A.AB_R, A.AB_T
    cap = A.make_bank(model, n, True, False)
    cap.set_retained(A.some_paths(model, R, T))
    cap.capture()
    graph = cap.graph
    assert graph is not None
    cap.launch()
    before = _record(cap)
    drawn = _clone(cap.draw(G.key(8), backward=True))
    assert cap.graph is graph
    for u, v in zip(before, _record(cap)):
        assert H.same_bits(u, v) if u.dtype != torch.int64 else torch.equal(u, v)
    keys2 = G.split(G.key(123), R)
    cap.rekey(keys2)
    cap.retain()
    assert cap.graph is graph                               # (only buffer contents changed)
    cap.launch()
    e = A.make_bank(model, n, True, False, keys=keys2)
    e.set_retained(drawn)
    e.launch()
    assert H.same_bits(cap.hist_xs, e.hist_xs) and H.same_bits(cap.hist_lws, e.hist_lws) and H.same_bits(cap.hist_ancs, e.hist_ancs)
    assert np.array_equal(cap.log_ml(), e.log_ml())
    assert H.same_bits(_stack(cap.draw(G.key(9), backward=True)), _stack(e.draw(G.key(9), backward=True)))


def _stack(v):
    return torch.stack(list(v)) if isinstance(v, (tuple, list)) else v


def check_no_mass(be, n):
    """hist_lws[t] of one chain set to -inf at one t < T - 1: FloatingPointError naming that step and the count 1"""
    import pytest
    import genjax_amd as G
    R, T = A.AB_R, A.AB_T
    cb = A.make_bank("lgssm", n, False, False)
    cb.launch()
    cb.draw(G.key(4), backward=True)
    cb.hist_lws[1, n:2 * n] = -float("inf")
    with pytest.raises(FloatingPointError, match=rf"draw\(backward=True\): step 1: 1 of the {R} chains"):
        cb.draw(G.key(4), backward=True)
    cb.hist_lws[T - 1, 0:n] = -float("inf")
    with pytest.raises(FloatingPointError, match=f"final weights of 1 of the {R} chains"):
        cb.draw(G.key(4), backward=True)


# --- the law and the mixing, against the exact smoother of the LGSSM ------------------------------------------------------------
def check_law(be, specialize, ancestors):
    """conditional_checks.check_law's recipe, unchanged, with run(..., backward=True): R = 16384 chains of n = 4 particles
    started from exact draws of the smoothing distribution; after 3 iterations the across-chain mean of x_t is the RTS mean
    and the mean of (x_t - RTS mean)^2 the RTS variance, each within 5 standard errors taken from the R values themselves.
    A float64 numpy restatement scored 1.9 .. 2.3 over four seeds for backward simulation (1.8 .. 2.6 with ancestor
    sampling as well), 39.6 .. 39.9 when the logits omit lw_t and 6.6 .. 9.7 when they are taken against the retained next
    state instead of the chosen one."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    ms, Ps, x_ref = C.exact_smoother()
    init, step = workloads.make_lgssm(G)
    cb = ConditionalBank(init, step, C.LAW_N, C.LAW_R, C.LAW_T, specialize=specialize, ancestor_sampling=ancestors)
    out = cb.run(G.key(2718), torch.from_numpy(workloads.lgssm_data(C.LAW_T)), C.LAW_ITERS,
                 retained=torch.from_numpy(x_ref.astype(np.float32)), backward=True)
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


def check_mixing(be, specialize):
    """ancestor_checks.check_mixing's sizes (R = 2048 chains of n = 8 particles, T = 32, retained paths drawn exactly from
    the smoother), ONE iteration of run() without ancestor sampling: with backward=True x_0 leaves the retained value in at
    least 0.4 of the chains (a float64 numpy restatement: 0.60 .. 0.62, standard error 0.011), and in at least 10 times as
    many chains as the lineage draw (the restatement: at most 0.001)"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import ConditionalBank
    start = torch.from_numpy(A.smoother_draws(A.MIX_T, A.MIX_R).astype(np.float32))
    init, step = workloads.make_lgssm(G)
    frac = {}
    for flag in (False, True):
        cb = ConditionalBank(init, step, A.MIX_N, A.MIX_R, A.MIX_T, specialize=specialize)
        out = cb.run(G.key(1618), torch.from_numpy(workloads.lgssm_data(A.MIX_T)), 1, retained=start, backward=flag)
        x0 = out[0].cpu().numpy()[:, 0]
        frac[flag] = float(np.mean(H.bits(x0) != H.bits(start.numpy()[:, 0])))
    print("mixing: the fraction of chains whose x_0 moved, lineage / backward simulation", frac[False], frac[True])
    assert frac[True] >= 0.4, frac
    assert frac[True] >= 10.0 * frac[False], frac
