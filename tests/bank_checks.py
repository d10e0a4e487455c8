"""Shared drivers of tests/test_bank_cpu.py (the C-ABI's CPU mirror) and tests/test_bank_gpu.py (the HIP library):
gmx_resample_rows against the oracle's per-row path (integers compared for equality), smc.resample on batched collections
against the 1-D calls row by row, and smc.BootstrapBank against single BootstrapSweeps, bit for bit."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import genjax_oracle as O
from tests import backward_checks as B
from tests import history_checks as H

ROW_KINDS = {"systematic": O.SYSTEMATIC, "stratified": O.STRATIFIED, "multinomial": O.MULTINOMIAL}
# the issue's sizes, plus the sizes either side of where the packing changes (one wave per row up to 256 columns, two up
# to 512, four up to 1024: four / two / one rows per workgroup)
ROW_SIZES = [1, 5, 64, 255, 1023, 1024, 1025, 2051, 4099]
PACKING_SIZES = [256, 257, 512, 513]
ROW_SHAPES = ["gap", "hole", "last", "first", "mixed"]
# n = 100: four rows per workgroup — 1 row (a workgroup with three idle groups), 7 (one full + three), 130 (32 full + two)
ROW_COUNTS = [1, 7, 130]


# --- gmx_resample_rows alone ---------------------------------------------------------------------------------------------
def resample_rows(be, kind, rows, keys, pad=0, stride=0):
    """rows: [R, n] float32, keys: [R, 2] uint32 -> (ancestors int32 [R, n], max float32 [R], total [R] python ints, status);
    rows are n + pad elements apart, the padding poisoned"""
    dev = be.device
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    R, n = rows.shape
    ld = n + pad
    host = np.full((R, ld), B.POISON, dtype=np.float32)
    host[:, :n] = rows
    lw = torch.from_numpy(host).to(dev)
    k_d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(R, 2)).to(dev)
    anc = torch.full((R, n), -7, dtype=torch.int32, device=dev)
    mx = torch.full((R,), 7.0, dtype=torch.float32, device=dev)
    total = torch.full((R,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((be.c.gmx_resample_rows_workspace(kind, R, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_resample_rows(kind, be.ptr(k_d), be.ptr(lw), R, n, ld, stride, be.ptr(mx), be.ptr(total), be.ptr(anc),
                                be.ptr(status), be.ptr(ws), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    tot = [int(v) & 0xFFFFFFFFFFFFFFFF for v in total.cpu().tolist()]
    return anc.cpu().numpy(), mx.cpu().numpy(), tot, int(status.item())


def oracle_row(kind, row, key):
    """the per-row path: (ancestors int32 [n], total, max as float32)"""
    cdf, total, M, _ = O.weight_cdf(np.asarray(row, np.float32))
    return np.asarray(O.ancestors(kind, key, cdf)).astype(np.int32), int(total), np.float32(M)


@functools.lru_cache(maxsize=None)
def row_case(name):
    """[R, n] rows of one case (never modified): backward_checks.pick_case, or "count<R>": R rows of 100 columns"""
    if name.startswith("count"):
        rows = np.random.default_rng(100).normal(size=(max(ROW_COUNTS), 100)).astype(np.float32)[:int(name[5:])]
        rows.setflags(write=False)
        return rows
    return B.pick_case(name)


@functools.lru_cache(maxsize=None)
def row_keys(R):
    return O.split(O.key(7), R)


@functools.lru_cache(maxsize=None)
def oracle_rows(kind_name, name):
    """the oracle's answer for every row of a case, computed once and shared"""
    rows, kind = row_case(name), ROW_KINDS[kind_name]
    keys = row_keys(rows.shape[0])
    return [oracle_row(kind, rows[r], keys[r]) for r in range(rows.shape[0])]


def assert_rows_equal(got, want, stride, n, what):
    anc, mx, tot, _ = got
    for r, (a, t, M) in enumerate(want):
        assert np.array_equal(anc[r] - r * stride, a), (what, "row", r, np.argwhere(anc[r] - r * stride != a)[:5].tolist())
        assert tot[r] == t, (what, "row", r, "total", tot[r], t)
        assert H.same_bits(mx[r:r + 1], np.array([M], np.float32)), (what, "row", r, "max", mx[r], M)


def check_rows_case(be, kind_name, name, pad=0, stride=0):
    rows = row_case(name)
    R, n = rows.shape
    want = oracle_rows(kind_name, name)
    got = resample_rows(be, ROW_KINDS[kind_name], rows, row_keys(R), pad=pad, stride=n if stride else 0)
    assert got[3] == 0, got[3]
    assert_rows_equal(got, want, n if stride else 0, n, (kind_name, name, pad, stride))
    if name == "last":
        assert all(np.all(a == n - 1) for a, _, _ in want)
    if name == "first":
        assert all(np.all(a == 0) for a, _, _ in want)


def check_rows_no_mass(be, kind_name, name):
    """row 2 all -inf among normal ones: status 1, the neighbours exact, its own answer the per-row path's (n - 1)"""
    rows = row_case(name).copy()
    rows[2] = -np.inf
    R, n = rows.shape
    kind, keys = ROW_KINDS[kind_name], row_keys(R)
    want = [oracle_row(kind, rows[r], keys[r]) for r in range(R)]
    assert want[2][1] == 0 and np.all(want[2][0] == n - 1)
    got = resample_rows(be, kind, rows, keys, pad=3, stride=n)
    assert got[3] == 1, got[3]
    assert_rows_equal(got, want, n, n, (kind_name, name, "no mass"))


def rows_refusal_calls():
    """argument tuples gmx_resample_rows must refuse before any launch, with what the message has to name"""
    import ctypes
    N, i64, i32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32
    buf = (ctypes.c_int64 * 8)()
    P = ctypes.cast(buf, ctypes.c_void_p)

    def call(kind=0, keys=P, lw=P, rows=2, n=10, ld=10, stride=0, mx=P, total=P, anc=P, status=P, ws=P):
        return (i32(kind), keys, lw, i64(rows), i64(n), i64(ld), i64(stride), mx, total, anc, status, ws, N)
    calls = [(call(**{a: N}), b"null") for a in ("keys", "lw", "mx", "total", "anc", "status", "ws")]
    calls += [(call(n=0), b"n = 0"), (call(n=2 ** 21 + 1, ld=2 ** 21 + 1), b"n = "), (call(rows=0), b"rows = 0"),
              (call(rows=2 ** 31), b"rows = "), (call(ld=9), b"ld = 9"),
              (call(kind=O.MULTINOMIAL_TILED), b"GMX_RESAMPLE_MULTINOMIAL_TILED"),
              (call(kind=O.MULTINOMIAL_SORTED), b"GMX_RESAMPLE_MULTINOMIAL_SORTED"), (call(kind=7), b"kind"),
              (call(rows=2 ** 21, n=1024, ld=1024, stride=1024), b"index_stride"),        # rows * stride = 2^31
              (call(stride=-1), b"index_stride")]
    return calls, buf


# --- more rows than one launch's grid holds ---------------------------------------------------------------------------------
CHUNK_ROWS, CHUNK_N = 65537, 1025       # the smallest that reach a second chunk (65535 rows each) on the tiled path
CHUNK_CALLS = ["systematic", "multinomial", "pick"]


def check_rows_chunks(be, which):
    """row r is row r % 3 of row_case("normal1025") under key r % 3, built on the device by indexing: rows 0, 1 and 2 are
    the oracle's per-row answer bit for bit, and every row r equals row r % 3 (compared on the device)"""
    R, n = CHUNK_ROWS, CHUNK_N
    dev = be.device
    rows, keys = row_case("normal%d" % n)[:3], row_keys(4)[:3]
    of = torch.arange(R, device=dev) % 3
    lw = torch.from_numpy(np.array(rows)).to(dev)[of].contiguous()
    k_d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(3, 2)).to(dev)[of].contiguous()
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    if which == "pick":
        out = torch.full((R,), -7, dtype=torch.int32, device=dev)
        ws = torch.empty(((be.c.gmx_pick_rows_workspace(R, n) + 7) // 8,), dtype=torch.int64, device=dev)
        rc = be.c.gmx_pick_rows(be.ptr(k_d), be.ptr(lw), R, n, n, be.ptr(out), be.ptr(status), be.ptr(ws), be.stream())
        assert rc == 0, be.c.gmx_last_error()
        assert out[:3].cpu().tolist() == [B.oracle_pick(rows[r], keys[r]) for r in range(3)]
    else:
        kind = ROW_KINDS[which]
        out = torch.full((R, n), -7, dtype=torch.int32, device=dev)
        mx = torch.full((R,), 7.0, dtype=torch.float32, device=dev)
        total = torch.full((R,), -7, dtype=torch.int64, device=dev)
        ws = torch.empty(((be.c.gmx_resample_rows_workspace(kind, R, n) + 7) // 8,), dtype=torch.int64, device=dev)
        rc = be.c.gmx_resample_rows(kind, be.ptr(k_d), be.ptr(lw), R, n, n, 0, be.ptr(mx), be.ptr(total), be.ptr(out),
                                    be.ptr(status), be.ptr(ws), be.stream())
        assert rc == 0, be.c.gmx_last_error()
        got = (out[:3].cpu().numpy(), mx[:3].cpu().numpy(), [int(v) & 0xFFFFFFFFFFFFFFFF for v in total[:3].cpu().tolist()], 0)
        assert_rows_equal(got, oracle_rows(which, "normal%d" % n)[:3], 0, n, (which, "chunks"))
    assert int(status.item()) == 0
    assert torch.equal(out, out[:3][of]), (which, "a row differs from row r % 3")


# --- smc.resample on a batched collection -----------------------------------------------------------------------------------
BATCH_R, BATCH_N = 3, 1500


def _collection(smc, scalar, val, score, ret, lw):
    from genjax_amd.static import DistributionTrace, StaticTrace
    from collections import OrderedDict
    tr = StaticTrace(None, (scalar,), ret, OrderedDict(x=DistributionTrace(None, (), val, score)))
    return smc.ParticleCollection(tr, lw)


def check_resample_batched(be, kind):
    """[3, 1500] log-weights; leaves: two of shape [3, 1500], one [3, 1500, 2], one scalar — against three 1-D calls"""
    import genjax_amd as G
    from genjax_amd import engine
    from genjax_amd.inference import smc
    R, n = BATCH_R, BATCH_N
    rng = np.random.default_rng(31)
    dev = be.device
    val, score, lw = (torch.from_numpy(rng.normal(size=(R, n)).astype(np.float32)).to(dev) for _ in range(3))
    ret = torch.from_numpy(rng.normal(size=(R, n, 2)).astype(np.float32)).to(dev)
    scalar = torch.tensor(2.5, dtype=torch.float32, device=dev)
    keys = G.split(G.key(11), R)
    out = smc.resample(keys, _collection(smc, scalar, val, score, ret, lw), kind)
    assert out.weights_are_zero() and tuple(out.get_log_weights().shape) == (R, n)
    assert out.ancestors.dtype == torch.int32 and tuple(out.ancestors.shape) == (R, n)
    off = out.log_ml_offset.value()
    assert isinstance(off, np.ndarray) and off.dtype == np.float64 and off.shape == (R,)
    est = out.get_log_marginal_likelihood_estimate()
    assert tuple(est.shape) == (R,)
    tr = out.get_particles()
    assert H.same_bits(tr.args[0].reshape(1), np.array([2.5], np.float32))
    for r in range(R):
        one = smc.resample(keys[r], _collection(smc, scalar, val[r].clone(), score[r].clone(), ret[r].clone(), lw[r].clone()), kind)
        assert H.same_bits(out.ancestors[r], one.ancestors), (kind, r)
        t1 = one.get_particles()
        assert H.same_bits(tr.subtraces["x"].value[r], engine.materialize(t1.subtraces["x"].value)), (kind, r, "value")
        assert H.same_bits(tr.subtraces["x"].score[r], engine.materialize(t1.subtraces["x"].score)), (kind, r, "score")
        assert H.same_bits(tr.retval[r], engine.materialize(t1.retval)), (kind, r, "retval")
        assert off[r] == one.log_ml_offset.value(), (kind, r, off[r], one.log_ml_offset.value())
        assert H.same_bits(est[r].reshape(1), one.get_log_marginal_likelihood_estimate().reshape(1)), (kind, r, "estimate")


def check_resample_batched_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd.inference import smc
    R, n = 3, 40
    dev = be.device
    z = torch.zeros((R, n), dtype=torch.float32, device=dev)

    def coll():
        return _collection(smc, torch.tensor(0.0, device=dev), z.clone(), z.clone(), torch.zeros((R, n, 2), device=dev), z.clone())
    with pytest.raises(ValueError, match=r"\(3, 40\).*keys of shape \(3,\).*got keys of shape \(\)"):
        smc.resample(G.key(1), coll())
    with pytest.raises(ValueError, match=r"got keys of shape \(4,\)"):
        smc.resample(G.split(G.key(1), 4), coll())
    keys = G.split(G.key(1), R)
    with pytest.raises(NotImplementedError, match="n_out"):
        smc.resample(keys, coll(), "systematic", n_out=10)
    for kind in ("multinomial_tiled", "multinomial_sorted"):
        with pytest.raises(NotImplementedError, match=kind):
            smc.resample(keys, coll(), kind)


# --- BootstrapBank against single BootstrapSweeps, bit for bit ---------------------------------------------------------------
BANK_R, BANK_N, BANK_T, BANK_SEED = 5, 1500, 8, 4242
BANK_SMALL_N = 200                      # several rows per workgroup of the row resampler (four of up to 256 columns)


def _models(name):
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd import workloads
    if name == "lgssm":
        return workloads.make_lgssm(G)
    return H.make_tracker(G, lambda a, b: jnp.stack([a, b]))


def _data(T):
    from genjax_amd import workloads
    return torch.from_numpy(workloads.lgssm_data(T))


def _np_state(state):
    x, lw, anc = state
    xs = tuple(v.cpu().numpy() for v in x) if isinstance(x, (tuple, list)) else x.cpu().numpy()
    return xs, lw.cpu().numpy(), anc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def single_sweeps(device_type, model, kind, n, specialize):
    """the R single sweeps a bank is held to: (state, log_ml) per key, computed once and shared (never modified)"""
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapSweep
    init, step = _models(model)
    keys = G.split(G.key(BANK_SEED), BANK_R)
    out = []
    for r in range(BANK_R):
        sw = BootstrapSweep(init, step, n, BANK_T, resample=kind, specialize=specialize).prepare(keys[r], _data(BANK_T))
        sw.launch()
        out.append((_np_state(sw.state()), sw.log_ml()))
    return out


def assert_row_equals_sweep(bank_state, bank_log_ml, r, want, what):
    (x, lw, anc), log_ml = want
    bx, blw, banc = bank_state
    assert H.same_bits(bx[r], x), (what, r, "x")
    assert H.same_bits(blw[r], lw), (what, r, "lw")
    assert H.same_bits(banc[r], anc), (what, r, "ancestors")
    assert bank_log_ml[r] == log_ml, (what, r, bank_log_ml[r], log_ml)


def run_bank(model, kind, n, specialize, capture=False, R=BANK_R):
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapBank
    init, step = _models(model)
    bank = BootstrapBank(init, step, n, R, BANK_T, resample=kind, specialize=specialize)
    bank.prepare(G.split(G.key(BANK_SEED), BANK_R)[:R], _data(BANK_T))
    if capture:
        bank.capture()
        bank.launch()                  # two replays
    bank.launch()
    return bank


def check_bank_against_sweeps(be, model, kind, n, specialize, capture=False):
    bank = run_bank(model, kind, n, specialize, capture)
    state, log_ml = _np_state(bank.state()), bank.log_ml()
    assert log_ml.dtype == np.float64 and log_ml.shape == (BANK_R,)
    assert state[2].dtype == np.int32 and state[2].shape == (BANK_R, n) and state[1].shape == (BANK_R, n)
    assert state[0].shape == ((BANK_R, n, 2) if model == "tracker" else (BANK_R, n))
    assert int(bank.status.item()) == 0
    want = single_sweeps(be.device.type, model, kind, n, specialize)
    for r in range(BANK_R):
        assert_row_equals_sweep(state, log_ml, r, want[r], (model, kind, n, capture))


# --- params ----------------------------------------------------------------------------------------------------------------
PARAM_R, PARAM_N, PARAM_T = 4, 300, 5
PARAM_SX = (0.3, 0.5, 0.8, 1.1)


def make_lgssm_sx(G, with_init_arg):
    """the LGSSM of workloads.make_lgssm with its process-noise scale as the step model's last argument"""
    from genjax_amd import workloads
    p = workloads.LGSSM
    a, sy, s0 = p["a"], p["sy"], p["s0"]

    if with_init_arg:
        @G.gen
        def init(sx):                  # (the initial state does not depend on the process noise)
            x = G.normal(0.0, s0) @ "x"
            _ = G.normal(x, sy) @ "y"
            return x
    else:
        @G.gen
        def init():
            x = G.normal(0.0, s0) @ "x"
            _ = G.normal(x, sy) @ "y"
            return x

    @G.gen
    def step(x_prev, sx):
        x = G.normal(a * x_prev, sx) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x
    return init, step


def _param_bank(be, values, keys, specialize, as_params=True):
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapBank
    R = len(keys)
    if as_params:
        init, step = make_lgssm_sx(G, True)
        bank = BootstrapBank(init, step, PARAM_N, R, PARAM_T, specialize=specialize,
                             params=(torch.tensor(values, dtype=torch.float32),))
    else:                               # the value as a traced 0-d tensor through step_extra (not a folded constant)
        init, step = make_lgssm_sx(G, False)
        v = torch.tensor(values[0], dtype=torch.float32, device=be.device)
        bank = BootstrapBank(init, step, PARAM_N, R, PARAM_T, specialize=specialize, step_extra=lambda t: (v,))
    bank.prepare(keys, _data(PARAM_T)).launch()
    return _np_state(bank.state()), bank.log_ml()


def check_params(be, specialize):
    import genjax_amd as G
    keys = G.split(G.key(77), PARAM_R)
    state, log_ml = _param_bank(be, list(PARAM_SX), keys, specialize)
    assert len(set(log_ml.tolist())) == PARAM_R
    for r in range(PARAM_R):           # independent of R and of the row position: an R = 1 bank with that key and value
        s1, l1 = _param_bank(be, [PARAM_SX[r]], keys[r:r + 1], specialize)
        assert_row_equals_sweep(state, log_ml, r, ((s1[0][0], s1[1][0], s1[2][0]), l1[0]), ("params", "R = 1"))
    same, l_same = _param_bank(be, [PARAM_SX[1]] * PARAM_R, keys, specialize)
    ref, l_ref = _param_bank(be, [PARAM_SX[1]], keys, specialize, as_params=False)
    for r in range(PARAM_R):
        assert_row_equals_sweep(same, l_same, r, ((ref[0][r], ref[1][r], ref[2][r]), l_ref[r]), ("params", "all equal"))
    assert H.same_bits(same[0][1], state[0][1])         # (row 1 carries that value in the first bank too)


# --- the law: E[Z^] = Z ---------------------------------------------------------------------------------------------------------
LAW_R, LAW_N, LAW_T = 512, 256, 10


def check_law(be, specialize):
    """R = 512 replicate keys, n = 256, T = 10 on the LGSSM: the bootstrap filter's evidence estimate is unbiased, so the
    mean of exp(log_ml - log Z_Kalman) over the replicates is 1 up to its standard error, taken from the 512 values
    themselves; 5 standard errors (the replicates are independent: the central limit theorem puts a 5-sigma miss at
    6e-7).  No row is left out."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapBank
    init, step = workloads.make_lgssm(G)
    ys = workloads.lgssm_data(LAW_T)
    bank = BootstrapBank(init, step, LAW_N, LAW_R, LAW_T, specialize=specialize)
    bank.prepare(G.split(G.key(2024), LAW_R), torch.from_numpy(ys)).launch()
    log_ml = bank.log_ml()
    assert log_ml.shape == (LAW_R,) and np.all(np.isfinite(log_ml))
    ratio = np.exp(log_ml - workloads.kalman_log_ml(ys))
    mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(LAW_R)
    print("law: mean of Z^/Z over", LAW_R, "filters", mean, "standard error", se, "z", (mean - 1.0) / se)
    assert abs(mean - 1.0) <= 5.0 * se, (mean, se)


# --- out of scope ---------------------------------------------------------------------------------------------------------------
def check_bank_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapBank
    init, step = workloads.make_lgssm(G)
    for kw, name in ((dict(rejuvenate=object()), "rejuvenate="), (dict(history=True), "history="),
                     (dict(noise_ahead=True), "noise_ahead="), (dict(fuse_resample=True), "fuse_resample="),
                     (dict(comm=object()), "comm="), (dict(resample="multinomial_tiled"), "multinomial_tiled"),
                     (dict(resample="multinomial_sorted"), "multinomial_sorted")):
        with pytest.raises(NotImplementedError, match=name):
            BootstrapBank(init, step, 64, 3, 4, **kw)
    with pytest.raises(NotImplementedError, match=r"R \* n >= 2\^31"):
        BootstrapBank(init, step, 2 ** 20, 2 ** 11, 4)
    bank = BootstrapBank(init, step, 64, 3, 4, specialize=False)
    with pytest.raises(NotImplementedError, match="per-filter observations"):
        bank.prepare(G.split(G.key(1), 3), torch.zeros((3, 4)))
    with pytest.raises(ValueError, match=r"keys of shape \(3,\)"):
        bank.prepare(G.key(1), torch.zeros((4,)))
