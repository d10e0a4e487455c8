"""Tile-relative addressing of the specialised kernels (csrc/gmx_jit.h: everything indexed by a particle's own row is
a workgroup-uniform base plus a 32-bit offset inside the tile), at the sizes where it can go wrong: one lane, under one
256-particle group, exactly one 1024-particle tile, a tile of one particle, three tiles with a short last one; rows of a
2-D launch that start at no multiple of a tile; `[T, n]` and 8-bit leaves.  Everything is held bit for bit to the C oracle
or to Threefry blocks computed on the host (gmx_threefry2x32_host)."""
from ctypes import c_uint32

import numpy as np
import pytest
import torch

from oracle import genjax_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu


# ---- sweeps ---------------------------------------------------------------------------------------------------------
_T = 3
_REF = {}


def _sweep_ref(n, seed):
    if n not in _REF:
        from genjax_amd import workloads
        oi, os_ = workloads.make_lgssm(O)
        _REF[n] = parity.oracle_bootstrap_sweep(oi, os_, n, _T, workloads.lgssm_data(_T), O.key(seed))
    return _REF[n]


@pytest.mark.parametrize("n", [1, 255, 1024, 1025, 2049])
def test_sweep_sizes(gpu, n):
    """BootstrapSweep, T = 3: one launch per step and two, noise ahead on and off, eager and captured — state,
    log-weights, ancestors (the index field of a tagged word), integer totals and log_ml against the oracle."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    seed = 1000 + n
    ys = workloads.lgssm_data(_T)
    init, step = workloads.make_lgssm(G)
    ref = _sweep_ref(n, seed)
    for fuse in (True, False):
        for na in (True, False):
            for capture in (False, True):
                what = dict(n=n, fuse=fuse, noise_ahead=na, capture=capture)
                sw = BootstrapSweep(init, step, n, _T, specialize=True, noise_ahead=na, fuse_resample=fuse).prepare(
                    G.key(seed), torch.from_numpy(ys))
                assert sw.fuse == fuse and sw.noise_ahead == na, what
                assert sw.p_init.comp.is_specialized() and sw.p_step.comp.is_specialized(), what
                if capture:
                    sw.capture()
                    sw.launch()
                sw.launch()
                log_ml = sw.log_ml()
                x, lw, anc = sw.state()
                assert np.array_equal(x.cpu().numpy(), ref["x"]), what
                assert np.array_equal(lw.cpu().numpy().view(np.uint32), ref["lw"].view(np.uint32)), what
                assert np.array_equal(anc.cpu().numpy() & 0xFFFFFF, ref["anc"]), what
                assert np.array_equal(sw.totals.cpu().numpy().view(np.uint64),
                                      np.array([h["total"] for h in ref["hist"]], dtype=np.uint64)), what
                assert log_ml == ref["log_ml"], (what, log_ml, ref["log_ml"])


# ---- keys: the background program's draws from Threefry blocks on the host ------------------------------------------
_CHAIN, _ELEM = (7,), 3


def _tf(be, k, c0, c1):
    out = (c_uint32 * 2)()
    be.c.gmx_threefry2x32_host(int(k[0]), int(k[1]), int(c0) & 0xFFFFFFFF, int(c1) & 0xFFFFFFFF, out)
    return int(out[0]), int(out[1])


def _host_uniforms(be, row_key, offset, n):
    """uniform(fold_in(split(row_key, .)[offset + j], 7), (), 0, 1) element 3 for j < n: the child is the Threefry block
    of the 64-bit counter offset + j as (hi, lo); value = bits_to_unit(hi ^ lo of the block of counter 3)"""
    bits = np.empty(n, dtype=np.uint32)
    for j in range(n):
        ctr = offset + j
        k = _tf(be, row_key, ctr >> 32, ctr)
        for c in _CHAIN:
            k = _tf(be, k, 0, c)
        a, b = _tf(be, k, 0, _ELEM)
        bits[j] = a ^ b
    return ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def _noise_program(n, specialize):
    from genjax_amd.static import NoiseProgram
    q = NoiseProgram([("LDKEY", _CHAIN, _ELEM, "uniform")], (n,))
    if specialize:
        q.comp.set_background(0)
        assert q.comp.specialize()
    assert q.comp.is_specialized() == specialize
    return q


_ROWS = np.array([[0x243F6A88, 0x85A308D3], [0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]], dtype=np.uint32)


@pytest.mark.parametrize("jit", [True, False])
def test_key_indices(gpu, monkeypatch, jit):
    """GMX_KEY_SPLIT and GMX_KEY_ROWSPLIT with index_offset in {0, 2^32 - 512, 2^33 + 7}, n = 1024 (the middle one
    crosses a multiple of 2^32 inside the launch): the specialised kernel (a 2-D launch for the rows) and, with
    GENMI_JIT=0, the interpreter."""
    from genjax_amd.random import Key, lazy_split
    if not jit:
        monkeypatch.setenv("GENMI_JIT", "0")
    n, dev = 1024, gpu.device
    q = _noise_program(n, jit)
    for offset in (0, 2 ** 32 - 512, 2 ** 33 + 7):
        want = [_host_uniforms(gpu, _ROWS[r], offset, n) for r in range(2)]
        out = torch.zeros((1, n), dtype=torch.float32, device=dev)
        q.run((n,), lazy_split(Key(host=_ROWS[0].copy()), n, offset), [out])
        assert np.array_equal(out.cpu().numpy().reshape(n).view(np.uint32), want[0].view(np.uint32)), ("split", offset)
        kd = torch.from_numpy(_ROWS[:2].view(np.int32).copy()).to(dev)
        out2 = torch.zeros((1, 2 * n), dtype=torch.float32, device=dev)
        q.run((2 * n,), Key(lazy=("rowsplit", Key(dev=kd), n), split_last=True, offset=offset), [out2])
        got = out2.cpu().numpy().reshape(2, n)
        for r in range(2):
            assert np.array_equal(got[r].view(np.uint32), want[r].view(np.uint32)), ("rowsplit", offset, r)


def test_rows_of_a_2d_launch(gpu):
    """three rows of keys, n = 1025: rows 1 and 2 start at no multiple of a tile, every row ends in a one-particle tile.
    The draws are those of three 1-D launches, and the host's."""
    from genjax_amd.random import Key, lazy_split
    n, dev, offset = 1025, gpu.device, 5
    q = _noise_program(n, True)
    kd = torch.from_numpy(_ROWS.view(np.int32).copy()).to(dev)
    out = torch.full((1, 3 * n + 1), -1.0, dtype=torch.float32, device=dev)
    q.run((3 * n,), Key(lazy=("rowsplit", Key(dev=kd), n), split_last=True, offset=offset), [out[:, :3 * n]])
    got = out.cpu().numpy().reshape(-1)
    assert got[3 * n] == -1.0                                    # nothing past the last row
    for r in range(3):
        one = torch.zeros((1, n), dtype=torch.float32, device=dev)
        q.run((n,), lazy_split(Key(host=_ROWS[r].copy()), n, offset), [one])
        assert np.array_equal(got[r * n:(r + 1) * n].view(np.uint32), one.cpu().numpy().reshape(n).view(np.uint32)), r
    assert np.array_equal(got[:n].view(np.uint32), _host_uniforms(gpu, _ROWS[0], offset, n).view(np.uint32))


# ---- [T, n] and 8-bit leaves through specialised kernels --------------------------------------------------------------
@pytest.fixture()
def always_specialize(monkeypatch):
    """every program specialises at its first launch, whatever its size"""
    from genjax_amd import engine
    monkeypatch.setattr(engine, "JIT_MIN_PARTICLES", 1)
    seen = []
    orig = engine.Compiled.specialize

    def spec(self, only_needed=False):
        ok = orig(self, only_needed)
        seen.append(ok)
        return ok
    monkeypatch.setattr(engine.Compiled, "specialize", spec)
    return seen


def test_step_leaves(gpu, always_specialize):
    """a scan of T = 3 steps over n = 1025 particles: the sites' values are stepped stores into `[T, n]` leaves, and an
    Update of every step's observation reads the `[T, n]` leaf of the latent path back (GMX_F_STEP)."""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, Diff, Update, numpy as jnp
    n, T, seed = 1025, 3, 5
    ys = np.array([0.3, -0.2, 0.5], np.float32)

    def mk(g):
        @g.gen
        def step(x, t):
            xn = g.normal(0.9 * x, 0.5) @ "x"
            g.normal(xn, 1.0) @ "y"
            return xn, xn * 2.0
        return step
    step, ostep = mk(G), mk(O)
    dev = gpu.device
    sc, osc = step.scan(n=T), O.Scan(ostep, T)
    a, oa = (torch.zeros(n, device=dev), jnp.zeros(T)), (np.zeros(n, np.float32), np.zeros(T, np.float32))
    t, ot = sc.simulate(G.split(G.key(seed), n), a), osc.simulate(O.split(O.key(seed), n), oa)
    for addr in ("x", "y"):
        got = t.get_choices()[addr].cpu().numpy()
        assert got.shape == (n, T) and np.array_equal(got, ot.get_choices()[addr]), addr
    assert np.array_equal(t.get_score().cpu().numpy(), ot.get_score())
    u, w, _, bwd = Update(C["y"].set(ys)).edit(G.split(G.key(seed + 1), n), t, Diff.no_change(a))
    ou, ow = O.scan_edit(osc, O.split(O.key(seed + 1), n), ot, oa, update=O.C.d({"y": ys}))
    assert np.array_equal(w.cpu().numpy(), ow)
    assert np.array_equal(u.get_score().cpu().numpy(), ou.get_score())
    assert np.array_equal(u.get_choices()["x"].cpu().numpy(), ot.get_choices()["x"])
    assert np.array_equal(bwd.constraint["y"].cpu().numpy(), ot.get_choices()["y"])
    assert always_specialize and all(always_specialize), always_specialize


def test_u8_leaves(gpu, always_specialize):
    """a flip site at n = 1025: its value is an 8-bit store, and assess reads the 8-bit leaf back"""
    import genjax_amd as G
    n, seed = 1025, 9

    def mk(g, lit):
        @g.gen
        def model():
            p = g.uniform(lit(0.2), lit(0.8)) @ "p"
            v = g.flip(p) @ "v"
            return v
        return model
    m, om = mk(G, float), mk(O, np.float32)
    tr, otr = m.simulate(G.split(G.key(seed), n), ()), om.simulate(O.split(O.key(seed), n), ())
    v = tr.get_choices()["v"].cpu().numpy()
    assert v.shape == (n,) and 0 < int(v.sum()) < n
    assert np.array_equal(v, otr.get_choices()["v"])
    assert np.array_equal(tr.get_choices()["p"].cpu().numpy(), otr.get_choices()["p"])
    assert np.array_equal(tr.get_score().cpu().numpy(), otr.get_score())
    s, _ = m.assess(tr.get_choices(), ())
    os_, _ = om.assess(otr.get_choices(), (), batch_shape=(n,))
    assert np.array_equal(s.cpu().numpy(), os_) and np.array_equal(s.cpu().numpy(), tr.get_score().cpu().numpy())
    assert always_specialize and all(always_specialize), always_specialize
