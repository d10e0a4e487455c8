"""`-m gpu` parity tests: every check goes through libgenmi_hip.so (the C-ABI)
on an MI355X and is compared with the CPU oracle on the same seeded inputs.
Integer / index results must be bit-exact; float results are bit-exact by
construction for elementwise work (same IEEE op sequence) and within the
stated tolerance for tree-ordered reductions."""
import sys

import os

import numpy as np
import pytest
import torch

from oracle import genjax_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_library_is_hip(gpu):
    assert gpu.device.type == "cuda"
    from genjax_amd import _lib
    assert gpu.c.gmx_version() == _lib.ABI_VERSION


def test_key_kernels_bit_exact(gpu):
    import genjax_amd as G
    from genjax_amd.random import lazy_split
    k = G.key(314159)
    for n in (1, 63, 64, 1000, 100_003):
        dev = lazy_split(k, n).data().cpu().numpy().view(np.uint32)
        ref = O.split(O.key(314159), n)
        assert np.array_equal(dev, ref)
    rows = G.split(k, 7)
    big = G.random.Key(lazy=("rowsplit", rows, 5000)).data().cpu().numpy().view(np.uint32).reshape(7, 5000, 2)
    assert np.array_equal(big, O.split(O.split(O.key(314159), 7), 5000))


def test_jax_docs_values_on_device(gpu):
    """The values jax's documentation prints for key(42) (see tests/test_oracle_pins.py), through the
    product: split -> key data, normal(key), normal(subkey)."""
    import genjax_amd as G
    k = G.key(42)
    ks = G.split(k)
    assert ks.data().cpu().numpy().view(np.uint32).reshape(2, 2).tolist() == [[1832780943, 270669613],
                                                                             [64467757, 2916123636]]
    assert float(G.normal.sample(k, 0.0, 1.0)) == float(np.float32(-0.028304616))
    new_key, subkey = ks
    assert float(G.normal.sample(subkey, 0.0, 1.0)) == float(np.float32(0.60576403))
    ind = G.normal.sample(G.split(k, 3), 0.0, 1.0).cpu().numpy()
    assert np.all(np.abs(ind.astype(np.float64) - [0.07592554, 0.60576403, 0.4323065]) < 5.1e-9)    # digits as printed
    import numpy
    allatonce = G.normal.sample(k, numpy.zeros(3, numpy.float32), 1.0).cpu().numpy()
    assert np.all(np.abs(allatonce.reshape(-1).astype(np.float64) - [-0.02830462, 0.46713185, 0.29570296]) < 5.1e-9)
    # the tutorial's loop of splits: draw 0 / 1 / 2 exactly as printed
    draws, kk = [], k
    for _ in range(3):
        kk, sub = G.split(kk)
        draws.append(repr(float(G.normal.sample(sub, 0.0, 1.0))))
    assert draws == ["0.6057640314102173", "-0.21089035272598267", "-0.3948981463909149"]
    # "The Sharp Bits" (jax >= 0.5 edition): key(0) -> normal [1.6226422]; split -> [1797259609 2579123966],
    # [928981903 3453687069] --> normal [-2.4424558]
    k0 = G.key(0)
    assert G.normal.sample(k0, numpy.zeros(1, numpy.float32), 1.0).cpu().numpy().reshape(-1).tolist() == [float(np.float32(1.6226422))]
    ks0 = G.split(k0)
    assert ks0.data().cpu().numpy().view(np.uint32).reshape(2, 2).tolist() == [[1797259609, 2579123966], [928981903, 3453687069]]
    assert G.normal.sample(ks0[1], numpy.zeros(1, numpy.float32), 1.0).cpu().numpy().reshape(-1).tolist() == [float(np.float32(-2.4424558))]


def _models(g):
    @g.gen
    def model(x_prev):
        x = g.normal(0.9 * x_prev, 0.5) @ "x"
        y = g.normal(x, 1.0) @ "y"
        return x
    return model


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10_000])
def test_gfi_simulate_importance_assess(gpu, n):
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    m, mo = _models(G), _models(O)
    keys, keyso = G.split(G.key(7), n), O.split(O.key(7), n)
    xp = np.linspace(-3, 3, n).astype(np.float32)
    tr = m.simulate(keys, (_dev(xp),))
    tro = mo.simulate(keyso, (xp,))
    for a in ("x", "y"):
        assert np.array_equal(tr.get_choices()[a].cpu().numpy(), tro.get_choices()[a])
    assert np.array_equal(tr.get_score().cpu().numpy(), tro.get_score())
    tr, w = m.importance(keys, C["y"].set(0.7), (_dev(xp),))
    tro, wo = mo.importance(keyso, O.C.d({"y": np.float32(0.7)}), (xp,))
    assert np.array_equal(tr.get_choices()["x"].cpu().numpy(), tro.get_choices()["x"])
    assert np.array_equal(w.cpu().numpy(), wo)
    s, _ = m.assess(C.kw(x=_dev(xp), y=0.3), (_dev(xp),))
    so, _ = mo.assess(O.C.kw(x=xp, y=np.float32(0.3)), (xp,), batch_shape=(n,))
    assert np.array_equal(s.cpu().numpy(), so)


def test_specialized_equals_interpreter(gpu):
    """gmx_program_specialize: same bits as the interpreter on a program that
    exercises most op classes (Beta / categorical / trig included)."""
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd import static

    @G.gen
    def m(a, b):
        p = G.beta(2.0, 3.0) @ "p"
        f = G.flip(p) @ "f"
        z = G.normal(jnp.where(f, a, b) + jnp.cos(a) * jnp.tanh(b), jnp.exp(0.1 * b)) @ "z"
        u = G.uniform(-1.0, 2.0) @ "u"
        k = G.categorical(logits=jnp.array([0.1, 0.2, 0.3]) * u) @ "k"
        w = G.bernoulli(logits=z) @ "w"
        return z * u + jnp.lgamma(jnp.abs(z) + 1.0)
    n = 20_000
    keys = G.split(G.key(3), n)
    a = _dev(np.linspace(-2, 2, n).astype(np.float32))
    b = _dev(np.linspace(1, -1, n).astype(np.float32))
    tr1 = m.simulate(keys, (a, b))
    comps = [c[0] for c in static._CACHE.values() if hasattr(c[0], "specialize")]
    assert comps and all(c.specialize() for c in comps), gpu.c.gmx_last_error()
    tr2 = m.simulate(keys, (a, b))
    for addr in ("p", "f", "z", "u", "k", "w"):
        v1, v2 = tr1.get_choices()[addr], tr2.get_choices()[addr]
        assert torch.equal(v1, v2), addr
    assert torch.equal(tr1.get_score(), tr2.get_score())
    assert torch.equal(tr1.get_retval(), tr2.get_retval())


def test_elementary_functions_bit_exact(gpu):
    """exp/log/... on the device == the oracle's C restatement, bit for bit."""
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, 10, 50_000), rng.uniform(-88, 88, 50_000)]).astype(np.float32)
    pos = np.abs(x) + np.float32(1e-3)
    unit = rng.uniform(-0.999, 0.999, x.size).astype(np.float32)
    cases = [("exp", jnp.exp, O.exp, x), ("log", jnp.log, O.log, pos), ("log1p", jnp.log1p, O.log1p, pos - 1),
             ("sqrt", jnp.sqrt, O.sqrt, pos), ("sin", jnp.sin, O.sin, x), ("cos", jnp.cos, O.cos, x),
             ("tanh", jnp.tanh, O.tanh, x / 10), ("sigmoid", jnp.sigmoid, O.sigmoid, x),
             ("softplus", jnp.softplus, O.softplus, x), ("lgamma", jnp.lgamma, O.lgamma, pos)]
    for name, f, fo, arg in cases:
        @G.gen
        def m(v, f=f):
            G.normal(f(v), 1.0) @ "z"
            return f(v)
        _, r = m.assess(G.ChoiceMap.kw(z=0.0), (_dev(arg),))
        assert np.array_equal(r.cpu().numpy().view(np.uint32), fo(arg).view(np.uint32)), name


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 4096, 100_000, 1_000_000])
def test_weight_cdf_bit_exact(gpu, n):
    from genjax_amd.inference import smc
    rng = np.random.default_rng(n)
    lw = (rng.normal(0, 3, n) - 5).astype(np.float32)
    if n > 10:
        lw[3] = -np.inf
    cdf, total, mx, shift = smc.weight_cdf(_dev(lw))
    rc, rt, rm, rs = O.weight_cdf(lw)
    assert shift == rs
    assert float(mx.item()) == rm
    assert np.array_equal(cdf.cpu().numpy().view(np.uint64), rc)
    assert int(total.item()) == rt


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 7, 1000, 65_537])
def test_ancestors_bit_exact(gpu, kind, n):
    import genjax_amd as G
    from genjax_amd.inference import smc
    rng = np.random.default_rng(100 + n)
    lw = rng.normal(0, 2, n).astype(np.float32)
    cdf, total, _, _ = smc.weight_cdf(_dev(lw))
    anc = smc.ancestors_from_cdf(kind, G.key(99), cdf, total)
    rc, _, _, _ = O.weight_cdf(lw)
    ref = O.ancestors(kind, O.key(99), rc)
    assert np.array_equal(anc.cpu().numpy(), ref)
    if kind != 2:
        assert np.all(np.diff(anc.cpu().numpy()) >= 0)        # sortedness property


def test_ancestors_degenerate_weights(gpu):
    """all mass on one particle -> every ancestor is that particle"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    n = 5000
    lw = np.full(n, -1e30, dtype=np.float32)
    lw[1234] = 0.0
    cdf, total, _, _ = smc.weight_cdf(_dev(lw))
    for kind in (0, 1, 2):
        anc = smc.ancestors_from_cdf(kind, G.key(1), cdf, total).cpu().numpy()
        assert np.all(anc == 1234)


@pytest.mark.parametrize("shape", [(1, 10), (1, 4097), (1, 1_000_000), (50, 50), (3, 70_000), (1000, 7)])
def test_logsumexp(gpu, shape):
    from genjax_amd import engine
    rng = np.random.default_rng(5)
    x = rng.normal(0, 5, shape).astype(np.float32)
    got = engine.logsumexp_rows(_dev(x)).cpu().numpy()
    ref = np.log(np.sum(np.exp(x.astype(np.float64) - x.max(-1, keepdims=True)), -1)) + x.max(-1)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6)     # f32 tree sum vs f64


@pytest.mark.parametrize("shape", [(1, 10), (7, 1023), (1, 1024), (3, 1025), (5, 4096), (50, 100_001), (2, 1_000_000),
                                   (1000, 100)])
def test_rows_summed_in_element_order(gpu, shape):
    """gmx_sum_rows_inorder: ((x0 + x1) + x2) + ... bit for bit, on both of its kernels (a thread per short row, a wave
    per long contiguous row) and on a strided view"""
    from genjax_amd import engine
    rng = np.random.default_rng(11)
    x = (rng.normal(0, 3, shape) * np.exp(rng.normal(0, 4, shape))).astype(np.float32)
    ref = np.cumsum(x, axis=1, dtype=np.float32)[:, -1]        # numpy's cumsum is the sequential chain
    got = engine.sum_rows_inorder(_dev(x)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    wide = _dev(np.concatenate([x, x], axis=1))
    got = engine.sum_rows_inorder(wide[:, :shape[1]]).cpu().numpy()                 # row stride != cols
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    got = engine.sum_rows_inorder(wide[:, ::2][:, :(shape[1] + 1) // 2]).cpu().numpy()   # column stride 2
    x2 = np.concatenate([x, x], axis=1)[:, ::2][:, :(shape[1] + 1) // 2]
    ref2 = np.cumsum(x2, axis=1, dtype=np.float32)[:, -1]
    assert np.array_equal(got.view(np.uint32), ref2.view(np.uint32))


def test_gather_and_categorical(gpu):
    import genjax_amd as G
    from genjax_amd import engine
    rng = np.random.default_rng(3)
    n = 10_000
    a = rng.normal(size=n).astype(np.float32)
    b = rng.integers(0, 100, size=(n, 3)).astype(np.int32)
    c = rng.integers(0, 2, size=n).astype(bool)
    anc = rng.integers(0, n, size=7777).astype(np.int32)
    ga, gb, gc = engine.gather_leaves([_dev(a), _dev(b), _dev(c)], _dev(anc))
    assert np.array_equal(ga.cpu().numpy(), a[anc])
    assert np.array_equal(gb.cpu().numpy(), b[anc])
    assert np.array_equal(gc.cpu().numpy(), c[anc])
    # all leaves 4 bytes wide: the four-outputs-per-thread kernel (k_gather4), ragged tails and sorted / random ancestors
    for m in (1, 3, 4, 7777, 100_001):
        for srt in (False, True):
            an = rng.integers(0, n, size=m).astype(np.int32)
            an = np.sort(an) if srt else an
            ga, gb = engine.gather_leaves([_dev(a), _dev(b)], _dev(an))
            assert np.array_equal(ga.cpu().numpy(), a[an]) and np.array_equal(gb.cpu().numpy(), b[an])
    logits = rng.normal(size=(64, 500)).astype(np.float32)
    keys = G.split(G.key(11), 64)
    idx = engine.categorical_rows(keys, _dev(logits)).cpu().numpy()
    ref = O.categorical.sample(O.split(O.key(11), 64), logits)
    assert np.array_equal(idx, ref)


@pytest.mark.parametrize("n,T,capture,specialize", [(4096, 5, False, False), (4096, 5, True, False),
                                                    (4096, 5, False, True), (100_000, 8, True, True),
                                                    (100_000, 8, True, False)])
def test_lgssm_sweep_matches_oracle(gpu, n, T, capture, specialize):
    """interpreter AND hiprtc-specialised kernels vs the oracle, bit for bit"""
    res = parity.check_lgssm_sweep(n=n, T=T, capture=capture, specialize=specialize)
    assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"], res
    assert res["lw_max_abs_diff"] == 0.0
    assert res["log_ml"] == res["log_ml_oracle"]


@pytest.mark.parametrize("n", [3000, 300_000])
def test_nonlinear_ssm_with_mh_rejuvenation(gpu, n):
    """BASELINE config 3 (miniature and mid-size): resample -> fused MH -> extend,
    states / weights / ancestors / accept masks bit-exact vs the oracle."""
    res = parity.check_nlssm_mh(n=n, T=4)
    assert res["ok"], res


def test_edit_requests_bit_exact(gpu):
    """Update / Regenerate / StaticRequest(Rejuvenate) weights and values vs the oracle."""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, SelectionBuilder as S

    def mk(g):
        @g.gen
        def linked():
            y1 = g.normal(0.0, 3.0) @ "y1"
            _ = g.normal(y1, 0.01) @ "y2"
        return linked
    m, mo = mk(G), mk(O)
    n = 5000
    ks, kso = G.split(G.key(314159), n), O.split(O.key(314159), n)
    tr, w = m.importance(ks, C.kw(y2=3.0), ())
    tro, wo = mo.importance(kso, O.C.kw(y2=np.float32(3.0)), ())
    assert np.array_equal(w.cpu().numpy(), wo)
    k2, k2o = G.split(G.key(5), n), O.split(O.key(5), n)
    new_tr, fw, _, _ = G.Regenerate(S["y1"]).edit(k2, tr, ())
    new_tro, fwo, _ = mo.regenerate(k2o, tro, O.selection("y1"), ())
    assert np.array_equal(fw.cpu().numpy(), fwo)
    assert np.array_equal(new_tr.get_choices()["y1"].cpu().numpy(), new_tro.get_choices()["y1"])
    nv = np.linspace(2.9, 3.1, n).astype(np.float32)
    u_tr, uw, _, disc = m.update(k2, tr, C.kw(y1=_dev(nv)), ())
    u_tro, uwo, udo = mo.update(k2o, tro, O.C.kw(y1=nv), ())
    assert np.array_equal(uw.cpu().numpy(), uwo) and np.array_equal(disc["y1"].cpu().numpy(), udo["y1"])
    req = G.StaticRequest({"y1": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.3))})
    r_tr, rw, _, _ = req.edit(k2, tr, ())
    r_tro, rwo = mo.edit_static(k2o, tro, {"y1": O.Rejuvenate(O.normal, lambda chm: (chm.get_value(), np.float32(0.3)))}, ())
    assert np.array_equal(rw.cpu().numpy(), rwo)
    assert np.array_equal(r_tr.get_choices()["y1"].cpu().numpy(), r_tro.get_choices()["y1"])


def test_importancek_and_vector_sites(gpu):
    """BASELINE config 4 in miniature: 8-schools ImportanceK + global systematic resample."""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, numpy as jnp
    from genjax_amd.inference import smc
    sig = [15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0]
    ys = np.array([28, 8, -3, 7, -1, 1, 18, 12], np.float32)

    @G.gen
    def schools():
        mu = G.normal(0.0, 5.0) @ "mu"
        log_tau = G.normal(0.0, 1.0) @ "log_tau"
        theta = G.normal(mu * jnp.ones(8), jnp.exp(log_tau) * jnp.ones(8)) @ "theta"
        _ = G.normal(theta, jnp.array(sig)) @ "y"
        return theta

    @O.gen
    def o_schools():
        mu = O.normal(0.0, 5.0) @ "mu"
        log_tau = O.normal(0.0, 1.0) @ "log_tau"
        theta = O.normal(mu[..., None] * np.ones(8, np.float32), O.exp(log_tau)[..., None] * np.ones(8, np.float32)) @ "theta"
        _ = O.normal(theta, np.array(sig, np.float32)) @ "y"
        return theta
    k = 20_000
    coll = smc.ImportanceK(G.Target(schools, (), C["y"].set(ys)), k_particles=k).run_smc(G.key(2))
    oc = O.ImportanceK(O.Target(o_schools, (), O.C.d({"y": ys})), k).run_smc(O.key(2))
    assert np.array_equal(coll.get_log_weights().cpu().numpy(), oc.get_log_weights())
    assert np.array_equal(coll.get_particles().get_choices()["theta"].cpu().numpy(), oc.get_particles().get_choices()["theta"])
    res = smc.resample(G.key(3), coll, "systematic")
    cdf, total, M, shift = O.weight_cdf(oc.get_log_weights())
    assert np.array_equal(res.ancestors.cpu().numpy(), O.ancestors(O.SYSTEMATIC, O.key(3), cdf))
    th = res.get_particles().get_choices()["theta"]
    assert np.array_equal(th.cpu().numpy(), oc.get_particles().get_choices()["theta"][res.ancestors.cpu().numpy()])
    lml = float(coll.get_log_marginal_likelihood_estimate())
    assert lml == pytest.approx(float(oc.get_log_marginal_likelihood_estimate()), rel=2e-6)


def test_config4_size_sorted_multinomial(gpu):
    """BASELINE config 4's k = 1e7 resampled with `multinomial_sorted` (past 2^21 particles the
    resampler reads tile prefixes and the table kernels walk the tiles in chunks): bit-exact vs the oracle"""
    assert parity.check_multinomial_sorted_big(n=10_000_000, seed=3) > 1_000_000
    assert parity.check_multinomial_sorted_big(n=(1 << 21) + 1, seed=4) > 100_000


def test_config4_full_size_importancek_and_global_resample(gpu):
    """BASELINE config 4 at its full size on one GPU: 8-schools, ImportanceK with k = 1e7 particles,
    one global systematic resample (2442 scan tiles: the ticketed look-back path of k_weight_cdf).
    Everything bit-exact against the oracle (C samplers / densities, unsigned __int128 ancestors)."""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, numpy as jnp
    from genjax_amd.inference import smc
    sig = parity.SCHOOL_SIGMA
    ys = parity.SCHOOL_Y

    @G.gen
    def schools():
        mu = G.normal(0.0, 5.0) @ "mu"
        log_tau = G.normal(0.0, 1.0) @ "log_tau"
        theta = G.normal(mu * jnp.ones(8), jnp.exp(log_tau) * jnp.ones(8)) @ "theta"
        _ = G.normal(theta, jnp.array(sig)) @ "y"
        return theta

    @O.gen
    def o_schools():
        mu = O.normal(0.0, 5.0) @ "mu"
        log_tau = O.normal(0.0, 1.0) @ "log_tau"
        theta = O.normal(mu[..., None] * np.ones(8, np.float32), O.exp(log_tau)[..., None] * np.ones(8, np.float32)) @ "theta"
        _ = O.normal(theta, np.array(sig, np.float32)) @ "y"
        return theta
    k = 10_000_000
    coll = smc.ImportanceK(G.Target(schools, (), C["y"].set(ys)), k_particles=k).run_smc(G.key(2))
    oc = O.ImportanceK(O.Target(o_schools, (), O.C.d({"y": ys})), k).run_smc(O.key(2))
    lw = coll.get_log_weights().cpu().numpy()
    assert np.array_equal(lw, oc.get_log_weights())
    otheta = oc.get_particles().get_choices()["theta"]
    assert np.array_equal(coll.get_particles().get_choices()["theta"].cpu().numpy(), otheta)
    res = smc.resample(G.key(3), coll, "systematic")
    cdf, total, M, shift = O.weight_cdf(oc.get_log_weights())
    anc = res.ancestors.cpu().numpy()
    assert np.array_equal(anc, O.ancestors_c(O.SYSTEMATIC, O.key(3), cdf))
    th = res.get_particles().get_choices()["theta"]
    assert np.array_equal(th.cpu().numpy(), otheta[anc])
    # size-independent properties: sorted ancestors, offspring counts within 1 of n*w
    assert np.all(np.diff(anc) >= 0)
    counts = np.bincount(anc, minlength=k).astype(np.float64)
    q = np.diff(np.concatenate([[0], cdf.astype(np.float64)]))
    assert np.max(np.abs(counts - k * q / float(total))) <= 1.0 + 1e-6
    # evidence: float32 tree reduction on the device vs float64 on the host
    lml = float(coll.get_log_marginal_likelihood_estimate())
    ref = float(np.log(np.mean(np.exp(lw.astype(np.float64) - lw.max()))) + lw.max())
    assert lml == pytest.approx(ref, rel=1e-5)


@pytest.mark.parametrize("n", [2049 * 1024 + 7, 5_000_000])
def test_fused_resampling_beyond_2048_tiles_on_device(gpu, n):
    """k_tile_prefix_big + the prefix-reading k_offspring_tile at n > 2^21 == gmx_weight_cdf + gmx_ancestors == the oracle"""
    parity.check_resample_beyond_2048_tiles(n=n)


def test_config4_resample_without_the_big_fused_path(gpu):
    """the CDF-array path that n > 2^21 took before (ticketed look-back scan + per-slot search) stays reachable and exact"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    from genjax_amd.inference.smc import ParticleCollection
    n = 3_000_000
    lw = np.random.default_rng(1).normal(0, 1.5, n).astype(np.float32)
    cdf, total, M, shift = O.weight_cdf_c(lw)
    cdf_d, tot, mx, sh = smc.weight_cdf(_dev(lw))
    anc = smc.ancestors_from_cdf(smc.SYSTEMATIC, G.key(5), cdf_d, tot)
    assert np.array_equal(anc.cpu().numpy(), O.ancestors_c(O.SYSTEMATIC, O.key(5), cdf))


@pytest.mark.parametrize("n", [257, 100_000])
def test_plates_match_oracle(gpu, n):
    parity.check_plates(n=n)


@pytest.mark.parametrize("n,world,kw", [
    # per-rank sizes are multiples of the 1024-particle CDF tile (shards start on a global tile boundary)
    (1024, 4, {}), (4096, 8, {"kind": 1, "seed": 3}), (1024, 3, {"skew": 2.0, "seed": 1}),
    (1024, 8, {"skew": -3.0, "seed": 2}), (64, 2, {"dead": True}), (100_352, 8, {"seed": 5}),
    (100_352, 8, {"seed": 6, "capacity": 12_500}), (250_880, 2, {"seed": 7, "skew": 0.5}),
    (101_376, 5, {"seed": 8}), (2048, 4, {"seed": 9, "kind": 1}),
    (2048, 4, {"seed": 12, "spike": 14.0}), (4096, 3, {"seed": 13, "spike": 30.0, "kind": 1}),   # wave-cooperative long runs
    # the two sides of the fill kernel's SMALL edge (world <= 8 and world * tiles <= 1024): 1024 table rows, then 1032
    (131_072, 8, {"seed": 31}), (132_096, 8, {"seed": 32}),
])
@pytest.mark.parametrize("fused", [False, True, "tiles", "stats"])
def test_global_resampling_routes_match_oracle(gpu, n, world, kw, fused):
    """gmx_shard_plan + gmx_shard_route, and their one-launch form gmx_shard_step, with every rank
    emulated on one GPU == the oracle's single-population resample (bit-exact ancestors => states)."""
    res = parity.check_shard_route(n, world, fused=fused, **kw)
    assert not res["overflow"]


def test_global_resampling_flags_overflow(gpu):
    assert parity.check_shard_route(1024, 3, skew=2.0, seed=1, capacity=5)["overflow"]
    assert parity.check_shard_route(1024, 3, skew=2.0, seed=1, capacity=5, fused="tiles")["overflow"]
    assert parity.check_shard_route(1024, 3, skew=2.0, seed=1, capacity=5, fused="stats")["overflow"]
    assert parity.check_shard_route(2048, 2, dead=True, fused="stats", capacity=100)["overflow"]


def test_fused_shard_step_heavy_tiles_and_ragged_shards(gpu):
    """gmx_shard_step_fused (the LDS-routed k_shard_step_fill): a tile that owns far more than 2048 slots (several fill
    passes, runs crossing rank boundaries), no mass at all, one rank, a shard that is not a multiple of the tile."""
    assert not parity.check_shard_route(4096, 4, seed=21, spike=40.0, fused="stats")["overflow"]
    assert not parity.check_shard_route(2048, 3, seed=22, spike=25.0, kind=O.STRATIFIED, fused="stats")["overflow"]
    assert not parity.check_shard_route(2048, 4, dead=True, fused="stats")["overflow"]
    assert not parity.check_shard_route(1000, 1, fused="stats", seed=23)["overflow"]
    assert not parity.check_shard_route(250_880, 4, seed=24, skew=1.0, fused="stats")["overflow"]      # 980 table rows: in registers
    assert not parity.check_shard_route(300_032, 4, seed=25, fused="stats")["overflow"]                # 1172 rows: the two-pass form
    assert not parity.check_shard_route(2048, 16, seed=26, skew=-1.0, fused="stats")["overflow"]       # 16 ranks: the two-pass form
    assert not parity.check_shard_route(125_952, 8, seed=27, fused="stats")["overflow"]                # 8 x 123: 1e6 split over a node


def test_sharded_sweep_world1_matches_oracle(gpu):
    """ShardedBootstrapSweep at world size 1 (collectives skipped) == BootstrapSweep oracle."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    n, T = 20_000, 5
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo).prepare(G.key(314159), torch.from_numpy(ys))
    sw.launch()
    oi, ost = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, ost, n, T, ys, O.key(314159))
    assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]])
    assert sw.totals.cpu().numpy().view(np.uint64).tolist() == [h["total"] for h in ref["hist"]]
    assert sw.log_ml() == ref["log_ml"]


def test_sharded_sweep_with_the_sorted_multinomial(gpu, tmp_path):
    """resample="multinomial_sorted" on the sharded router (gmx_shard_step_sorted: plan + route against
    the order-statistics table of all N slots) — world size 1 in this process, and two ranks (processes sharing the
    box's GPU, p2p communicator) — equal to the single-process oracle sweep."""
    import json
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.sharded import ShardedBootstrapSweep
    from tests.test_distributed_cpu import _launch

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    n, T = 300_000, 5
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    oi, ost = workloads.make_lgssm(O)
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, resample="multinomial_sorted").prepare(G.key(314159), torch.from_numpy(ys))
    sw.launch()
    ref = parity.oracle_bootstrap_sweep(oi, ost, n, T, ys, O.key(314159), kind=O.MULTINOMIAL_SORTED)
    assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]])
    assert sw.totals.cpu().numpy().view(np.uint64).tolist() == [h["total"] for h in ref["hist"]]
    assert sw.log_ml() == ref["log_ml"]
    n_total, T = 8192, 6
    out = str(tmp_path / "sorted_gpu")
    r = _launch(2, [out, str(n_total // 2), str(T)],
                extra_env={"GENMI_COMM": "p2p", "GENMI_COMM_TIMEOUT": "60",
                           "GENMI_TEST_OPTS": json.dumps({"on_gpu": 1, "resample": "multinomial_sorted"})})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    ys = workloads.lgssm_data(T)
    ref = parity.oracle_bootstrap_sweep(oi, ost, n_total, T, ys, O.key(314159), kind=O.MULTINOMIAL_SORTED)
    meta = json.load(open(out + ".json"))
    assert [int(t) for t in meta["totals"]] == [h["total"] for h in ref["hist"]] and meta["log_ml"] == ref["log_ml"]
    assert np.array_equal(np.load(out + ".npy"), ref["x"][ref["anc"]])


def test_sharded_sweep_over_the_peer_mapped_communicator_world1(gpu, monkeypatch):
    """GENMI_COMM=p2p on the device at world size 1: the collectives of every step go through gmx_p2p_exchange (put into
    the peer-mapped buffer — here the rank's own — flag, wait, device-side epoch), eagerly AND as a captured hipGraph
    replayed twice (the epoch must advance across replays); equal to the oracle.  Across GPUs: unmeasured."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.comm import P2PComm
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    monkeypatch.setenv("GENMI_COMM", "p2p")
    n, T = 300_000, 5
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, always_communicate=True).prepare(G.key(314159), torch.from_numpy(ys))
    assert isinstance(sw.cx, P2PComm) and sw.noise_ahead
    e0 = int(sw.cx.state[0].item())          # (the communicator's self-test made two exchanges)
    oi, ost = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, ost, n, T, ys, O.key(314159))
    sw.launch()
    assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]]) and sw.log_ml() == ref["log_ml"]
    sw.capture()
    for _ in range(2):
        sw.launch()
        sw.finish()
        assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]]) and sw.log_ml() == ref["log_ml"]
    # two exchanges per step; four sweeps: the eager one, capture()'s warm-up, two replays (the capture itself runs nothing)
    assert not sw.cx.failed() and int(sw.cx.state[0].item()) - e0 == 4 * 2 * T
    sw.close()


@pytest.mark.parametrize("n", [300_000, 20_000])
def test_sharded_sweep_over_the_fused_peer_exchange_world1(gpu, monkeypatch, n):
    """GENMI_COMM=peer on the device at world size 1 ("Fused peer exchange"): a step is the site program (whose epilogue
    would put its statistics to the other ranks) + gmx_shard_step_peer — NO collective launch; tags advance across
    sweeps through gmx_peer_bump inside the captured graph.  Eager and captured + replayed twice, specialised (n =
    300 000: the epilogue's statistics) and interpreted (n = 20 000: gmx_tile_stats + gmx_peer_put_stats); equal to the
    oracle.  With an MH move per step: two routed leaves through the same launch."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.comm import PeerComm
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    monkeypatch.setenv("GENMI_COMM", "peer")
    T = 5
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, always_communicate=True).prepare(G.key(314159), torch.from_numpy(ys))
    assert isinstance(sw.cx, PeerComm) and sw.peer_mode
    oi, ost = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, ost, n, T, ys, O.key(314159))
    sw.launch()
    assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]]) and sw.log_ml() == ref["log_ml"]
    sw.capture()
    for _ in range(2):
        sw.launch()
        sw.finish()
        assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]]) and sw.log_ml() == ref["log_ml"]
    # four sweeps: the eager one, capture()'s warm-up, two replays — T tags each on top of the initial 1
    assert int(sw.peer_tag.item()) == 1 + 4 * T and int(sw.peer_status.item()) == 0
    sw.close()
    # config 3: the MH move's second routed leaf through the same launch
    T = 4
    ys = workloads.nlssm_data(T)
    init, step = workloads.make_nlssm(G)
    req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, always_communicate=True, rejuvenate=req,
                               step_extra=lambda t: (float(t),)).prepare(G.key(7), torch.from_numpy(ys))
    assert sw.peer_mode and sw.peer_leaves == 2
    sw.launch()
    ref = parity.oracle_nlssm_mh_sweep(n, T, 7)
    assert np.array_equal(sw.state().cpu().numpy(), ref["resampled"])
    sw.close()


def test_conditional_smc_and_proposals(gpu):
    parity.check_csmc(k=10_001)


@pytest.mark.parametrize("n,specialize", [(3000, False), (200_000, False), (200_000, True), (1_000_000, True)])
def test_mixture_assignments_match_oracle(gpu, n, specialize):
    """BASELINE config 5: K = 64 cluster assignments, bit-exact against the oracle's materialised
    [n, K] categorical draw — up to the full N = 1e6."""
    parity.check_mixture_assignments(n=n, K=64, specialize=specialize)


@pytest.mark.parametrize("n", [257, 100_000])
def test_scan_matches_oracle(gpu, n):
    parity.check_scan(n=n, T=6)


@pytest.mark.parametrize("n", [257, 50_000])
def test_plate_edits_match_oracle(gpu, n):
    parity.check_plate_edits(n=n)


@pytest.mark.parametrize("n", [257, 100_000])
def test_hmc_reference_behaviour_and_oracle(gpu, n):
    parity.check_hmc(n=n)


@pytest.mark.parametrize("n,capture,specialize", [(3000, False, False), (100_000, True, True), (1_000_000, True, True)])
def test_nonlinear_ssm_mh_sweep_matches_oracle(gpu, n, capture, specialize):
    """BASELINE config 3 as one (captured) sweep with the fused MH move between resampling and extension: the
    one-stream form, and the noise-ahead form (proposal, accept and extension draws by background programs on a second
    stream — two of them per step, one per key)."""
    parity.check_nlssm_mh_sweep(n=n, T=5, capture=capture, specialize=specialize, noise_ahead=False)
    parity.check_nlssm_mh_sweep(n=n, T=13 if n <= 100_000 else 5, capture=capture, specialize=specialize, noise_ahead=True)


def test_config3_full_size_sweep_bit_exact(gpu):
    """BASELINE config 3 AT ITS FULL SIZE — 1e6 particles x 100 steps, one MH move per step — as `bench.py` runs it (one
    hipGraph, noise ahead, the move chained into the extension, one launch per step): final particles, log-weights, the
    last move's accept flags and the evidence against the oracle's run of the same sweep, COMMITTED as hashes + 300
    sampled entries (tests/golden/full_size.json, written by tests/golden/make_full_size.py: two minutes of numpy that
    no longer run inside the GPU suite; test_nonlinear_ssm_mh_sweep_matches_oracle holds 1e5 particles x 23 steps to
    the live oracle)."""
    res = parity.check_nlssm_mh_sweep(n=1_000_000, T=100, capture=True, specialize=True, noise_ahead=True, golden="config3")
    assert 0.5 < res["accept_rate"] <= 1.0


def test_dirichlet_matches_oracle_and_scipy(gpu):
    parity.check_dirichlet(n=50_000)


def test_interpreter_top_registers(gpu):
    """Raw programs through the C-ABI that write the highest registers (n_regs = 16 and 32): the
    interpreter's vector register file must hold them (regression: r15 of the 16-element file)."""
    import ctypes
    import struct
    from genjax_amd import _lib
    from genjax_amd.program import MAGIC, OPC, VERSION

    def f2u(x):
        return struct.unpack("<I", struct.pack("<f", x))[0]

    def ins(op, dst=0, a=0, b=0, imm=0):
        return [OPC[op] | (dst & 0xff) << 8 | (a & 0xff) << 16 | (b & 0xff) << 24, imm & 0xffffffff]
    for n_regs in (15, 16, 31, 32):
        top = n_regs - 1
        w = ins("CONST", 2, imm=f2u(3.5)) + ins("LGAMMA", top, 2) + ins("STOUT", 0, 0, top) + \
            ins("CONST", top, imm=f2u(2.25)) + ins("STOUT", 0, 1, top)
        blob = np.array([MAGIC, VERSION, len(w) // 2, n_regs, 0, 2, 0, 0, 0, 0] + w, dtype=np.uint32)
        h = ctypes.c_void_p()
        gpu.check(gpu.c.gmx_program_create(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), blob.size, h), "create")
        A = _lib.RunArgs()
        outs = [torch.full((70,), -7.0, device="cuda") for _ in range(2)]
        for k, o in enumerate(outs):
            A.out_d[k] = o.data_ptr()
        rc = gpu.c.gmx_program_run(h, 70, A, gpu.stream())
        if n_regs == 32:
            assert rc != 0                      # 32 live values: specialised kernels only
            continue
        gpu.check(rc, "run")
        torch.cuda.synchronize()
        assert abs(float(outs[0][69]) - 1.2009736) < 1e-6 and float(outs[1][0]) == 2.25, n_regs


def test_random_programs_interpreter_jit_and_host_agree(gpu):
    """Differential fuzz of the three executors of gmx_vm_step: random straight-line programs (register
    pressure 3..31, all float ops, keys, samplers) through (a) the gfx950 interpreter, (b) the hiprtc-
    specialised kernel, (c) the same template compiled for the host (tests/hostsim, loaded beside the
    HIP backend, never installed).  Every output must agree bit for bit."""
    import ctypes
    import tests.hostsim as hs
    from genjax_amd import _lib
    from genjax_amd.program import Graph, compile_graph
    host = _lib.Backend(ctypes.CDLL(hs.build()), torch.device("cpu"), uses_streams=False)
    rng = np.random.default_rng(7)
    n = 1000
    xin = rng.uniform(0.5, 2.0, (3, n)).astype(np.float32)
    unary = ["NEG", "ABS", "EXP", "LOG", "LOG1P", "SQRT", "SQUARE", "RECIP", "SIGMOID", "SIN", "COS", "TANH",
             "SOFTPLUS", "LGAMMA", "FLOOR"]
    binary = ["ADD", "SUB", "MUL", "DIV", "MIN", "MAX"]
    n_checked = 0
    for trial in range(24):
        g = Graph()
        live = [g.input("f32") for _ in range(3)]
        key = g.add("LDKEY", dtype="key")
        width = int(rng.integers(3, 29))
        for step in range(int(rng.integers(20, 90))):
            r = rng.random()
            if r < 0.45:
                a, b = (live[int(rng.integers(len(live)))] for _ in range(2))
                node = g.add(binary[int(rng.integers(len(binary)))], (a, b))
            elif r < 0.8:
                a = live[int(rng.integers(len(live)))]
                # keep magnitudes tame: unary ops act on a value squashed into (0.5, 1.5)
                sq = g.add("ADD", (g.add("SIGMOID", (a,)), g.const_f32(0.5)))
                node = g.add(unary[int(rng.integers(len(unary)))], (sq,))
            elif r < 0.9:
                k2 = g.add("KDERIVE", (key,), imm=int(rng.integers(1, 50)), dtype="key")
                node = g.add("S_NORMAL", (k2, live[0], g.const_f32(1.0)), imm=int(rng.integers(0, 4)))
            else:
                c = g.add("FLT", (live[int(rng.integers(len(live)))], live[int(rng.integers(len(live)))]), dtype="bool")
                node = g.add("SEL", (c, live[int(rng.integers(len(live)))], live[int(rng.integers(len(live)))]))
            live.append(node)
            if len(live) > width:
                live.pop(int(rng.integers(3, len(live))))
        acc = live[0]
        for v in live[1:]:                       # everything still live feeds the outputs
            acc = g.add("ADD", (g.add("MUL", (acc, g.const_f32(0.5))), v))
        for v in (acc, live[-1], live[len(live) // 2]):
            g.store(v)
        blob, const_pool = compile_graph(g)
        if int(blob[3]) > 31:
            continue
        results = []
        for be, dev, jit in ((gpu, "cuda", False), (gpu, "cuda", True), (host, "cpu", False)):
            h = ctypes.c_void_p()
            be.check(be.c.gmx_program_create(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), blob.size, h), "create")
            if jit:
                be.check(be.c.gmx_program_specialize(h), "specialize")
            A = _lib.RunArgs()
            ins_ = [torch.from_numpy(xin[k]).to(dev) for k in range(3)]
            outs = [torch.zeros((n,), dtype=torch.float32, device=dev) for _ in range(3)]
            for k in range(3):
                A.in_d[k], A.out_d[k] = ins_[k].data_ptr(), outs[k].data_ptr()
            A.key_mode, A.key0, A.key1 = _lib.KEY_SPLIT, 0, 42 + trial
            be.check(be.c.gmx_program_run(h, n, A, be.stream() if dev == "cuda" else None), "run")
            if dev == "cuda":
                torch.cuda.synchronize()
            results.append([o.cpu().numpy() for o in outs])
            be.c.gmx_program_destroy(h)
        for k in range(3):
            assert np.array_equal(results[0][k], results[2][k], equal_nan=True), (trial, k, int(blob[3]), "interp vs host")
            assert np.array_equal(results[1][k], results[2][k], equal_nan=True), (trial, k, int(blob[3]), "jit vs host")
        n_checked += 1
    assert n_checked >= 12


def test_sharded_mh_sweep_world1_matches_oracle(gpu):
    """ShardedBootstrapSweep(rejuvenate=...) at world size 1 on the GPU == the config-3 oracle."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    n, T = 30_000, 5
    ys = workloads.nlssm_data(T)
    init, step = workloads.make_nlssm(G)
    req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, rejuvenate=req,
                               step_extra=lambda t: (float(t),)).prepare(G.key(7), torch.from_numpy(ys))
    sw.launch()
    ref = parity.oracle_nlssm_mh_sweep(n, T, 7)
    assert np.array_equal(sw.state().cpu().numpy(), ref["resampled"])
    assert abs(sw.log_ml() - sum(ref["terms"])) < 1e-9 * max(1.0, abs(sum(ref["terms"])))


def test_sharded_importancek_global_resample_world1(gpu):
    """sharded_importance_resample (config 4's multi-GPU form) at world size 1 == the oracle."""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, numpy as jnp
    from genjax_amd.inference.sharded import sharded_importance_resample

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    sig = np.array(parity.SCHOOL_SIGMA, np.float32)

    @G.gen
    def schools():
        mu = G.normal(0.0, 5.0) @ "mu"
        log_tau = G.normal(0.0, 1.0) @ "log_tau"
        theta = G.normal(mu * jnp.ones(8), jnp.exp(log_tau) * jnp.ones(8)) @ "theta"
        _ = G.normal(theta, jnp.array(parity.SCHOOL_SIGMA)) @ "y"
        return theta

    @O.gen
    def o_schools():
        mu = O.normal(0.0, 5.0) @ "mu"
        log_tau = O.normal(0.0, 1.0) @ "log_tau"
        theta = O.normal(mu[..., None] * np.ones(8, np.float32), O.exp(log_tau)[..., None] * np.ones(8, np.float32)) @ "theta"
        _ = O.normal(theta, sig) @ "y"
        return theta
    k = 100_000
    coll, lw = sharded_importance_resample(G.Target(schools, (), C["y"].set(parity.SCHOOL_Y)), k, G.key(2), _Solo)
    oc = O.ImportanceK(O.Target(o_schools, (), O.C.d({"y": parity.SCHOOL_Y})), k).run_smc(O.key(2))
    assert np.array_equal(lw.cpu().numpy(), oc.get_log_weights())
    cdf, total, M, shift = O.weight_cdf(oc.get_log_weights())
    anc = O.ancestors_c(O.SYSTEMATIC, O.split(O.key(2))[0], cdf)
    assert np.array_equal(coll.get_particles().get_choices()["theta"].cpu().numpy(),
                          oc.get_particles().get_choices()["theta"][anc])


@pytest.mark.parametrize("n,capture,specialize", [(3000, False, False), (300_000, True, True)])
def test_vector_state_sweep_matches_oracle(gpu, n, capture, specialize):
    """BootstrapSweep with a 2-D state (position, velocity), stored [2, n] struct-of-arrays."""
    parity.check_vector_state_sweep(n=n, T=5, capture=capture, specialize=specialize)


def test_full_size_sweep_properties(gpu):
    """BASELINE config 2 at full size (1e6 particles, T = 100): size-independent
    properties — sorted ancestors, determinism, and log-ML within Monte-Carlo
    error of the exact Kalman answer."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    n, T = 1_000_000, 100
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T).prepare(G.key(314159), torch.from_numpy(ys)).capture()
    sw.launch()
    a = sw.log_ml()
    anc1 = sw.anc.clone()
    sw.launch()
    assert sw.log_ml() == a and torch.equal(anc1, sw.anc)          # idempotent / deterministic
    assert bool(torch.all(anc1[1:] >= anc1[:-1]))                  # systematic => sorted
    assert int(sw.ws.view(torch.int32)[1].item()) == 0             # scan never hit its spin bound
    kal = workloads.kalman_log_ml(ys)
    assert abs(a - kal) < 0.05, (a, kal)


def test_full_size_sweep_bit_exact_vs_c_oracle(gpu):
    """BASELINE config 2 at FULL size (1e6 particles x 100 steps), the sweep bench.py times (noise-ahead form),
    against oracle/orc_sweep.c — the OpenMP statement of the oracle's sweep, itself held to the numpy oracle in
    tests/test_oracle_pins.py::test_c_sweep_equals_numpy_sweep: final particles, log-weights, ancestors, and every
    step's integer total and maximum, bit for bit."""
    import ctypes
    import os
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    n, T, seed = 1_000_000, 100, 314159
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T).prepare(G.key(seed), torch.from_numpy(ys)).capture()
    assert sw.noise_ahead
    sw.launch()
    x, lw, anc = [v.cpu().numpy() for v in sw.state()]
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_build", "liborc_sweep.so")
    lib = ctypes.CDLL(so)
    shift = O.cdf_shift(n)
    f32, u64, i32 = np.float32, np.uint64, np.int32
    ox, ox2, olw = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    ocdf, oanc = np.zeros(n, u64), np.zeros(n, i32)
    omax, otot = np.zeros(T, f32), np.zeros(T, u64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.orc_lgssm_sweep(ctypes.c_int64(n), ctypes.c_int64(T), P(ys), ctypes.c_uint32(0), ctypes.c_uint32(seed),
                             ctypes.c_float(0.9), ctypes.c_float(0.5), ctypes.c_float(1.0), ctypes.c_float(1.0),
                             ctypes.c_int(shift), P(ox), P(ox2), P(olw), P(ocdf), P(oanc), P(omax), P(otot))
    assert rc == 0
    assert np.array_equal(sw.totals.cpu().numpy().view(np.uint64), otot)
    assert np.array_equal(sw.maxs.cpu().numpy().view(np.uint32), omax.view(np.uint32))
    assert np.array_equal(x.view(np.uint32), ox.view(np.uint32))
    assert np.array_equal(lw.view(np.uint32), olw.view(np.uint32))
    assert np.array_equal(anc, oanc)


def test_config2_sizes_log_ml_bit_exact(gpu):
    """bench.py's `other_configs.config2_sizes` (BASELINE config 2 at 1.25e5 ... 8e6 particles x 100 steps; one launch
    per step up to 2^20 particles, two beyond): every step's integer total and maximum — the terms of the log-ML — and
    the last ancestors against oracle/orc_sweep.c, bit for bit, at every size (run live up to 1e6; its committed outputs
    — tests/golden/full_size.json — at 2e6 and 8e6, where one core needs 20 s)"""
    import ctypes
    import os
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    T, seed = 100, 314159
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_build", "liborc_sweep.so")
    lib = ctypes.CDLL(so)
    f32, u64, i32 = np.float32, np.uint64, np.int32
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for n in bench.CONFIG2_SIZES:
        sw = BootstrapSweep(init, step, n, T).prepare(G.key(seed), torch.from_numpy(ys)).capture()
        sw.launch()
        lml = sw.log_ml()
        _, _, anc = [v.cpu().numpy() for v in sw.state()]
        anc = anc & 0xffffff if sw.fuse else anc          # (the one-launch step leaves TAGGED ancestor words)
        if n > 1_000_000:       # the two sizes past one launch per step: the committed oracle outputs of that size
            g = parity.load_golden("config2_sizes")[str(n)]       # (tests/golden/make_full_size.py config2_sizes)
            assert (g["T"], g["seed"]) == (T, seed)
            assert [int(v) for v in sw.totals.cpu().numpy().view(np.uint64)] == g["totals"], n
            assert [int(v) for v in sw.maxs.cpu().numpy().view(np.uint32)] == g["maxs_bits"], n
            assert parity.equals_golden(anc.astype(np.int32), g["anc"], g["index"]), n
            assert lml == float.fromhex(g["log_ml"]), (n, lml)
            assert sw.fuse          # ONE launch per step past 2^20 particles too: the looped resample-first kernel
            del sw
            continue
        shift = O.cdf_shift(n)
        ox, ox2, olw = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
        ocdf, oanc = np.zeros(n, u64), np.zeros(n, i32)
        omax, otot = np.zeros(T, f32), np.zeros(T, u64)
        rc = lib.orc_lgssm_sweep(ctypes.c_int64(n), ctypes.c_int64(T), P(ys), ctypes.c_uint32(0), ctypes.c_uint32(seed),
                                 ctypes.c_float(0.9), ctypes.c_float(0.5), ctypes.c_float(1.0), ctypes.c_float(1.0),
                                 ctypes.c_int(shift), P(ox), P(ox2), P(olw), P(ocdf), P(oanc), P(omax), P(otot))
        assert rc == 0
        assert np.array_equal(sw.totals.cpu().numpy().view(np.uint64), otot), n
        assert np.array_equal(sw.maxs.cpu().numpy().view(np.uint32), omax.view(np.uint32)), n
        assert np.array_equal(anc, oanc), n
        olml = float(np.sum(np.array([O.cdf_reference(v) for v in omax], np.float64) + np.log(otot.astype(np.float64))
                            - shift * np.log(2.0) - np.log(n)))
        assert lml == olml, (n, lml, olml)
        assert (n <= 1 << 20) == bool(sw.fuse), n
        del sw


def test_empty_batch_on_device(gpu):
    """zero particles: no launch, empty results (a 0-size device tensor has a null pointer)"""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C

    @G.gen
    def m():
        x = G.normal(0.0, 1.0) @ "x"
        _ = G.normal(x, 1.0) @ "y"
        return x
    ks = G.split(G.key(0), 0)
    tr, w = m.importance(ks, C.kw(y=1.0), ())
    assert w.shape == (0,) and tr.get_score().shape == (0,) and w.is_cuda
    assert m.simulate(ks, ()).get_retval().shape == (0,)


def test_sharded_vector_state_world1_matches_oracle(gpu):
    """ShardedBootstrapSweep with a 2-vector state at world size 1 on the device: each component is a routed
    leaf written through a strided [D, n] window of the [D, n + W*C] extended state."""
    import genjax_amd as G
    from genjax_amd import numpy as jnp
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    n, T = 50_000, 5
    init, step = parity.make_tracker(G, lambda a, b: jnp.stack([a, b]))
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo).prepare(G.key(5), torch.from_numpy(parity.tracker_data(T)))
    sw.launch()
    ref = parity.oracle_tracker_sweep(n, T, 5)
    x = sw.state().cpu().numpy()
    assert x.shape == (n, 2) and np.array_equal(x, ref["x"][ref["anc"]])
    assert sw.log_ml() == ref["log_ml"]


def test_specialised_code_object_cache(gpu, tmp_path, monkeypatch):
    """GENMI_JIT_CACHE: the first specialisation writes <hash>.co, a second program with the same
    instruction stream loads it instead of calling hiprtc, a damaged entry is recompiled; results identical."""
    import time
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    monkeypatch.setenv("GENMI_JIT_CACHE", str(tmp_path))

    def run():
        @G.gen
        def m(a):
            x = G.normal(a, 1.25) @ "x"
            _ = G.normal(x * x, 0.5) @ "y"
            return x
        from genjax_amd.static import MinimalGenerate
        from genjax_amd.random import lazy_split
        n = 4096
        p = MinimalGenerate(m, (0.75,), C.kw(y=1.0), (n,))
        t0 = time.perf_counter()
        assert p.comp.specialize()
        dt = time.perf_counter() - t0
        outs = p.comp.run(p.leaves((0.75,), C.kw(y=1.0)), (n,), lazy_split(G.key(3), n))
        return dt, [o.cpu().numpy() for o in outs]
    t_cold, a = run()
    files = list(tmp_path.glob("*.co"))
    assert len(files) == 1 and files[0].stat().st_size > 1000
    t_warm, b = run()
    assert t_warm < 0.5 * t_cold, (t_cold, t_warm)
    files[0].write_bytes(b"not a code object")
    _, c = run()
    assert files[0].stat().st_size > 1000          # rewritten after the recompile
    for u, v, w in zip(a, b, c):
        assert np.array_equal(u, v) and np.array_equal(u, w)


def test_sweep_with_separate_tile_stats_launch(gpu):
    """an interpreted site program does not write the CDF tile statistics; gmx_resample's own k_tile_stats pass
    does.  Same sweep, bit for bit (the default path lets the specialised program write them)."""
    res = parity.check_lgssm_sweep(n=50_000, T=6, capture=True, specialize=False)
    assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"] and res["lw_max_abs_diff"] == 0.0
    assert res["log_ml"] == res["log_ml_oracle"]


def test_long_scan_config2_as_one_generative_function(gpu):
    """`step.scan(n=100)` on config 2's model, importance for 1e5 particles as ONE generative
    function / one launch (interpreter), bit-exact vs the oracle; the same through the hiprtc-specialised kernel
    (n >= 2^18 particles), and the importance-sampling evidence of a short chain against the Kalman filter."""
    parity.check_scan_long(n=40_000, T=100)
    parity.check_scan_long(n=270_000, T=24)                  # >= 2^18: the specialised kernel (GMX_JIT_LOOP)
    r = parity.check_scan_long(n=400_000, T=17)
    assert abs(r["log_ml_is"] - r["kalman"]) < 0.25, r         # prior-proposal IS over 18 steps: MC error ~0.1


def test_runtime_indexed_addresses(gpu):
    """`C["schools", idx, "y"].set(v)` with one index per particle (ref choice_map.py:1453-1531)"""
    parity.check_runtime_indexed(n=257)
    parity.check_runtime_indexed(n=100_000, seed=3)


def test_conditional_smc_under_a_batch_of_keys(gpu):
    """`vmap(alg.estimate_logpdf)` over 1 000 keys as ONE launch set over [keys, K] (retained
    particle in slot K-1 of every row), incl. ChangeTarget.run_csmc, the reciprocal normalising constant and a nested
    Marginal(algorithm=...); equal to the per-key runs."""
    parity.check_batched_csmc(k=33, B=1000)


def test_plate_on_the_launch_axis_and_config5_through_the_gfi(gpu):
    """VERDICT r3 item 2 (ref vmap.py:180-218 is jax.vmap): a 1e6-element plate under ONE key runs with its elements on
    the launch axis — simulate / importance / assess / Update bit-exact vs the oracle's Vmap (choices, per-element
    scores AND the fixed-tree plate sums), within 1.5x of the same model launched with the datapoints as the particle
    batch; BASELINE config 5 written as `generate_datapoint.repeat(n = 1e6)` + gibbs.enumerative_gibbs on the plate's
    trace: bit-exact assignments, within 1.5x of the bare gibbs_categorical launch."""
    parity.check_plate_on_the_launch_axis(n=10_000)
    t_plate, t_batch = parity.check_plate_on_the_launch_axis(n=1_000_000, seed=4, compare_batch_form=True)
    assert t_plate <= 1.5 * t_batch + 2e-4, (t_plate, t_batch)
    parity.check_mixture_gibbs_through_the_plate(n=20_000)
    t_gfi, t_bare = parity.check_mixture_gibbs_through_the_plate(n=1_000_000, timing=True)
    assert t_gfi <= 1.5 * t_bare + 2e-4, (t_gfi, t_bare)


def test_large_plates_as_a_counted_loop(gpu):
    """`Vmap` plates of any size (ref vmap.py:180-218) as OP_LOOP with split(key, n)[j] keys —
    a 4096-element plate x 1e3 particles (interpreter) and a 40-element plate x 2.7e5 particles (specialised kernel),
    simulate / importance / assess / Update / IndexRequest, bit-exact vs the oracle."""
    parity.check_plates_long(n=300, P=40)
    parity.check_plates_long(n=270_000, P=24, seed=3)
    parity.check_plates_long(n=1000, P=4096, seed=5, light=True)        # simulate / importance / assess / single-element constraints
    parity.check_plates_long(n=100, P=4096, seed=6)


def test_index_request_on_a_long_plate_is_o1(gpu):
    """VERDICT r3 item 6 (ref vmap.py:277-332 `edit_index`: dynamic_slice / edit / dynamic_update_slice): one element of
    a 4096-element plate x 1e5 particles is edited at least 20x faster than the counted-loop form that re-scores all
    4096 (static.run_edit), with the same result; chains of edits, Python-int and per-particle index, one and two
    plate levels, bit-exact vs the oracle."""
    import time
    import genjax_amd as G
    from genjax_amd import Diff, IndexRequest, Regenerate, SelectionBuilder as S, static
    parity.check_index_request_o1(n=100, P=4096, seed=5, edits=7)
    parity.check_index_request_o1(n=270_000, P=24, seed=6, edits=6, nested=False)
    parity.check_index_request_o1(n=300, P=40, seed=7, edits=40, nested=False)        # (longer than PATCH_DEPTH_MAX: folded)
    n, P = 100_000, 4096
    school = parity._school(G)
    v = school.vmap(in_axes=(None, None, 0))
    args = (1.0, 2.0, torch.linspace(1.0, 3.0, P).cuda())
    tr = v.simulate(G.split(G.key(1), n), args)
    keys = G.split(G.key(2), n)
    idx = torch.randint(0, P, (n,), dtype=torch.int32).cuda()

    def timed(fn, reps=3):
        out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / reps
    for ix in (7, idx):
        req = IndexRequest(ix, Regenerate(S["theta"]))
        (new, w, _, _), t_o1 = timed(lambda: req.edit(keys, tr, Diff.no_change(args)))
        (ref, w_ref, _, _), t_loop = timed(lambda: static.run_edit(v, keys, tr, req, Diff.no_change(args)))
        assert torch.equal(w, w_ref) and torch.equal(new.get_choices()["theta"], ref.get_choices()["theta"])
        assert torch.equal(new.get_score(), ref.get_score())
        assert 20.0 * t_o1 <= t_loop, (t_o1, t_loop)


def test_one_trace_of_a_model_with_large_plates_runs_site_by_site(gpu):
    """4_index_request.ipynb c3-c12 on the device: ONE trace of a model with three 1e6-element plates (two of bare
    distributions, one of a `@gen` element inside a nested call) and an observation of their sums — site by site, plates
    on the launch axis — bit-exact vs the oracle; `StaticRequest({"a": IndexRequest(3, Update(42.0))})` touches one
    element and is several times cheaper than updating the whole plate."""
    parity.check_one_trace_with_large_plates(n=20_000)
    t_index, t_update = parity.check_one_trace_with_large_plates(n=1_000_000, seed=9, timing=True)
    assert t_index < t_update, (t_index, t_update)
    parity.check_one_trace_with_large_vector_sites(n=5000)
    parity.check_one_trace_with_large_vector_sites(n=100_000, K=64, seed=2)      # the mixture model's data site
    parity.check_mixture_notebook_model(n=5000, k=40)                        # the notebook's own sizes
    parity.check_mixture_notebook_model(n=100_000, k=64, seed=3)            # ... and BASELINE config 5's K (its N: test_mixture_assignments_match_oracle)


def test_large_plate_of_a_small_particle_batch_is_deferred(gpu):
    """50 particles over a model with 1e5 datapoints (the shape of `ImportanceK(target, 50)` on a data-heavy model): in
    the loop form 50 lanes walk 1e5 elements each; deferred, the plate is one launch over 5e6 elements — the same bits,
    and at least 5x faster on the importance call."""
    parity.check_deferred_plate(B=64, n=4096)
    t_def, t_loop = parity.check_deferred_plate(B=50, n=100_000, seed=7, timing=True)
    assert 5.0 * t_def <= t_loop, (t_def, t_loop)


def test_scan_carries_that_forward_each_other(gpu):
    """`(xn, a)` from `(a, b)` and `(b, a)` carries through the counted loop — interpreter and the
    specialised kernel (n >= 2^18) — bit-exact vs the oracle for simulate / generate / Update / Regenerate."""
    parity.check_scan_carry_forms(n=1000)
    parity.check_scan_carry_forms(n=270_000, Ts=(17,))


def test_indexed_and_masked_constraints(gpu):
    """a plate constrained on a subset of its indices (Indexed, ref choice_map.py:1453-1531) and
    Mask(value, flag) constraints with one flag per particle (ref distribution.py:129-142, 189-224): OP_SEL between
    the importance and simulate results inside the site program; bit-exact vs the oracle's restatement."""
    parity.check_masked_constraints(n=257)
    parity.check_masked_constraints(n=10_000, seed=3)


@pytest.mark.parametrize("n,T,capture", [(4096, 5, False), (100_000, 23, True), (100_003, 12, True)])
def test_noise_ahead_sweep_matches_oracle(gpu, n, T, capture):
    """BootstrapSweep's two-stream form (the steps' normal draws by background programs on a second stream, a group
    of steps ahead) and its one-stream form, both against the oracle, bit for bit: eager and captured,
    T not a multiple of the noise group, ragged last tile."""
    for na in (True, False):
        res = parity.check_lgssm_sweep(n=n, T=T, capture=capture, specialize=True, noise_ahead=na)
        assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"] and res["lw_max_abs_diff"] == 0.0
        assert abs(res["log_ml"] - res["log_ml_oracle"]) < 1e-11


def test_noise_ahead_with_stratified_resampling_and_env_switch(gpu, monkeypatch):
    """the two-stream form with the stratified resampler (one Threefry block per slot edge in the chain's resampler),
    and GENMI_NOISE_AHEAD=0 as the default's off switch"""
    import genjax_amd as G
    for na in (True, False):    # the per-slot uniforms from the background stream (gmx_slot_uniforms), or drawn in the resampler
        res = parity.check_lgssm_sweep(n=50_000, T=23, capture=True, specialize=True, resample="stratified", noise_ahead=na)
        assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"] and res["lw_max_abs_diff"] == 0.0
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    ys = workloads.lgssm_data(3)
    init, step = workloads.make_lgssm(G)
    assert BootstrapSweep(init, step, 4096, 3).prepare(G.key(1), torch.from_numpy(ys)).noise_ahead
    monkeypatch.setenv("GENMI_NOISE_AHEAD", "0")
    assert not BootstrapSweep(init, step, 4096, 3).prepare(G.key(1), torch.from_numpy(ys)).noise_ahead


def test_noise_ahead_full_size_equals_one_stream(gpu):
    """BASELINE config 2 at full size (1e6 particles x 100 steps): the two forms leave the same particles,
    log-weights, ancestors and integer totals; replaying the captured two-stream graph is deterministic."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    n, T = 1_000_000, 100
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    got = []
    for na in (False, True):
        sw = BootstrapSweep(init, step, n, T, noise_ahead=na).prepare(G.key(314159), torch.from_numpy(ys))
        assert sw.noise_ahead == na
        sw.capture()
        for _ in range(3 if na else 1):
            sw.launch()
        got.append([v.clone() for v in sw.state()] + [sw.totals.clone(), sw.maxs.clone()])
        if na:
            sw.launch()
            again = [v.clone() for v in sw.state()] + [sw.totals.clone(), sw.maxs.clone()]
            assert all(torch.equal(a, b) for a, b in zip(got[-1], again))
    assert all(torch.equal(a, b) for a, b in zip(*got))


def test_noise_ahead_beyond_the_fused_resampler(gpu):
    """n > 2^21: the chain resamples with gmx_weight_cdf + gmx_ancestors (two launches) instead of the tile form;
    the two-stream sweep still equals the one-stream one, multinomial resampling included."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    for n, T, kind in ((2_500_000, 3, "systematic"), (300_000, 4, "multinomial")):
        ys = workloads.lgssm_data(T)
        init, step = workloads.make_lgssm(G)
        got = []
        for na in (False, True):
            sw = BootstrapSweep(init, step, n, T, resample=kind, noise_ahead=na).prepare(G.key(5), torch.from_numpy(ys))
            assert sw.noise_ahead == na and (sw.fused == (kind == "systematic" and n <= 2 ** 21))
            sw.capture()
            sw.launch()
            got.append([v.clone() for v in sw.state()] + [sw.totals.clone()])
        assert all(torch.equal(a, b) for a, b in zip(*got))


def test_tuple_state_sweep_three_site_step_model(gpu):
    """BootstrapSweep over a step model with three latent sites and a tuple state, 1e5 particles,
    captured + specialised, bit-exact vs the oracle"""
    parity.check_tuple_state_sweep(n=100_000, T=5, capture=True, specialize=True, noise_ahead=False)
    parity.check_tuple_state_sweep(n=100_000, T=5, capture=True, specialize=True, noise_ahead=True)   # three draws per step
    parity.check_tuple_state_sweep(n=3001, T=4)


@pytest.mark.parametrize("kind", ["systematic", "multinomial_sorted"])
def test_functional_loop_captured_equals_eager(gpu, kind):
    """smc.capture: resample -> rejuvenate -> extend written with the functional API, captured once into a hipGraph;
    the replayed particles, ancestors and accept bits equal the eager loop's (and the step programs leave the
    resampler's tile statistics themselves once they run specialised: no separate pass over the log-weights)."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    n, T = 300_000, 4
    ys = workloads.nlssm_data(T)
    init, step = workloads.make_nlssm(G)
    req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})

    def sweep(key):
        ancs = []
        for t in range(T):
            kp, kr, km = G.split(G.fold_in(key, t), 3)
            obs = G.ChoiceMap.kw(y=float(ys[t]))
            if t == 0:
                coll = smc.ImportanceK(G.Target(init, (), obs), k_particles=n).run_smc(kp)
            else:
                coll = smc.resample(kr, coll, kind)
                ancs.append(coll.ancestors)
                coll = smc.rejuvenate(km, coll, req)
                coll = smc.extend(kp, coll, step, lambda tr_: (tr_.get_retval(), float(t)), obs)
        return coll, ancs
    ref, ref_anc = sweep(G.key(11))
    ref_x = ref.get_particles().get_retval().clone()
    ref_lw = ref.get_log_weights().clone()
    ref_anc = [a.clone() for a in ref_anc]
    for na in (False, True):        # noise_ahead: the loop's draws by background programs on a second stream
        cap = smc.capture(sweep, G.key(11), noise_ahead=na)
        assert (cap.noise is not None and cap.noise.demand > 0) == na
        for _ in range(2):
            coll, ancs = cap.replay()
            torch.cuda.synchronize()
            assert torch.equal(coll.get_particles().get_retval(), ref_x)
            assert torch.equal(coll.get_log_weights(), ref_lw)
            for a, b in zip(ancs, ref_anc):
                assert torch.equal(a, b)
    # the graph's kernel nodes point into the site programs' code — the captured loop itself keeps the
    # programs it launched, so dropping every program cache (public API) and collecting must not break a replay
    import gc
    assert len(cap.programs) >= 3
    G.clear_caches()
    gc.collect()
    coll, ancs = cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(coll.get_particles().get_retval(), ref_x) and torch.equal(coll.get_log_weights(), ref_lw)
    # against the oracle's statement of the same loop (ancestors, states, weights bit-exact)
    parity.check_nlssm_mh(n=2000, T=4)


def test_captured_loop_without_mh_hoists_the_extension_draws(gpu):
    """smc.capture(noise_ahead=True) under "auto": a loop with no MH move hands over the draws of its extend /
    ImportanceK launches instead; replays equal the eager loop bit for bit"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    n, T = 300_000, 5
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)

    def sweep(key):
        for t in range(T):
            kp, kr, _ = G.split(G.fold_in(key, t), 3)
            obs = G.ChoiceMap.kw(y=float(ys[t]))
            if t == 0:
                coll = smc.ImportanceK(G.Target(init, (), obs), k_particles=n).run_smc(kp)
            else:
                coll = smc.resample(kr, coll, "systematic")
                coll = smc.extend(kp, coll, step, lambda tr_: (tr_.get_retval(),), obs)
        return coll
    ref = sweep(G.key(3))
    ref_x, ref_lw = ref.get_particles().get_retval().clone(), ref.get_log_weights().clone()
    cap = smc.capture(sweep, G.key(3), noise_ahead=True)
    assert cap.noise.kinds == ("generate", "simulate") and len(cap.noise.plan) == T
    for _ in range(2):
        coll = cap.replay()
        torch.cuda.synchronize()
        assert torch.equal(coll.get_particles().get_retval(), ref_x) and torch.equal(coll.get_log_weights(), ref_lw)


@pytest.mark.parametrize("kind", ["stratified", "multinomial", "multinomial_tiled", "multinomial_sorted"])
def test_captured_functional_loop_with_every_resampling_kind(gpu, kind):
    """`smc.resample(kind=...)` inside a captured Python loop (the tile / sorted multinomials build their count buffers
    and order-statistics table inside the capture): replays equal the eager loop bit for bit (the eager calls are held to
    the oracle kind by kind in tests/test_host_logic.py::TestSMCMoves::test_resample_extend_api)"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    n, T = 50_000, 4
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)

    def sweep(key):
        for t in range(T):
            kp, kr, _ = G.split(G.fold_in(key, t), 3)
            obs = G.ChoiceMap.kw(y=float(ys[t]))
            if t == 0:
                coll = smc.ImportanceK(G.Target(init, (), obs), k_particles=n).run_smc(kp)
            else:
                coll = smc.resample(kr, coll, kind)
                coll = smc.extend(kp, coll, step, lambda tr_: (tr_.get_retval(),), obs)
        return coll
    ref = sweep(G.key(3))
    ref_x, ref_lw = ref.get_particles().get_retval().clone(), ref.get_log_weights().clone()
    cap = smc.capture(sweep, G.key(3))
    for _ in range(2):
        coll = cap.replay()
        torch.cuda.synchronize()
        assert torch.equal(coll.get_particles().get_retval(), ref_x) and torch.equal(coll.get_log_weights(), ref_lw)


def test_captured_loop_noise_ahead_edges(gpu, monkeypatch):
    """smc.capture(noise_ahead=True): launches below 2^18 particles keep their draws (empty plan, same results); an
    arena bound of 0 MB falls back to the one-stream capture."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    ys = workloads.lgssm_data(3)
    init, step = workloads.make_lgssm(G)

    def make(n):
        def sweep(key):
            for t in range(3):
                kp, kr, _ = G.split(G.fold_in(key, t), 3)
                obs = G.ChoiceMap.kw(y=float(ys[t]))
                if t == 0:
                    coll = smc.ImportanceK(G.Target(init, (), obs), k_particles=n).run_smc(kp)
                else:
                    coll = smc.extend(kp, smc.resample(kr, coll, "systematic"), step, lambda tr_: (tr_.get_retval(),), obs)
            return coll
        return sweep
    small = make(50_000)
    ref = small(G.key(9)).get_particles().get_retval().clone()
    cap = smc.capture(small, G.key(9), noise_ahead=True)
    assert cap.noise is not None and cap.noise.plan == []
    assert torch.equal(cap.replay().get_particles().get_retval(), ref)
    big = make(300_000)
    ref = big(G.key(9)).get_particles().get_retval().clone()
    monkeypatch.setattr(smc.CapturedLoop, "NOISE_ARENA_MB", 0)
    cap = smc.capture(big, G.key(9), noise_ahead=True)
    assert cap.noise is None
    assert torch.equal(cap.replay().get_particles().get_retval(), ref)


def test_tile_stats_from_the_site_program(gpu):
    """the specialised program's epilogue writes the same (m_b, A_b) as gmx_tile_stats, ragged last tile included"""
    import genjax_amd as G
    from genjax_amd import _lib, workloads
    from genjax_amd.inference.smc import BootstrapSweep
    be = _lib.get()
    n, T = 100_003, 3
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T).prepare(G.key(1), torch.from_numpy(workloads.lgssm_data(T)))
    assert sw.tile_stats
    sw.launch()
    torch.cuda.synchronize()
    tiles = (n + 1023) // 1024
    tmax = torch.zeros(tiles, dtype=torch.float32, device="cuda")
    agg = torch.zeros(tiles, dtype=torch.int64, device="cuda")
    be.check(be.c.gmx_tile_stats(be.ptr(sw.lw), n, sw.shift, be.ptr(tmax), be.ptr(agg), be.stream()), "gmx_tile_stats")
    assert torch.equal(tmax, sw.partials[0, :tiles]) and torch.equal(agg, sw.tile_agg)
    lw = sw.lw.cpu().numpy()
    for b in (0, tiles - 1):
        x = lw[b * 1024:(b + 1) * 1024]
        q = np.zeros(x.size, np.uint64)
        ref = O.tile_ref(O.tile_exp(x.max()))          # block floating point: weights relative to ceil(max / ln 2) * ln 2
        O.lib().orc_weight_fixed(O.I64(x.size), O._p(x), O.ctypes.c_float(ref), O.ctypes.c_int(sw.shift), O._p(q))
        assert int(q.sum()) == int(agg[b].item()) and float(tmax[b].item()) == float(x.max())


@pytest.mark.parametrize("n", [100_003, 1_000_000, 2_000_000])
def test_tile_prefixes_equal_the_statistics_pass(gpu, n):
    """gmx_tile_prefix (one workgroup: M, K, the exclusive tile prefixes, the total) equals the host's integers, and
    gmx_resample_tiles_p reading those prefixes gives the ancestors of gmx_resample_tiles, whose workgroups each reduce
    the whole statistics table (PER = 1 / 4 / 8 rows of the table per thread)."""
    import genjax_amd as G
    from ctypes import c_uint32
    from genjax_amd import _lib, workloads
    from genjax_amd.inference.smc import BootstrapSweep
    be = _lib.get()
    T = 3
    init, step = workloads.make_lgssm(G)
    ys = torch.from_numpy(workloads.lgssm_data(T))
    sw = BootstrapSweep(init, step, n, T).prepare(G.key(2), ys)
    sw.launch()
    torch.cuda.synchronize()
    tiles = (n + 1023) // 1024
    pref_t = torch.zeros((int(be.c.gmx_tile_prefix_words(n)),), dtype=torch.int64, device=be.device)
    be.check(be.c.gmx_tile_prefix(be.ptr(sw.partials), be.ptr(sw.tile_agg), n, be.ptr(pref_t), be.stream()), "gmx_tile_prefix")
    pref = pref_t.cpu().numpy().view(np.uint64)
    tm = sw.partials[0, :tiles].cpu().numpy()
    agg = sw.tile_agg.cpu().numpy().view(np.uint64)
    M = tm.max()
    K = O.tile_exp(M)
    G_ = [int(a) >> min(K - O.tile_exp(m), 63) for a, m in zip(agg, tm)]
    assert [int(v) for v in pref[:tiles]] == list(np.cumsum([0] + G_[:-1], dtype=object))
    assert int(pref[tiles]) == sum(G_) == int(sw.totals[T - 1].item()) & (2 ** 64 - 1)
    assert int(pref[tiles + 1]) & 0xFFFFFFFF == int(np.float32(M).view(np.uint32)) and (int(pref[tiles + 1]) >> 32) == K & 0xFFFFFFFF
    kh = sw.step_keys[T - 1][1].host()
    kk = (c_uint32 * 2)(int(kh[0]), int(kh[1]))
    anc = torch.zeros_like(sw.anc)
    mx, tot = torch.zeros_like(sw.maxs[:1]), torch.zeros_like(sw.totals[:1])
    be.check(be.c.gmx_resample_tiles_p(sw.kind, kk, be.ptr(sw.lw), n, sw.shift, be.ptr(sw.partials), be.ptr(pref_t), be.ptr(mx),
                                       be.ptr(tot), be.ptr(anc), be.stream()), "gmx_resample_tiles_p")
    assert torch.equal(anc, sw.anc) and torch.equal(tot, sw.totals[T - 1:]) and torch.equal(mx, sw.maxs[T - 1:])


def test_tile_stats_are_dropped_when_the_weights_change_in_place(gpu):
    """`extend` leaves the resampler's tile statistics on the weight tensor; an in-place change of the
    weights afterwards (tempering, masking) must not be resampled against the stale statistics."""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    n = 300_000
    ys = workloads.lgssm_data(2)
    init, step = workloads.make_lgssm(G)
    coll = smc.ImportanceK(G.Target(init, (), G.ChoiceMap.kw(y=float(ys[0]))), k_particles=n).run_smc(G.key(3))
    coll = smc.resample(G.key(4), coll, "systematic")
    coll = smc.extend(G.key(5), coll, step, lambda tr_: (tr_.get_retval(),), G.ChoiceMap.kw(y=float(ys[1])))
    lw = coll.get_log_weights()
    assert getattr(lw, "_gmx_tile_stats", None) is not None          # the step's program wrote them
    fresh = smc.resample(G.key(6), coll, "systematic").ancestors.clone()
    lw.mul_(0.25)                                                      # tempering, in place
    tempered = smc.resample(G.key(6), coll, "systematic").ancestors
    plain = smc.ParticleCollection(coll.get_particles(), lw.clone(), True, coll.log_ml_offset)
    want = smc.resample(G.key(6), plain, "systematic").ancestors
    assert torch.equal(tempered, want) and not torch.equal(tempered, fresh)


@pytest.mark.parametrize("case", ["nan_inf", "huge", "plus_inf", "all_nan"])
def test_integer_cdf_special_values(gpu, case):
    """NaN / +-inf / absurdly large log-weights: gmx_weight_cdf and the fused gmx_resample give the oracle's
    integers and ancestors (NaN and -inf carry no mass; +inf or |lw| > 2^29 ln 2 saturate the tile exponent and
    carry none either; no mass at all -> every slot maps to the last particle)."""
    import genjax_amd as G
    from genjax_amd.inference import smc
    n = 5000
    rng = np.random.default_rng(17)
    lw = rng.normal(0, 2, n).astype(np.float32)
    if case == "nan_inf":
        lw[7] = np.nan; lw[1500] = -np.inf; lw[2047] = np.nan; lw[4999] = -np.inf
    elif case == "huge":
        lw[100] = 1e30; lw[3000] = -1e30
    elif case == "plus_inf":
        lw[2500] = np.inf
    else:
        lw[:] = np.nan
    cdf, total, mx, shift = smc.weight_cdf(_dev(lw))
    rc, rt, rm, rs = O.weight_cdf(lw)
    assert np.array_equal(cdf.cpu().numpy().view(np.uint64), rc) and int(total.item()) == rt
    ref = O.ancestors(0, O.key(3), rc) if rt else np.full(n, n - 1, np.int32)
    got = smc.ancestors_from_cdf(0, G.key(3), cdf, total).cpu().numpy()
    assert np.array_equal(got, ref)
    # the fused form: tile statistics + k_offspring_tile, no CDF in memory
    from ctypes import c_uint32
    from genjax_amd import _lib
    be = _lib.get()
    lw_d = _dev(lw)
    ws = torch.zeros(((be.c.gmx_resample_workspace(n) + 7) // 8,), dtype=torch.int64, device="cuda")
    mx2 = torch.zeros(1, dtype=torch.float32, device="cuda")
    tot2 = torch.zeros(1, dtype=torch.int64, device="cuda")
    anc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    kh = G.key(3).host()
    kk = (c_uint32 * 2)(int(kh[0]), int(kh[1]))
    be.check(be.c.gmx_resample(0, kk, be.ptr(lw_d), n, shift, None, 0, be.ptr(mx2), be.ptr(tot2), be.ptr(anc),
                               be.ptr(ws), be.stream()), "gmx_resample")
    assert int(tot2.item()) == rt and np.array_equal(anc.cpu().numpy(), ref)
    m_ref, m_got = np.float32(rm), np.float32(mx2.item())
    assert (np.isnan(m_ref) and np.isnan(m_got)) or m_ref == m_got


def test_gmx_resample_is_the_one_entry_for_every_kind(gpu):
    """include/genmi.h: `gmx_resample(kind, ...)` dispatches to the staged forms — systematic, stratified, multinomial
    (iid), multinomial_tiled, multinomial_sorted at n = 5000; the ordered kinds past 2048 tiles too — and gives the
    ancestors the staged calls (each held to the oracle by its own test) give"""
    from ctypes import c_uint32
    import genjax_amd as G
    from genjax_amd import _lib
    from genjax_amd.inference import smc
    be = _lib.get()
    rng = np.random.default_rng(5)
    for n, kinds in ((5000, (0, 1, 2, 3, 4)), ((1 << 21) + 4097, (0, 1, 4))):
        lw = (rng.normal(size=n) * 1.5).astype(np.float32)
        lw_d = _dev(lw)
        shift = smc.cdf_shift(n)
        ws = torch.zeros(((be.c.gmx_resample_workspace(n) + 7) // 8,), dtype=torch.int64, device="cuda")
        kh = G.key(11).host()
        kk = (c_uint32 * 2)(int(kh[0]), int(kh[1]))
        for kind in kinds:
            mx = torch.zeros(1, dtype=torch.float32, device="cuda")
            tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            anc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            be.check(be.c.gmx_resample(kind, kk, be.ptr(lw_d), n, shift, None, 0, be.ptr(mx), be.ptr(tot), be.ptr(anc),
                                       be.ptr(ws), be.stream()), "gmx_resample")
            if kind == 2:
                cdf, total, _, _ = smc.weight_cdf(lw_d)
                ref, rtot = smc.ancestors_from_cdf(2, G.key(11), cdf, total), total
            else:
                ref, rtot, _, _ = smc.resample_fused(kind, G.key(11), lw_d.clone())
            assert int(tot.item()) == int(rtot.item()), (n, kind)
            assert torch.equal(anc, ref), (n, kind)


def test_resampler_fuzz(gpu):
    """random sizes (ragged tiles, single tile, many tiles) x random weight shapes x both ordered kinds:
    gmx_weight_cdf's integers and gmx_resample's ancestors against the oracle"""
    from ctypes import c_uint32
    import genjax_amd as G
    from genjax_amd import _lib
    from genjax_amd.inference import smc
    be = _lib.get()
    rng = np.random.default_rng(2024)
    for it in range(40):
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 1000, 1023, 1024, 1025, 2047, 2049, 4097, 10_007, 65_536, 200_003]))
        style = it % 5
        lw = rng.normal(0, [0.1, 1, 3, 10, 30][style], n).astype(np.float32)
        if style == 3 and n > 10:
            lw[rng.choice(n, n // 3, replace=False)] = -np.inf
        if style == 4 and n > 2048:
            lw[:1024] -= 200.0                      # a whole tile 200 nats below the rest: shifted out entirely
            lw[1024:2048] += 20.0
        kind = it % 2
        key, okey = G.key(1000 + it), O.key(1000 + it)
        rc, rt, rm, rs = O.weight_cdf_c(lw)
        cdf, total, mx, shift = smc.weight_cdf(_dev(lw))
        assert shift == rs and int(total.item()) == rt, (it, n, style)
        assert np.array_equal(cdf.cpu().numpy().view(np.uint64), rc), (it, n, style)
        ref = O.ancestors(kind, okey, rc) if rt else np.full(n, n - 1, np.int32)
        anc, tot2, mx2, _ = smc.resample_fused(kind, key, _dev(lw))
        assert int(tot2.item()) == rt and np.array_equal(anc.cpu().numpy(), ref), (it, n, style, kind)
        assert float(mx2.item()) == rm


@pytest.mark.parametrize("kind", [0, 1])
def test_fused_resampler_at_its_size_limit(gpu, kind):
    """n = 2^21 = RS_MAX_TILES tiles of 1024: the largest ensemble the table-per-block resampler takes; its entry point
    refuses one more particle loudly, and `resample_fused` then goes through the tile-prefix form (same ancestors)."""
    import genjax_amd as G
    from genjax_amd import _lib
    from genjax_amd.inference import smc
    n = 2048 * 1024
    rng = np.random.default_rng(5)
    lw = rng.normal(0, 4, n).astype(np.float32)
    rc, rt, rm, rs = O.weight_cdf_c(lw)
    ref = O.ancestors(kind, O.key(9), rc)
    anc, tot, mx, _ = smc.resample_fused(kind, G.key(9), _dev(lw))
    assert int(tot.item()) == rt and float(mx.item()) == rm
    assert np.array_equal(anc.cpu().numpy(), ref)
    from ctypes import c_uint32
    be = _lib.get()
    lw1 = _dev(np.concatenate([lw, np.float32([1.5])]))
    ws = torch.zeros(((be.c.gmx_resample_workspace(n + 1) + 7) // 8,), dtype=torch.int64, device=be.device)
    out = [torch.zeros((1,), dtype=torch.float32, device=be.device), torch.zeros((1,), dtype=torch.int64, device=be.device),
           torch.zeros((n + 1,), dtype=torch.int32, device=be.device)]
    tiles1 = (n + 1 + 1023) // 1024
    st = (torch.zeros((tiles1,), dtype=torch.float32, device=be.device), torch.zeros((tiles1,), dtype=torch.int64, device=be.device))
    be.check(be.c.gmx_tile_stats(be.ptr(lw1), n + 1, smc.cdf_shift(n + 1), be.ptr(st[0]), be.ptr(st[1]), be.stream()), "gmx_tile_stats")
    with pytest.raises(_lib.GenmiError, match="too large"):          # the table-per-block form itself refuses
        be.check(be.c.gmx_resample_tiles(kind, (c_uint32 * 2)(1, 2), be.ptr(lw1), n + 1, smc.cdf_shift(n + 1), be.ptr(st[0]),
                                         be.ptr(st[1]), be.ptr(out[0]), be.ptr(out[1]), be.ptr(out[2]), be.stream()),
                 "gmx_resample_tiles")
    rc1, rt1, rm1, _ = O.weight_cdf_c(lw1.cpu().numpy())
    ref1 = O.ancestors_c(kind, O.key(9), rc1)
    anc1, tot1, mx1, _ = smc.resample_fused(kind, G.key(9), lw1)
    assert int(tot1.item()) == rt1 and float(mx1.item()) == rm1
    assert np.array_equal(anc1.cpu().numpy(), ref1)
    # ... and the one entry point dispatches to the tile-prefix form by itself
    kh = G.key(9).host()
    be.check(be.c.gmx_resample(kind, (c_uint32 * 2)(int(kh[0]), int(kh[1])), be.ptr(lw1), n + 1, smc.cdf_shift(n + 1), None, 0,
                               be.ptr(out[0]), be.ptr(out[1]), be.ptr(out[2]), be.ptr(ws), be.stream()), "gmx_resample")
    assert int(out[1].item()) == rt1 and np.array_equal(out[2].cpu().numpy(), ref1)


@pytest.mark.parametrize("n,shape", [(8192, "normal"), (10_000, "onehot"), (10_000, "none"), (100_003, "heavy"),
                                     (1_000_000, "normal"), (3_000_000, "sparse")])
def test_multinomial_two_level_search(gpu, n, shape):
    """multinomial ancestors for n >= 8192 go through k_ancestors_mn (coarse CDF samples in LDS, then log2(S)
    global reads): the same integer predicate as the one-level search, so the oracle's indices bit for bit"""
    import genjax_amd as G
    from genjax_amd.inference import smc
    lw = parity.pull_weights(n, shape, seed=n % 7) if hasattr(parity, "pull_weights") else None
    if lw is None:
        rng = np.random.default_rng(n)
        lw = rng.normal(0, 2, n).astype(np.float32)
        if shape == "onehot":
            lw[:] = -np.inf; lw[(n * 5) // 7] = 0.0
        elif shape == "none":
            lw[:] = -np.inf
        elif shape == "heavy":
            lw = rng.normal(0, 12, n).astype(np.float32)
        elif shape == "sparse":
            keep = rng.choice(n, n // 997, replace=False)
            m = np.full(n, -np.inf, np.float32); m[keep] = lw[keep]; lw = m
    cdf, total, _, _ = smc.weight_cdf(_dev(lw))
    rc, rt, _, _ = O.weight_cdf_c(lw)
    assert int(total.item()) == rt
    anc = smc.ancestors_from_cdf(2, G.key(5), cdf, total).cpu().numpy()
    ref = O.ancestors_c(2, O.key(5), rc) if rt else np.full(n, n - 1, np.int32)
    assert np.array_equal(anc, ref)


@pytest.mark.parametrize("n,capture,specialize", [(3000, False, False), (100_000, True, True)])
def test_vector_state_mh_sweep_matches_oracle(gpu, n, capture, specialize):
    """the fused MH sweep with a 2-vector state (one vector-valued site), interpreter and specialised + captured"""
    parity.check_vector_mh_sweep(n=n, T=5, capture=capture, specialize=specialize)


@pytest.mark.parametrize("chained", [False, True])
def test_mh_move_chained_into_the_extension(gpu, chained):
    """BootstrapSweep(chain_mh=) on the HIP library: the MH move + the extension as one specialised program (4 particles
    per thread, tile statistics from its epilogue) or as two launches — ancestors, states, weights, accept bits and
    evidence equal the oracle's, interpreter and specialised kernel, eager and captured."""
    parity.check_nlssm_mh_sweep(n=3000, T=5, want_chained=chained, chain_mh=chained)
    parity.check_nlssm_mh_sweep(n=100_003, T=4, specialize=True, capture=True, want_chained=chained, chain_mh=chained)
    res = parity.check_vector_mh_sweep(n=2500, T=4, chain_mh=chained)
    assert 0.3 < res["accept_rate"] < 1.0


@pytest.mark.parametrize("case", ["normal", "flat", "skewed", "sparse", "one", "nan_inf", "none"])
def test_multinomial_through_the_guide_table(gpu, case):
    """gmx_multinomial (guide table + a search over ~3 entries) == gmx_ancestors' per-slot binary search, slot for slot,
    on mild, flat, skewed, sparse, degenerate and NaN / inf weight vectors, n_out != n_in included; the mild case also
    against the oracle."""
    import genjax_amd as G
    from genjax_amd.inference import smc
    n = 300_007
    rng = np.random.default_rng(5)
    lw = rng.normal(0, 1, n).astype(np.float32)
    if case == "flat":
        lw[:] = 0.0
    elif case == "skewed":
        lw = rng.normal(0, 6, n).astype(np.float32)
    elif case == "sparse":
        lw = np.where(rng.random(n) < 1e-3, 0.0, -60.0).astype(np.float32)
    elif case == "one":
        lw[:] = -1e30
        lw[77_777] = 0.0
    elif case == "nan_inf":
        lw[5] = np.nan; lw[100_000] = -np.inf; lw[200_001] = np.nan; lw[n - 1] = -np.inf
    elif case == "none":
        lw[:] = -np.inf
    cdf, total, _, _ = smc.weight_cdf(_dev(lw))
    from ctypes import c_uint32
    be = G._lib.get()
    kh = G.key(31).host()
    kk = (c_uint32 * 2)(int(kh[0]), int(kh[1]))
    for n_out in (n, 40_000, 500_000):
        a = smc.ancestors_from_cdf(2, G.key(31), cdf, total, n_out=n_out)           # through the guide table
        b = torch.empty((n_out,), dtype=torch.int32, device=cdf.device)             # the per-slot search
        be.check(be.c.gmx_ancestors(2, kk, be.ptr(cdf), n, 0, be.ptr(total), n_out, 0, n_out, be.ptr(b), be.stream()),
                 "gmx_ancestors")
        assert torch.equal(a, b)
    if case == "normal":
        rc, _, _, _ = O.weight_cdf(lw)
        assert np.array_equal(b.cpu().numpy(), O.ancestors_c(2, O.key(31), rc, n_out=500_000))


def test_long_scan_with_a_vector_valued_site(gpu):
    """counted-loop scan, 2-D latent state in one site: interpreter (n = 130) and specialised kernel (n = 70 000)"""
    parity.check_scan_long_vector_site()
    parity.check_scan_long_vector_site(n=70_000, T=24, seed=8)


def test_long_scan_update_and_regenerate(gpu):
    """counted-loop Scan.edit on the HIP library: interpreter (n = 150) and specialised kernel (n = 70 000, T = 24)"""
    parity.check_scan_long_edits()
    parity.check_scan_long_edits(n=70_000, T=24, seed=4)


def test_long_scan_vector_sites_constraints_and_edits(gpu):
    parity.check_scan_long_vector_constraints()
    parity.check_scan_long_vector_constraints(n=50_000, T=20, seed=2)


@pytest.mark.parametrize("n,no,T,jit", [(5000, 3, 40, True), (5000, 24, 40, True), (2000, 24, 40, False), (1500, 100, 100, True)])
def test_plate_of_long_scans_as_nested_loops(gpu, monkeypatch, n, no, T, jit):
    """a plate of time series: two nested counted loops in one launch (interpreter, and the specialised kernel: the
    threshold above which a program is specialised is lowered for the test), simulate / importance / assess bit-exact vs
    the oracle; 100 series x 100 steps = 1e4 latent pairs per particle"""
    from genjax_amd import engine
    monkeypatch.setattr(engine, "JIT_MIN_PARTICLES", 1024 if jit else 1 << 40)
    monkeypatch.setattr(engine, "JIT_MIN_WORK", 1024 if jit else 1 << 40)
    import genjax_amd as G
    G.clear_caches()
    parity.check_plate_of_scans(n=n, no=no, T=T)


@pytest.mark.parametrize("jit", [True, False])
def test_nested_combinators_on_device(gpu, monkeypatch, jit):
    """plate of plates, scan of plate, scan of scan (both levels long) through the interpreter and the specialised kernel"""
    from genjax_amd import engine
    monkeypatch.setattr(engine, "JIT_MIN_PARTICLES", 1024 if jit else 1 << 40)
    monkeypatch.setattr(engine, "JIT_MIN_WORK", 1024 if jit else 1 << 40)
    import genjax_amd as G
    G.clear_caches()
    parity.check_nested_combinators(n=3000)
    parity.check_nested_constraint_forms(n=2000)
    parity.check_nested_edge_cases()


def test_two_stage_multinomial_on_device(gpu):
    """gmx_multinomial_tiled (k_mn_hist + k_mn_tile) == the oracle's definition: ragged / one-tile / one-particle sizes,
    a spike that gives one tile almost every slot, no mass at all, 1e6 particles; and whole sweeps resampled with it
    (one stream, and noise ahead with the stage-1 uniforms from the background stream), captured"""
    for kw in (dict(n=5000), dict(n=1024, seed=6), dict(n=3333, seed=7, spike=30.0), dict(n=2500, seed=8, dead=True),
               dict(n=1, seed=9), dict(n=1025, seed=10, sigma=8.0), dict(n=1_000_000, seed=11, sigma=1.5),
               dict(n=300_001, seed=12, spike=12.0)):
        parity.check_multinomial_tiled(**kw)
    for na in (False, True):
        res = parity.check_lgssm_sweep(n=50_000, T=13, capture=True, specialize=True, resample="multinomial_tiled", noise_ahead=na)
        assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"] and res["lw_max_abs_diff"] == 0.0


def test_sorted_multinomial_on_device(gpu):
    """gmx_sorted_uniforms (k_sorted_exp + k_sorted_guide) word for word against the oracle's statement of the table, and
    gmx_resample_sorted (k_offspring_tile on the order-statistics table) == the oracle's definition: ragged / one-tile /
    one- and two-particle sizes, a spike that owns almost every slot, no mass at all, 1e6 and 2^21 particles; whole sweeps
    resampled with it (one stream, and noise ahead with the tables from the background stream), captured"""
    for kw in (dict(n=5000, rows=3), dict(n=1024, seed=6), dict(n=3333, seed=7, spike=30.0), dict(n=2500, seed=8, dead=True),
               dict(n=1, seed=9), dict(n=2, seed=13), dict(n=1025, seed=10, sigma=8.0), dict(n=1_000_000, seed=11, sigma=1.5, rows=2),
               dict(n=300_001, seed=12, spike=12.0), dict(n=2048 * 1024, seed=14, sigma=0.5)):
        parity.check_multinomial_sorted(**kw)
    for na in (False, True):
        res = parity.check_lgssm_sweep(n=50_000, T=13, capture=True, specialize=True, resample="multinomial_sorted", noise_ahead=na)
        assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"] and res["lw_max_abs_diff"] == 0.0


@pytest.mark.parametrize("kind", ["systematic", "stratified", "multinomial", "multinomial_tiled", "multinomial_sorted"])
def test_evidence_estimate_is_unbiased_on_device(gpu, kind):
    """E[Z_hat] = Z (Kalman closed form) over 1000 sweeps of 32 particles on the HIP library: independent of the oracle"""
    parity.check_evidence_unbiased(kind, R=1000, seed0=5000)


def test_sampler_laws_against_scipy_on_device(gpu):
    """the HIP samplers against scipy's distributions: KS / chi-square / moments, independent of the oracle"""
    parity.check_sampler_laws(n=400_000)


@pytest.mark.parametrize("kind", ["systematic", "stratified", "multinomial", "multinomial_tiled", "multinomial_sorted"])
def test_offspring_laws_on_device(gpu, kind):
    parity.check_offspring_laws(kind, R=2000)


@pytest.mark.parametrize("A,T", [(3, 20), (12, 20), (40, 40)])
def test_update_through_a_plate_of_long_scans_on_device(gpu, A, T):
    parity.check_nested_edits(A, T, n=3000)


@pytest.mark.parametrize("A,T,n", [(20, 24, 9), (3, 24, 2000), (40, 40, 3000)])
def test_index_requests_through_nested_loops_on_device(gpu, A, T, n):
    """IndexRequest into a plate of long scans and into a scan of plates, gated inside the loops: interpreter (n = 9)
    and specialised kernels, against the oracle and scipy"""
    parity.check_nested_index_edits(A, T, n=n)


def test_a_sweep_prepared_again_runs_the_new_key(gpu):
    """BootstrapSweep.prepare() a second time on the same object (found by the unbiasedness test: the noise-ahead form
    kept the first run's background launches): every re-prepared run equals a fresh sweep's, eager and captured"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    T, N = 8, 4096
    ys = torch.from_numpy(workloads.lgssm_data(T))
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, N, T)
    for r in range(4):
        sw.prepare(G.key(70 + r), ys)
        if r >= 2:
            sw.capture()
        sw.launch()
        fresh = BootstrapSweep(init, step, N, T).prepare(G.key(70 + r), ys)
        fresh.launch()
        assert sw.log_ml() == fresh.log_ml()
        for a, b in zip(sw.state(), fresh.state()):
            assert torch.equal(a, b)


def test_importancek_evidence_is_unbiased_on_device(gpu):
    parity.check_importance_unbiased(R=20000)


def test_evidence_estimate_is_unbiased_with_mh_moves_on_device(gpu):
    parity.check_evidence_unbiased("systematic", R=1000, T=6, mh=True, seed0=900000)


def test_marginal_density_estimates_are_unbiased_on_device(gpu):
    parity.check_marginal_density_unbiased(R=20000)


def test_long_scan_importance_weights_against_kalman_on_device(gpu):
    parity.check_scan_importance_vs_kalman(n=2_000_000)


@pytest.mark.parametrize("comm,world,na,capture", [("p2p", 2, 0, 0), ("p2p", 2, 1, 1), ("p2p", 4, 1, 1),
                                                   ("peer", 2, 0, 0), ("peer", 2, 1, 1), ("peer", 4, 1, 1)])
def test_peer_mapped_exchange_between_two_processes_on_the_device(gpu, tmp_path, comm, world, na, capture):
    """GENMI_COMM=peer: the FUSED exchange — the site programs put their statistics into the other PROCESSES' landing
    tables as tagged granules, gmx_shard_step_peer polls its own, puts states into the owners' landing blocks and waits
    for what its slots need; no collective launch, no fence.
    GENMI_COMM=p2p at WORLD SIZE 2 (and 4) on real device memory: the processes (ranks) share the box's one GPU, map each
    other's fine-grained landing buffers and flags through IPC handles (gmx_p2p_alloc / gmx_p2p_open) and run the
    sharded sweep with every collective as ONE gmx_p2p_exchange launch — puts into the peer's memory, release, flag,
    bounded wait, copy out, device-side epoch.  Bit-exact against the single-process oracle, eagerly and as a captured
    graph replayed twice, one-stream and noise ahead.  (Same-GPU peers say nothing about xGMI speed: correctness only.)"""
    import json
    from genjax_amd import workloads
    from tests.test_distributed_cpu import _launch
    n_total, T = 8192, 6
    out = str(tmp_path / "p2p_gpu")
    r = _launch(world, [out, str(n_total // world), str(T)],
                extra_env={"GENMI_COMM": comm, "GENMI_NOISE_GROUP": "3", "GENMI_COMM_TIMEOUT": "60",
                           "GENMI_TEST_OPTS": json.dumps({"on_gpu": 1, "noise_ahead": na, "capture": capture})})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    x = np.load(out + ".npy")
    meta = json.load(open(out + ".json"))
    assert meta["communicator"].startswith(comm)
    # (peer: ONE launch per step — the gathering program routes the previous step first, between PROCESSES here)
    assert meta["one_launch_per_step"] == (comm == "peer"), meta
    ys = workloads.lgssm_data(T)
    oi, ost = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, ost, n_total, T, ys, O.key(314159))
    assert [int(t) for t in meta["totals"]] == [h["total"] for h in ref["hist"]]
    assert meta["log_ml"] == ref["log_ml"]
    assert np.array_equal(x, ref["x"][ref["anc"]])


@pytest.mark.parametrize("world,capture", [(2, 0), (2, 1), (4, 1)])
def test_sharded_mh_sweep_routes_inside_the_move_between_processes_on_the_device(gpu, tmp_path, world, capture):
    """BASELINE config 3 sharded over the fused peer exchange (round 6): the MH move's program is the one that gathers, so
    IT routes the previous step first — two routed leaves per state component (the particle and the state it was extended
    from) — and the extension reads the moved state locally: two launches per step instead of three, no routing launch,
    no collective.  Between PROCESSES on the box's one GPU, eagerly and as a captured graph replayed twice; equal to the
    single-process oracle."""
    import json
    from tests.test_distributed_cpu import _launch
    n_total, T = 8192, 5
    out = str(tmp_path / "peer_mh_gpu")
    r = _launch(world, [out, str(n_total // world), str(T), "0", "mh"],
                extra_env={"GENMI_COMM": "peer", "GENMI_COMM_TIMEOUT": "60",
                           "GENMI_TEST_OPTS": json.dumps({"on_gpu": 1, "capture": capture})})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    x = np.load(out + ".npy")
    meta = json.load(open(out + ".json"))
    assert meta["communicator"].startswith("peer")
    assert meta["one_launch_per_step"] is True and meta["chained_mh"] is True, meta
    ref = parity.oracle_nlssm_mh_sweep(n_total, T, 7)
    assert np.array_equal(x, ref["resampled"])
    assert abs(meta["log_ml"] - sum(ref["terms"])) < 1e-9 * max(1.0, abs(sum(ref["terms"])))


def test_rows_of_logits_at_one_categorical_site_on_device(gpu):
    """`categorical(logits [J, 3])` per particle (J draws at one site): simulate / importance / update against the oracle,
    at an interpreter size and at 2^17 particles (specialised)"""
    parity.check_rows_of_logits_at_one_site(B=257, J=12)
    parity.check_rows_of_logits_at_one_site(B=1 << 17, J=8, seed=11)


def test_mixture_with_latent_means_on_device(gpu):
    """a Gaussian mixture whose means are latent (`normal(mus[zs], 1)`: traced indices into values computed in the model),
    at an interpreter size and at 2^17 particles (specialised): simulate / importance / update against the oracle"""
    parity.check_mixture_with_latent_means(B=129)
    parity.check_mixture_with_latent_means(B=129, n_comp=20, seed=9)        # a long vector site's values: a search loop
    parity.check_mixture_with_latent_means(B=1 << 17, J=5, seed=13)
    parity.check_mixture_with_latent_means(B=1 << 17, J=4, n_comp=20, seed=14)


def test_slices_of_a_long_per_particle_vector_on_device(gpu):
    """slices (`ys[1:]`, `ys[10:40]`, differences, reversed, strided) of a long per-particle vector and of a latent one as
    a vector site's parameter, interpreter size and 2^17 particles (specialised): importance weights against the oracle"""
    parity.check_slices_of_a_long_per_particle_vector(B=65)
    parity.check_slices_of_a_long_per_particle_vector(B=1 << 17, N=24, seed=6)


def test_changed_per_particle_vector_argument_on_device(gpu):
    """`update` under a changed per-particle vector argument of a large plate, a long scan and a vector site: weights and
    scores against the oracle, interpreter size and 2^17 particles (specialised)"""
    parity.check_changed_per_particle_vector_argument(B=65)
    parity.check_changed_per_particle_vector_argument(B=1 << 17, N=20, seed=15)


def test_gather_of_a_latent_vector_at_a_table_of_group_indices_on_device(gpu):
    """as tests/test_host_logic.py: interpreter size and 2^17 particles (specialised)"""
    parity.check_gather_at_group_indices()
    parity.check_gather_at_group_indices(J=24, N=200, K=1 << 17, seed=5)


def test_gather_by_index_vector_on_device(gpu):
    """`normal(means[zs] + s, 1)` with the assignments given as a table or one vector per particle: importance and update
    under changed assignments against the oracle"""
    assert parity.check_gather_by_index_vector(B=129) == 6


def test_sweep_with_vector_observations_on_device(gpu):
    """BootstrapSweep over an HMM with 24 observations per step (a long vector-valued site in the step program: one
    counted loop per particle), interpreter size and 2^18 particles (specialised, one launch per step): log-ML and every
    step's integer total against the oracle's sweep"""
    parity.check_sweep_with_vector_observations(n=2048, T=4, m=24)
    parity.check_sweep_with_vector_observations(n=1 << 18, T=5, m=24, seed=9)


def test_sweep_verdict_on_device(gpu, monkeypatch):
    """gmx_sweep_verdict + finish() on the HIP library, over the fused peer exchange (status words exist)"""
    monkeypatch.setenv("GENMI_COMM", "peer")
    assert parity.check_sweep_verdict() >= 2


def test_peer_route_of_twelve_leaves_between_two_processes_on_the_device(gpu, tmp_path):
    """the fused peer exchange past eight routed leaves (GMX_PEER_MAX_LEAVES = 32): a 6-vector state
    and one MH move per step — the particle and the state it was extended from travel as 2 x 6 leaves between two
    PROCESSES on the device, capacity 0 (automatic) — equals the single-process oracle"""
    import json
    from tests.test_distributed_cpu import _launch
    n_total, T, D = 8192, 4, 6
    out = str(tmp_path / "peer12")
    r = _launch(2, [out, str(n_total // 2), str(T), "0", "vec6mh"],
                extra_env={"GENMI_COMM": "peer", "GENMI_COMM_TIMEOUT": "60", "GENMI_TEST_OPTS": json.dumps({"on_gpu": 1})})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    x = np.load(out + ".npy")
    meta = json.load(open(out + ".json"))
    assert meta["communicator"].startswith("peer")
    oi, ost = parity.make_vec_mh(O, lambda *v: np.stack(v, axis=-1), np.ones(D, np.float32))
    oreq = {"x": O.Rejuvenate(O.normal, lambda chm: (chm.get_value(), np.float32(0.2)))}
    ref = parity.oracle_mh_sweep(oi, ost, oreq, parity.tracker_data(T), n_total, T, 11, extra=lambda t: (np.float32(t),))
    assert x.shape == (n_total, D) and np.array_equal(x, ref["x"][ref["anc"]])
    assert abs(meta["log_ml"] - sum(ref["terms"])) < 1e-9 * max(1.0, abs(sum(ref["terms"])))


def test_random_models_match_the_oracle_on_device(gpu):
    """tests/fuzz_models.py on the HIP path: 10 random models on the interpreter (7 particles, 2 to 4 statements each — long
    models, chains of launches, have a test of their own and run in tools/experiments/fuzz_on_device.py; plates, plates of plates and scans of long vector
    sites among them)
    and 2 through the hiprtc-specialised programs (2^18 particles: engine.JIT_MIN_PARTICLES; long vector sites, a latent
    vector feeding a vector site, beside scans), every GFI method bit for bit against the oracle.  (The seeds are
    named: a draw of sixteen in a row held five long models, and a plate of long vector sites at 2^18 particles is two
    minutes of numpy oracle — tools/experiments/fuzz_on_device.py runs those, profiles/r05z_fuzz_on_device.json.)"""
    from tests import fuzz_models as F
    ran = 0
    small = (1000, 1001, 1003, 1006, 1012, 1016, 1019, 1020, 1023, 1029)
    for seed, B in [(s, 7) for s in small] + [(s, 1 << 18) for s in (2000, 2006)]:
        try:
            F.run_one(seed, B=B)
            ran += 1
        except F.OverTheLimits:
            pass
    assert ran == 12, ran
    for seed in range(3000, 3004):
        F.run_smc_one(seed)
    for seed in range(4000, 4003):
        F.run_big_one(seed)
    F.run_big_one(4100, n_big=100_003, K=50)


def test_models_of_more_sites_than_one_launch_holds_on_device(gpu):
    """ref static.py:254-380: 32-, 40- and 200-site models as chains of launches (program.split_graph) on the HIP
    library — the interpreter (9 / 130 particles) and the hiprtc-specialised programs (2^18 particles) — every GFI
    method bit for bit against the oracle"""
    from tests import parity
    for ns in (32, 40, 200):
        parity.check_many_sites(ns=ns)
    parity.check_many_sites(ns=67, B=130, seed=8, kinds=("normal", "flip", "normal", "uniform"))
    parity.check_many_sites(ns=40, B=1 << 18, seed=5, kinds=("normal", "flip", "normal", "uniform"))


def test_three_combinator_levels_at_loop_sizes_on_device(gpu):
    """ref vmap.py:180-218: vmap(vmap(vmap(elem))) over 20 x 20 x 20 — three counted loops in one site program — on
    the interpreter (5 particles) and the hiprtc-specialised kernel (2^18 particles would be 2e9 element draws on the
    oracle: 4096 particles through an explicit specialize), and mixed sizes; against the oracle"""
    from genjax_amd import engine
    from tests import parity
    parity.check_three_nested_plates()
    parity.check_three_nested_plates(dims=(3, 20, 17), B=9, seed=4)
    parity.check_three_nested_plates(dims=(18, 2, 33), B=3, seed=5)
    old = engine.JIT_MIN_PARTICLES
    engine.JIT_MIN_PARTICLES = 64
    try:
        engine.clear_caches()
        parity.check_three_nested_plates(dims=(20, 20, 20), B=128, seed=7)
    finally:
        engine.JIT_MIN_PARTICLES = old
        engine.clear_caches()


def test_index_request_on_a_long_scan_is_o1_on_device(gpu):
    """ref scan.py:325-416 `edit_index` in O(1) steps (combinators._scan_edit_index_o1): chains of edits on 40- and
    70-step scans against the oracle and the counted-loop form; 2^18 particles through the specialised programs"""
    from tests import parity
    parity.check_scan_index_request_o1()
    parity.check_scan_index_request_o1(n=9, T=70, seed=3, edits=40)
    parity.check_scan_index_request_o1(n=1 << 18, T=24, seed=5, edits=4)


def test_nested_index_request_on_a_plate_of_long_scans_is_o1_on_device(gpu):
    """a one-step edit of one element of a 64 x 4 096 plate of scans (`kernel.scan(n=T).vmap()`) is at
    least 20x faster than the counted-loop form, with the same weights / scores / values (1 000 particles: a leaf is
    1 GB; the 1e5 the verdict names would be 105 GB per leaf); the chains of edits against the oracle at small sizes,
    Python-int and per-particle indices at both levels"""
    import os
    import sys
    from tests import parity
    parity.check_plate_of_scans_index_request_o1()
    parity.check_plate_of_scans_index_request_o1(n=300, J=17, T=70, seed=5, edits=12)
    parity.check_scan_of_plates_index_request_o1(n=300, T=70, P=20, seed=8, edits=8)     # a plate inside the scan's step
    for seed in range(8):
        parity.check_direct_plate_of_scans_random(seed)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import nested_index_request_cost as cost
    out = cost.run(1000, 64, 4096)
    print("nested index request:", out)
    assert out["same_weights_scores_values"] and out["speedup"] >= 20.0, out
    out_pp = cost.run(1000, 64, 1024, per_particle=True)
    print("nested index request, one index per particle:", out_pp)
    assert out_pp["same_weights_scores_values"] and out_pp["speedup"] >= 5.0, out_pp


def test_hmc_programs_over_long_vector_sites_as_specialised_kernels(gpu):
    """the HMC / Regenerate / Rejuvenate programs of tests/cookbook.py — loops, per-element gradient contributions, sums, the
    gather's scatter-add, ONE trace — with EVERY program sent through hiprtc (engine.JIT_MIN_PARTICLES = 1) at J = 40:
    specialised kernels against the oracle, each also held to the interpreter by the first-launch cross-check"""
    from genjax_amd import engine
    from tests import cookbook
    old = engine.JIT_MIN_PARTICLES
    before = int(gpu.c.gmx_jit_rejected_count())
    engine.JIT_MIN_PARTICLES = 1
    try:
        engine.clear_caches()
        cookbook.check_hmc_through_long_vector_sites(npts=100, J=40)
    finally:
        engine.JIT_MIN_PARTICLES = old
        engine.clear_caches()
    assert int(gpu.c.gmx_jit_rejected_count()) == before


def test_long_vector_valued_sites_on_device(gpu):
    """ref tensorflow_probability/__init__.py:52-62 + distribution.py:383-396: `normal(a * xs + b, sigma) @ "y"` with 40 /
    500 / 5 000 observations under a particle batch as ONE counted loop per particle — interpreter (few particles) and
    hiprtc-specialised (2^18 particles) — bit for bit against the oracle"""
    from tests import parity
    parity.check_long_vector_sites(n=500, K=64)
    parity.check_long_vector_sites(n=40, K=9, seed=3)
    parity.check_long_vector_sites(n=5000, K=17, seed=5)
    parity.check_long_vector_sites(n=48, K=1 << 18, seed=7)


def test_latent_vector_feeding_the_next_vector_site_on_device(gpu):
    """8-schools at J = 40 / 200 schools (BASELINE config 4's model beyond J = 8): the latent vector's values are the next
    vector site's parameters, read back from the launch's own output in that site's loop (engine.StepAlias; Regenerate
    of the vector: unrolled, a chain of launches) — interpreter and hiprtc-specialised (2^18 particles, J = 24) —
    against the oracle, bit for bit"""
    parity.check_hierarchical_vector_latent(J=40)
    parity.check_hierarchical_vector_latent(J=200, K=9, seed=4)
    parity.check_hierarchical_vector_latent(J=24, K=1 << 18, seed=8)


def test_update_under_a_changed_table_argument_on_device(gpu):
    """an UnknownChange argument that is a launch-uniform table (> 16 elements, read at a run-time index in the loop):
    every element re-scored — one plate, a plate of plates, a scan over a table, `means[idx]` (ref vmap.py:236-275)"""
    parity.check_update_under_changed_table_arguments()
    parity.check_update_under_changed_table_arguments(B=2000, n=100, seed=9)


def test_mask_combinator_and_masked_scans_on_device(gpu):
    """ref combinators/mask.py:96-262, scan.py:1050-1150 (VERDICT r3 missing item 5b): MaskCombinator, plates of masked
    elements, masked_iterate / masked_iterate_final on the HIP path, bit for bit against the oracle"""
    parity.check_mask_combinator()
    parity.check_mask_combinator(B=3000, T=12, n_plate=100, seed=8)
    parity.check_masked_image_model()
    parity.check_masked_image_model(B=3, size=200, seed=2)       # the notebook's own image size (masking.ipynb c26)


def test_hmc_move_leaves_the_posterior_invariant_on_device(gpu):
    parity.check_hmc_invariance(n=1_000_000)


def test_edit_request_weights_against_scipy_on_device(gpu):
    parity.check_edit_weights_against_scipy(n=500_000)


def test_csmc_weights_against_scipy_on_device(gpu):
    parity.check_csmc_weights_against_scipy(B=200_000)


def test_more_closed_forms_on_device(gpu):
    parity.check_more_closed_forms(n=1_000_000)


# ---------------------------------------------------------------------------
# the reference's cookbook as a parity corpus (tests/cookbook.py), through the C-ABI
# ---------------------------------------------------------------------------
def test_cookbook_speed_gains_on_device(gpu):
    """3_speed_gains.ipynb: SIR (c8) at its `model_sizes` x 100 particles; the MH move (c15) for ONE trace at c17's sizes up
    to 1e6 and for 100 and 10 000 chains — interpreter and (from 2^18 particles) specialised kernels"""
    from tests import cookbook
    for n in (10, 100, 1000):
        cookbook.check_speed_gains_sir(n=n, N=100)
    for n, N in ((10, None), (1000, None), (4096, None), (1_000_000, None), (10, 100), (100, 100), (1000, 100), (100, 10_000)):
        cookbook.check_speed_gains_mh(n=n, N=N)


def test_cookbook_mcmc_and_importance_sampling_on_device(gpu):
    from tests import cookbook
    cookbook.check_mcmc_notebook(N=None)
    cookbook.check_mcmc_notebook(N=50)
    cookbook.check_mcmc_notebook(N=300_000, steps=3)       # past the specialisation threshold
    cookbook.check_importance_sampling_sir()


def test_cookbook_mixture_model_under_a_batch_on_device(gpu):
    """(programs of more than 31 live values are hiprtc-specialised at ANY particle count, and the compile of a mixture
    program grows with k: 14 / 21 / 83 / 147 s of hiprtc for the five programs at k = 12 / 20 / 40 / 64
    (profiles/r06i_slow_tests.txt) — the two large ones run in the test below, outside the default suite, and on the CPU
    mirror in tests/test_host_logic.py)"""
    from tests import cookbook
    for k, n in ((12, 40), (20, 100)):
        cookbook.check_mixture_notebook_under_a_batch(k=k, n=n)
    cookbook.check_mixture_notebook_under_a_batch(k=20, n=100, B=3000, seed=4)


@pytest.mark.skipif(not os.environ.get("GENMI_SLOW_TESTS"), reason="4 minutes of hiprtc: GENMI_SLOW_TESTS=1 (profiles/r06a_cookbook_gpu.log, r06i)")
def test_cookbook_mixture_model_at_the_notebook_sizes_on_device(gpu):
    from tests import cookbook
    for k, n in ((40, 500), (64, 1000)):
        cookbook.check_mixture_notebook_under_a_batch(k=k, n=n)


def test_cookbook_scan_outputs_and_array_carries_on_device(gpu):
    from tests import cookbook
    for T_, N in ((8, None), (8, 6), (40, None), (40, 6), (300, 6), (100, 5000)):
        cookbook.check_scan_outputs_and_array_carries(T_=T_, N=N)


def test_first_launch_cross_check_rejects_a_wrong_specialised_kernel(gpu, monkeypatch):
    """VERDICT r5 item 5 (hiprtc miscompiled two specialised kernels in round 5): every freshly specialised program runs
    once beside the ahead-of-time interpreter on the first 256 particles of its first launch (engine.Compiled._cross_check);
    a kernel that differs is dropped and the interpreter takes over.  A DELIBERATELY wrong kernel (GENMI_JIT_FAULT=1: every
    stored 32-bit word has its lowest bit flipped) must be caught — the results then equal the oracle's all the same — and
    a correct one must pass without being dropped.  (The two recorded seeds, 17049 / 19153, held a copy loop the tracer no
    longer emits: they cannot be rebuilt; the fault injection stands in for them.)"""
    import warnings
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C
    n = 1 << 18           # (the size from which a program is specialised at its first launch)

    def mk(g, c):
        @g.gen
        def m(a):
            x = g.normal(a * c, 1.0 if g is G else np.float32(1.0)) @ "x"
            y = g.normal(x * c, 2.0 if g is G else np.float32(2.0)) @ "y"
            return x + y
        return m
    a = np.random.default_rng(0).normal(size=n).astype(np.float32)
    before = int(gpu.c.gmx_jit_rejected_count())
    # a correct kernel passes
    m, om = mk(G, 0.731), mk(O, np.float32(0.731))
    tr = m.simulate(G.split(G.key(3), n), (torch.from_numpy(a).to(gpu.device),))
    otr = om.simulate(O.split(O.key(3), n), (a,))
    assert np.array_equal(tr.get_choices()["y"].cpu().numpy(), otr.get_choices()["y"])
    assert int(gpu.c.gmx_jit_rejected_count()) == before
    # a wrong one is caught, dropped, and the launch still returns the right numbers (the interpreter's)
    monkeypatch.setenv("GENMI_JIT_FAULT", "1")
    m2, om2 = mk(G, 0.377), mk(O, np.float32(0.377))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr2 = m2.simulate(G.split(G.key(4), n), (torch.from_numpy(a).to(gpu.device),))
    monkeypatch.delenv("GENMI_JIT_FAULT")
    otr2 = om2.simulate(O.split(O.key(4), n), (a,))
    assert int(gpu.c.gmx_jit_rejected_count()) == before + 1
    assert any("disagreed with the interpreter" in str(w.message) for w in rec)
    assert b"rejected" in gpu.c.gmx_last_error()
    assert np.array_equal(tr2.get_choices()["y"].cpu().numpy(), otr2.get_choices()["y"])
    assert np.array_equal(tr2.get_score().cpu().numpy(), np.asarray(otr2.get_score(), np.float32))


def test_hmc_and_regenerate_through_long_vector_sites_on_device(gpu):
    from tests import cookbook
    for npts, J in ((100, 40), (500, 200)):          # (J = 1 000: on the CPU mirror, tests/test_host_logic.py)
        cookbook.check_hmc_through_long_vector_sites(npts=npts, J=J)
    cookbook.check_hmc_through_long_vector_sites(npts=500, J=200, K=300_000, L=1)          # specialised kernels
