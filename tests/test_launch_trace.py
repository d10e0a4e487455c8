"""The C-ABI calls of every sweep form and one-off resampling (tests/launch_trace.py) against the record made at the
parent of the commit that gave inference/smc.py ONE resampling launcher and ONE step loop
(tests/golden/make_launch_trace.py): same calls, same order, same integers, same sharing of buffers — on the C-ABI's
CPU mirror.  The "sharded/" and "sharded_importance/" cases were recorded at the parent of the commit that gave
inference/sharded.py its _ShardRouter; the "state/" and "bank/" cases at the parent of the commit that gave the sweeps
one _StateStore and one table of step programs.  (The device's record — the one-launch step, the chained MH form and the
captured sweeps, which the mirror never runs, with the state and bank cases — was made on an MI355X at that last
parent: tests/test_launch_trace_gpu.py.)"""
import pytest

from tests import launch_trace as L


@pytest.mark.parametrize("name", L.case_names("cpu"))
def test_calls_on_the_mirror_are_the_recorded_ones(hostsim, name):
    L.check_case(hostsim, "cpu", name)


def test_the_record_covers_every_case():
    assert sorted(L.load_golden("cpu")["cases"]) == sorted(L.case_names("cpu"))


def test_the_proxy_leaves_the_backend_as_it_found_it(hostsim):
    c = hostsim.c
    L.trace_case(hostsim, "lgssm/systematic/n700")
    assert hostsim.c is c


def test_refused_combinations_are_refused_as_before(hostsim):
    """the two messages of the ordered multinomials past their form: smc.resample's and BootstrapSweep.prepare's"""
    import torch
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference import smc
    coll = L._collection(L._weights(hostsim, 300))
    for kind in ("multinomial_tiled", "multinomial_sorted"):
        with pytest.raises(NotImplementedError, match=r"n_out = n <= 2\^21; 'multinomial_sorted': n_out = n"):
            smc.resample(G.key(1), coll, kind, n_out=100)
        init, step = workloads.make_lgssm(G)
        with pytest.raises(NotImplementedError, match=r"n <= 2\^21 per GPU \(use 'multinomial'\)"):
            smc.BootstrapSweep(init, step, 2 ** 21 + 1, 2, resample=kind).prepare(G.key(1), torch.zeros(2))
    F = smc._Resampler.form_of
    assert F(smc.SYSTEMATIC, 2 ** 21) == "tiles" and F(smc.SYSTEMATIC, 2 ** 21 + 1) == "prefix"
    assert F(smc.SYSTEMATIC, 2 ** 21 + 1, sweep=True) == "cdf" and F(smc.SYSTEMATIC, 2 ** 31 - 8192) == "cdf"
    assert F(smc.STRATIFIED, 3000, n_out=100) == "cdf" and F(smc.MULTINOMIAL, 3000) == "cdf" and F(smc.SYSTEMATIC, 0) == "cdf"


def test_refused_sharded_combinations_are_refused_as_before(hostsim, monkeypatch):
    """the messages of ShardedBootstrapSweep and sharded_importance_resample, and _ShardRouter.form_of at its edges"""
    import torch
    import genjax_amd as G
    from genjax_amd import _lib, numpy as jnp, workloads
    from genjax_amd.inference import sharded, smc
    from tests import parity
    init, step = workloads.make_lgssm(G)
    ys, Solo = torch.zeros(2), L._Solo
    with pytest.raises(NotImplementedError, match=r"the router takes the ORDERED schemes — systematic, stratified, "
                                                  r"multinomial_sorted \(one-GPU sweeps also offer"):
        sharded.ShardedBootstrapSweep(init, step, 3072, 2, Solo, resample="multinomial")
    with pytest.raises(NotImplementedError, match=r"sharded_importance_resample: the router takes the ordered schemes"):
        sharded.sharded_importance_resample(None, 3072, G.key(1), Solo, kind="multinomial_tiled")
    with pytest.raises(NotImplementedError, match=r"\(fuse_step=True\): needs the fused peer exchange, systematic "
                                                  r"resampling, specialised programs that leave tile statistics, world <= 8"):
        sharded.ShardedBootstrapSweep(init, step, 3072, 2, Solo, fuse_step=True).prepare(G.key(1), ys)
    req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})
    ninit, nstep = workloads.make_nlssm(G)
    with pytest.raises(NotImplementedError, match=r"\(noise_ahead=True, rejuvenate=...\): needs the chained move \+ "
                                                  r"extension program as the one-launch sharded step"):
        sharded.ShardedBootstrapSweep(ninit, nstep, 3072, 2, Solo, rejuvenate=req, step_extra=lambda t: (float(t),),
                                      noise_ahead=True).prepare(G.key(1), ys)
    # (no allocation: refused before prepare() sizes anything by n)
    with pytest.raises(NotImplementedError, match=r"resample='multinomial_sorted' across ranks: n_per_rank \* world < 2\^31"):
        sharded.ShardedBootstrapSweep(init, step, 2 ** 31, 2, Solo, resample="multinomial_sorted").prepare(G.key(1), ys)
    monkeypatch.setenv("GENMI_COMM", "peer")
    D = _lib.PEER_MAX_LEAVES // 2 + 1
    vinit, vstep = parity.make_vec_mh(G, lambda *v: jnp.stack(list(v)), jnp.ones(D))
    sw = sharded.ShardedBootstrapSweep(vinit, vstep, 1024, 2, Solo, always_communicate=True, rejuvenate=req,
                                       step_extra=lambda t: (float(t),), noise_ahead=False)
    with pytest.raises(NotImplementedError, match=r"over the fused peer exchange: at most 32 routed leaves \(GMX_PEER_MAX_LEAVES\)"):
        sw.prepare(G.key(1), ys)
    sw.close()
    F = sharded._ShardRouter.form_of
    for kind in (smc.SYSTEMATIC, smc.STRATIFIED):
        assert F(kind, 2 ** 21, 1) == "tiles" and F(kind, 2 ** 21 + 1, 1) == "cdf"
        assert F(kind, 2 ** 21, 64, peer_capable=True) == "peer" and F(kind, 2 ** 21, 65, peer_capable=True) == "cdf"
        assert F(kind, 2 ** 21 + 1, 1, peer_capable=True) == "cdf" and F(kind, 1024, 64) == "tiles" and F(kind, 1024, 65) == "cdf"
        assert F(kind, 2 ** 21 + 1, 1, sweep=False) == "tiles" and F(kind, 2 ** 21 + 1, 65, sweep=False) == "cdf"
        assert F(kind, 3072, 1, cdf_form=True, peer_capable=True) == "cdf" and F(kind, 3072, 1, cdf_form=True, sweep=False) == "cdf"
    assert F(smc.MULTINOMIAL_SORTED, 3072, 1, peer_capable=True) == "cdf" and F(smc.MULTINOMIAL_SORTED, 3072, 1, sweep=False) == "cdf"
    assert F(smc.MULTINOMIAL_SORTED, 2 ** 31 - 1, 1) == "cdf" and F(smc.MULTINOMIAL_SORTED, 2 ** 31, 1, sweep=False) == "cdf"
    with pytest.raises(NotImplementedError, match=r"n_per_rank \* world < 2\^31"):
        F(smc.MULTINOMIAL_SORTED, 2 ** 25, 64)
