"""The C-ABI calls of every sweep form and one-off resampling (tests/launch_trace.py) against the record made at the
parent of the commit that gave inference/smc.py ONE resampling launcher and ONE step loop
(tests/golden/make_launch_trace.py): same calls, same order, same integers, same sharing of buffers — on the C-ABI's
CPU mirror.  (The same cases on the HIP library, plus the captured form, need a record made on the device at that
parent commit: `make_launch_trace.py --gpu` writes it; none is committed yet.)"""
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
