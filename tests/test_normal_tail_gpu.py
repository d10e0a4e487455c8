"""The tail of the normal draw on the MI355X.  On the device gmx_neg_log1m_sq divides without the scale / fix-up
instructions of the IEEE sequence (csrc/gmx_math.h gmx_div_near); v_rcp_f32's bits exist on the device only, so that
stands on the first test here: all 2^23 inputs a draw can have, one call of gmx_std_normal_from_bits, the oracle's bits.
Then gmx_logf's split through a traced one-op program, and one sweep whose background (noise) launch is two-dimensional
and whose particles cross a tile."""
import numpy as np
import pytest
import torch

from oracle import genjax_oracle as O
from tests import normal_tail_checks as C
from tests import parity

pytestmark = pytest.mark.gpu


def test_every_normal_draw_matches_the_oracle(gpu):
    C.hold_normal(gpu, lambda t: t.to(gpu.device))


def test_vm_log_matches_the_oracle_on_the_fixed_set(gpu):
    C.hold_log(lambda t: t.to(gpu.device))


def test_sweep_with_noise_ahead_across_a_tile(gpu):
    """BootstrapSweep, n = 1025, T = 3, noise ahead: state, log-weights, ancestors and log_ml are the oracle's"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    n, T, seed = 1025, 3, 2025
    ys = workloads.lgssm_data(T)
    oi, os_ = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, os_, n, T, ys, O.key(seed))
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T, specialize=True, noise_ahead=True).prepare(G.key(seed), torch.from_numpy(ys))
    assert sw.noise_ahead and sw.p_init.comp.is_specialized() and sw.p_step.comp.is_specialized()
    sw.launch()
    log_ml = sw.log_ml()
    x, lw, anc = sw.state()
    assert np.array_equal(x.cpu().numpy().view(np.uint32), ref["x"].view(np.uint32))
    assert np.array_equal(lw.cpu().numpy().view(np.uint32), ref["lw"].view(np.uint32))
    assert np.array_equal(anc.cpu().numpy() & 0xFFFFFF, ref["anc"])
    assert log_ml == ref["log_ml"], (log_ml, ref["log_ml"])
