"""The tagged fill of the one-launch sharded step (csrc/gmx_shard_fill.h: the body a specialised site program of a sharded
sweep runs first; its marks are bare source indices, the tag is ORed in at the stores) at the shapes where the fill through
LDS (gmx_fill_pass, csrc/gmx_resample.h) can go wrong: a tile that owns more than 2048 slots (a second pass, which zeroes
the marks without a barrier in front and in which the range continues at mark 0), a one-particle tile behind a tile whose
slots nearly all come from one source (the word-by-word tail stores), and a step without any mass (the explicit
`(n - 1) | tag` words, polled by the next step).  tests/test_step_slots_gpu.py holds the single-GPU body to the same cases.
ShardedBootstrapSweep on the LGSSM at world size 1 over the fused peer exchange, eager and captured, against
parity.oracle_bootstrap_sweep, bit for bit: the resampled state, the integer totals, log_ml."""
import numpy as np
import pytest
import torch

from oracle import genjax_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu

_KEY = 11


class _Solo:
    @staticmethod
    def get_rank(): return 0
    @staticmethod
    def get_world_size(): return 1


def _owned(anc):
    """slots per source that owns any, largest first"""
    return np.sort(np.bincount(anc))[::-1]


def _hold(monkeypatch, n, ys):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.comm import PeerComm
    from genjax_amd.inference.sharded import ShardedBootstrapSweep
    monkeypatch.setenv("GENMI_COMM", "peer")
    T = len(ys)
    oi, os_ = workloads.make_lgssm(O)
    ref = parity.oracle_bootstrap_sweep(oi, os_, n, T, ys, O.key(_KEY))
    totals = np.array([h["total"] for h in ref["hist"]], dtype=np.uint64)
    init, step = workloads.make_lgssm(G)
    sw = ShardedBootstrapSweep(init, step, n, T, _Solo, specialize=True, always_communicate=True).prepare(
        G.key(_KEY), torch.from_numpy(ys))
    try:
        assert isinstance(sw.cx, PeerComm) and sw.peer_mode
        assert sw.fuse_sh, n                                               # (the case is the one it says it is)

        def check(what):
            assert np.array_equal(sw.state().cpu().numpy(), ref["x"][ref["anc"]]), what
            assert np.array_equal(sw.totals.cpu().numpy().view(np.uint64), totals), what
            assert sw.log_ml() == ref["log_ml"], (what, sw.log_ml(), ref["log_ml"])
            assert int(sw.peer_status.item()) == 0, what
        sw.launch()
        check("eager")
        sw.capture()
        sw.launch()
        sw.finish()
        check("captured")
    finally:
        sw.close()
    return ref


def test_tile_owning_more_than_a_fill_pass(gpu, monkeypatch):
    """n = 5000, an observation at 60 sigma at step 1: one source owns more than 2048 slots (3224, then 1626 and 150), so its
    tile's fill loop takes a second pass"""
    ref = _hold(monkeypatch, 5000, np.array([0.3, 60.0, -0.2, 0.1], np.float32))
    own = _owned(ref["hist"][1]["anc"])
    assert own[0] > 2048 and np.count_nonzero(own) >= 2, own[:4]


def test_tail_stores(gpu, monkeypatch):
    """n = 2049: a full tile and a one-particle tile, 2046 of the 2049 slots from one source — the last thread groups of the
    owning tile and the one-particle tile store word by word"""
    ref = _hold(monkeypatch, 2049, np.array([0.3, 40.0, -0.2, 0.1], np.float32))
    own = _owned(ref["hist"][1]["anc"])
    assert own[0] > 2000 and np.count_nonzero(own) >= 2, own[:4]


def test_no_mass(gpu, monkeypatch):
    """an infinite observation at step 1: every weight is -inf, the total is 0, every slot maps to the last particle, log_ml
    is -inf, step 2 has mass again"""
    n = 5000
    ref = _hold(monkeypatch, n, np.array([0.3, np.inf, -0.2, 0.1], np.float32))
    assert int(ref["hist"][1]["total"]) == 0 and np.all(ref["hist"][1]["anc"] == n - 1)
    assert int(ref["hist"][2]["total"]) > 0 and ref["log_ml"] == -np.inf
