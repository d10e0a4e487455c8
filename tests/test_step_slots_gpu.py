"""The ancestor tag folded into the marks of the fused resampler (csrc/gmx_offspring.h: a source's mark is written as
{tag | index}, so the max-scan, the carries and the stores OR nothing) and the specialised chain kernels compiled without
the SLP vectoriser, at the shapes where the fold can go wrong: a tile that owns more than 2048 slots (a second fill pass,
a range that continues at mark 0), a one-particle tile behind a tile whose slots nearly all come from one source (the
tail stores), a step without any mass (the explicit `(n - 1) | tag` words, polled by the next step), and a sweep long
enough for the tags 1 .. 255 to wrap.  BootstrapSweep on the LGSSM against parity.oracle_bootstrap_sweep, bit for bit:
state, log-weights, ancestors (the index field of a tagged word), integer totals, log_ml."""
import numpy as np
import pytest
import torch

from oracle import genjax_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu

_KEY = 11
_REF = {}


def _ref(n, ys):
    k = (n, ys.tobytes())
    if k not in _REF:
        from genjax_amd import workloads
        oi, os_ = workloads.make_lgssm(O)
        ref = parity.oracle_bootstrap_sweep(oi, os_, n, len(ys), ys, O.key(_KEY))
        # BootstrapSweep.log_ml is np.sum over the T per-step terms (smc.evidence_terms says so), the oracle's sweep adds them
        # one after the other: the same float below 8 terms, where np.sum is sequential too, and not above (T = 260: pairwise).
        # The reference is the ORACLE's terms, summed in the order the product states.
        terms = []
        for h in ref["hist"]:
            shift = O.weight_cdf(h["lw"])[3]
            with np.errstate(divide="ignore"):
                terms.append(O.log_ml_increment(h["M"], h["total"], shift, n))
        ref["log_ml_sum"] = float(np.sum(np.array(terms, np.float64)))
        if len(ys) < 8:
            assert ref["log_ml_sum"] == ref["log_ml"]
        _REF[k] = ref
    return _REF[k]


def _owned(anc):
    """slots per source that owns any, largest first"""
    return np.sort(np.bincount(anc))[::-1]


def _hold(n, ys, forms):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    T = len(ys)
    init, step = workloads.make_lgssm(G)
    ref = _ref(n, ys)
    for fuse, capture in forms:
        what = dict(n=n, fuse=fuse, capture=capture)
        sw = BootstrapSweep(init, step, n, T, specialize=True, fuse_resample=fuse).prepare(G.key(_KEY), torch.from_numpy(ys))
        assert sw.fuse == fuse, what
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
        assert log_ml == ref["log_ml_sum"], (what, log_ml, ref["log_ml_sum"])
    return ref


_ALL = [(fuse, capture) for fuse in (True, False) for capture in (False, True)]


def test_tile_owning_more_than_a_fill_pass(gpu):
    """n = 5000, an observation at 60 sigma at step 1: one source owns more than 2048 slots, so its tile's fill loop
    takes a second pass (base != T0) in which the range continues at mark 0"""
    ys = np.array([0.3, 60.0, -0.2, 0.1], np.float32)
    ref = _hold(5000, ys, _ALL)
    own = _owned(ref["hist"][1]["anc"])
    assert own[0] > 2048 and np.count_nonzero(own) >= 2, own[:4]          # (the case is the one it says it is)


def test_tail_stores(gpu):
    """n = 2049: a full tile and a one-particle tile, nearly all slots from one source — the last thread groups of the
    owning tile and the one-particle tile store word by word"""
    ys = np.array([0.3, 40.0, -0.2, 0.1], np.float32)
    ref = _hold(2049, ys, _ALL)
    own = _owned(ref["hist"][1]["anc"])
    assert own[0] > 2000 and np.count_nonzero(own) >= 2, own[:4]


def test_no_mass(gpu):
    """an infinite observation at step 1: every weight is -inf, the total is 0, every slot maps to the last particle
    (words written as `(n - 1) | tag`, which the next step's workgroups poll), log_ml is -inf, step 2 has mass again"""
    n = 5000
    ys = np.array([0.3, np.inf, -0.2, 0.1], np.float32)
    ref = _hold(n, ys, _ALL)
    assert int(ref["hist"][1]["total"]) == 0 and np.all(ref["hist"][1]["anc"] == n - 1)
    assert int(ref["hist"][2]["total"]) > 0 and ref["log_ml"] == -np.inf


def test_whole_and_clamped_rows_of_the_tile_table(gpu):
    """n = 257 * 1024 + 1: 258 tiles, so the prologue's table pass reads row 0 of the tile table whole (scalar row base + a
    32-bit offset) and row 1 clamped (two entries), tiles 256 and 257 have a whole row in front of them, and both halves of
    the one-tree pair of wave sums carry mass"""
    from genjax_amd import workloads
    _hold(257 * 1024 + 1, workloads.lgssm_data(3), [(True, False), (True, True), (False, False)])


def test_tag_wrap(gpu):
    """T = 260 steps in one captured, fused sweep over a tile and a one-particle tile: the tags 1 .. 255 cycle"""
    from genjax_amd import workloads
    _hold(1025, workloads.lgssm_data(260), [(True, True)])
