"""The resampling prologue of the one-launch SMC step (csrc/gmx_offspring.h) after the pass that went looking for vector
instructions the result does not need: the statistics-table pass split by workgroup-uniform row conditions (rows wholly in
front of / behind the workgroup's tile take no per-lane compare; only the table's last row is re-masked), and the lower
slot edge of waves 1 .. 3 taken from the wave before through LDS for every kind (only wave 0 evaluates its own).  The
third part of that pass — handing the packed fixed-point weights from one launch's epilogue to the next one's prologue —
was measured slower and is not in the tree; the cases it asked for stay, they cost nothing.

Both changes are the same integers by construction, so every case is held to the Python oracle bit for bit — particles,
ancestors, integer totals, log-weights and the evidence (tests/parity.check_lgssm_sweep, parity.oracle_bootstrap_sweep):
nothing is compared with another run of the code under test.  Sizes: the smallest at which each change takes another path."""
import numpy as np
import pytest
import torch

from tests import parity

TILE = 1024
ROW = 256 * TILE          # particles one row of the tile-statistics table covers (256 tiles: one entry per thread)


def _exact(res):
    assert res["ancestors_equal"] and res["x_equal"] and res["totals_equal"], res
    assert res["lw_max_abs_diff"] == 0.0, res
    assert res["log_ml"] == res["log_ml_oracle"], res


# n = 1024: one tile, one table row, wave 0 .. 3 of ONE workgroup (the lower edge through LDS, nothing else);
# 3 * 1024 + 17: a partial last tile (sources past n own no slot); 256 * 1024: exactly one whole table row (no clamp, no
# re-masking); 257 * 1024 + 1: two rows, the second with two live lanes — first_tile crosses the row boundary at tiles
# 255 .. 257 (rows wholly in front of / straddling / behind the workgroup's tile)
@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("n", [TILE, 3 * TILE + 17, ROW, ROW + TILE + 1])
def test_one_launch_step_is_bit_exact(gpu, n, capture):
    _exact(parity.check_lgssm_sweep(n=n, T=4, seed=20 + n % 7, capture=capture, specialize=True, fuse_resample=True))


@pytest.mark.gpu
def test_one_launch_step_with_noise_ahead(gpu):
    _exact(parity.check_lgssm_sweep(n=ROW + TILE + 1, T=4, seed=5, capture=True, specialize=True, fuse_resample=True,
                                    noise_ahead=True))


@pytest.mark.gpu
def test_stratified_takes_the_lower_edge_through_lds(gpu):
    """the standalone tile resampler (two launches per step): same body, same table pass"""
    _exact(parity.check_lgssm_sweep(n=ROW + TILE + 1, T=4, seed=6, specialize=True, resample="stratified"))


@pytest.mark.gpu
def test_two_launch_and_interpreted_forms(gpu, monkeypatch):
    """two launches per step (the standalone resampler), and the interpreter (GENMI_JIT=0: no specialised kernel)"""
    n = 3 * TILE + 17
    _exact(parity.check_lgssm_sweep(n=n, T=4, seed=8, specialize=True, fuse_resample=False))
    monkeypatch.setenv("GENMI_JIT", "0")
    _exact(parity.check_lgssm_sweep(n=n, T=4, seed=8, specialize=True))


# ---- whole tiles without mass ------------------------------------------------------------------------------------------
ZM_N, ZM_T, ZM_SEED, ZM_W = 4 * TILE, 4, 16, 0.05
ZM_YS = np.array([2.7, 2.75, 2.75, 2.75], np.float32)


def _zero_mass_models(g):
    """an observed uniform whose support moves with the state: -inf for every particle further than ZM_W from y.  A handful
    of particles survive step 0, each owning a contiguous block of slots, and the state barely moves: whole 1024-particle
    tiles then stand outside the next step's support"""
    @g.gen
    def init():
        x = g.normal(0.0, 1.0) @ "x"
        g.uniform(x - ZM_W, x + ZM_W) @ "y"
        return x

    @g.gen
    def step(x0):
        x = g.normal(x0, 0.001) @ "x"
        g.uniform(x - ZM_W, x + ZM_W) @ "y"
        return x
    return init, step


def _check_zero_mass_sweep(**kw):
    import genjax_amd as G
    from genjax_amd.inference.smc import BootstrapSweep
    from oracle import genjax_oracle as O
    n, T = ZM_N, ZM_T
    ref = parity.oracle_bootstrap_sweep(*_zero_mass_models(O), n, T, ZM_YS, O.key(ZM_SEED))
    # what the case is for, from the oracle's weights: at steps the NEXT launch's prologue resamples (t < T - 1) there are
    # tiles with no mass at all beside tiles with mass, and a tile that is only partly dead
    dead = [[b for b in range(n // TILE) if not np.isfinite(h["lw"][b * TILE:(b + 1) * TILE]).any()] for h in ref["hist"]]
    assert all(0 < len(dead[t]) < n // TILE for t in (0, 1)), dead
    assert any(0 < np.isfinite(h["lw"][b * TILE:(b + 1) * TILE]).sum() < TILE for h in ref["hist"][:T - 1] for b in range(n // TILE))
    assert all(int(h["total"]) > 0 for h in ref["hist"])
    init, step = _zero_mass_models(G)
    sw = BootstrapSweep(init, step, n, T, **kw).prepare(G.key(ZM_SEED), torch.from_numpy(ZM_YS))
    sw.launch()
    log_ml = sw.log_ml()
    x, lw, anc = sw.state()
    assert np.array_equal(anc.cpu().numpy(), ref["anc"])
    assert np.array_equal(x.cpu().numpy(), ref["x"])
    assert np.array_equal(lw.cpu().numpy(), ref["lw"])
    assert np.array_equal(sw.totals.cpu().numpy().view(np.uint64), np.array([h["total"] for h in ref["hist"]], dtype=np.uint64))
    assert log_ml == ref["log_ml"]
    return sw


@pytest.mark.gpu
def test_tiles_without_mass_in_the_one_launch_step(gpu):
    assert _check_zero_mass_sweep(specialize=True, fuse_resample=True).fuse


def test_tiles_without_mass_on_the_mirror(hostsim):
    """the same driver on the C-ABI's CPU mirror (one-launch form): the case and its oracle twin agree"""
    _check_zero_mass_sweep(specialize=True, fuse_resample=True)
