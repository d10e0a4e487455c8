"""gmx_pick_rows_take and smc.ConditionalBank.draw(key, backward=True) on the C-ABI's CPU mirror (tests/hostsim), plus the
argument refusals and workspace sizes of the entry point on the HIP library itself (no GPU involved).  The drivers are in
tests/pgbs_checks.py; tests/test_pgbs_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import ancestor_checks as A
from tests import pgbs_checks as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    return ctypes.CDLL(so)


@pytest.mark.parametrize("n", P.TAKE_SIZES)
def test_pick_rows_take_is_its_definition_and_the_oracles_pick(hostsim, n):
    P.check_take_case(hostsim, n, 5)


@pytest.mark.parametrize("rows", P.TAKE_COUNTS)
@pytest.mark.parametrize("n", P.TAKE_COUNT_SIZES)
def test_pick_rows_take_row_counts_around_the_packing(hostsim, n, rows):
    P.check_take_case(hostsim, n, rows, oracle=False, full=False)


@pytest.mark.parametrize("n", P.SPECIAL_SIZES)
def test_pick_rows_take_special_logits(hostsim, n):
    P.check_take_specials(hostsim, n)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    P.check_refusals_of(_hip_library())


def test_mirror_refuses_the_same_arguments_and_sizes_the_same_workspace(hostsim):
    P.check_refusals_of(hostsim.c)
    assert P.workspace_sizes(hostsim.c) == P.workspace_sizes(_hip_library())


@pytest.mark.parametrize("ancestors", [False, True])
@pytest.mark.parametrize("retained", [False, True])
@pytest.mark.parametrize("n", P.PB_SIZES)
def test_backward_draw_is_the_defined_draw(hostsim, n, retained, ancestors):
    P.check_oracle_replay(hostsim, specialize=False, n=n, retained=retained, ancestors=ancestors)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_backward_draw_ends_where_the_lineage_draw_ends(hostsim, model, n):
    P.check_last_state(hostsim, model, n, specialize=False)


def test_backward_draw_of_one_step_is_the_draw(hostsim):
    P.check_one_step(hostsim)


def test_backward_draw_tuple_state_and_refusals(hostsim):
    P.check_pair_refusals(hostsim)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_retain_takes_a_backward_draw(hostsim, model, n):
    P.check_retain(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("n", [200, 1500])
def test_backward_draw_without_mass_names_the_step(hostsim, n):
    P.check_no_mass(hostsim, n)


@pytest.mark.parametrize("ancestors", [False, True])
def test_backward_simulation_leaves_the_smoothing_distribution_invariant(hostsim, ancestors):
    P.check_law(hostsim, specialize=False, ancestors=ancestors)


def test_backward_simulation_moves_the_start_of_the_trajectory(hostsim):
    P.check_mixing(hostsim, specialize=False)
