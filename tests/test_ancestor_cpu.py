"""gmx_rows_pin, gmx_resample_rows_as and smc.ConditionalBank(ancestor_sampling=True) on the C-ABI's CPU mirror
(tests/hostsim), plus the argument refusals and workspace sizes of the entry points on the HIP library itself (no GPU
involved).  The drivers are in tests/ancestor_checks.py; tests/test_ancestor_gpu.py runs the same ones through the HIP
kernels."""
import ctypes
import os

import pytest

from tests import ancestor_checks as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    return ctypes.CDLL(so)


@pytest.mark.parametrize("D", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 5, 257, 1025])
def test_rows_pin_then_the_multinomial_is_the_pinned_resampler(hostsim, n, D):
    A.check_pin_composition(hostsim, n, 5, D, stride=(n % 2 == 1))


@pytest.mark.parametrize("n", A.AS_SIZES)
def test_rows_as_is_its_definition_and_the_oracles_per_row_path(hostsim, n):
    A.check_as_case(hostsim, n, 5)


@pytest.mark.parametrize("rows", A.AS_COUNTS)
@pytest.mark.parametrize("n", A.AS_COUNT_SIZES)
def test_rows_as_row_counts_around_the_packing(hostsim, n, rows):
    A.check_as_case(hostsim, n, rows, oracle=False)


@pytest.mark.parametrize("n", A.SPECIAL_SIZES)
def test_rows_as_special_ancestor_logits(hostsim, n):
    A.check_as_specials(hostsim, n)


@pytest.mark.parametrize("n", [200, 1500])
def test_rows_as_counts_the_two_kinds_of_empty_rows_apart(hostsim, n):
    A.check_as_no_weight_mass(hostsim, n)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    A.check_refusals_of(_hip_library())


def test_mirror_refuses_the_same_arguments_and_sizes_the_same_workspace(hostsim):
    A.check_refusals_of(hostsim.c)
    assert A.workspace_sizes(hostsim.c) == A.workspace_sizes(_hip_library())


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", A.AB_SIZES)
def test_only_the_pinned_ancestor_moves(hostsim, model, n):
    A.check_only_the_pinned_ancestor_moves(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("n", [200, 1500])
def test_the_pinned_ancestor_is_the_defined_draw(hostsim, n):
    A.check_oracle_replay(hostsim, specialize=False, n=n)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_nothing_retained_is_the_multinomial_bank_bit_for_bit(hostsim, model, n):
    A.check_unconditional(hostsim, model, n, specialize=False)


def test_ancestor_sampling_refusals_name_what_they_refuse(hostsim):
    A.check_refusals(hostsim)


def test_ancestor_sampling_leaves_the_smoothing_distribution_invariant(hostsim):
    A.check_law(hostsim, specialize=False)


def test_ancestor_sampling_moves_the_start_of_the_trajectory(hostsim):
    A.check_mixing(hostsim, specialize=False)
