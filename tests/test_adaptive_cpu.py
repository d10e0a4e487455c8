"""gmx_resample_rows_ess and smc.BootstrapBank(ess_threshold=) on the C-ABI's CPU mirror (tests/hostsim), plus the argument
refusals and workspace sizes of the entry point on the HIP library itself (no GPU involved).  The drivers are in
tests/adaptive_checks.py; tests/test_adaptive_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import adaptive_checks as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    return ctypes.CDLL(so)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", A.ESS_SIZES)
def test_rows_ess_is_its_definition(hostsim, n, kind):
    A.check_case(hostsim, "sized", n, kind, need_both=n > 1)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("rows", A.ESS_COUNTS)
def test_rows_ess_row_counts_around_the_packing(hostsim, rows, kind):
    A.check_case(hostsim, "count", rows, kind, need_both=rows > 1, strides=(None,))


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("name", list(A.SHAPE_CASES))
def test_rows_ess_row_shapes_on_both_sides_of_the_threshold(hostsim, name, kind):
    A.check_case(hostsim, "shape", name, kind)


@pytest.mark.parametrize("k", ["1", "3", "n"])
@pytest.mark.parametrize("n", [5, 300, 1024])
def test_rows_ess_boundary_is_exact(hostsim, n, k):
    A.check_boundary(hostsim, n, n if k == "n" else int(k), "systematic")


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", [5, 257, 1024])
def test_rows_ess_never_and_always(hostsim, n, kind):
    A.check_extremes(hostsim, n, kind)


@pytest.mark.parametrize("n", [64, 513])
def test_rows_ess_row_without_mass(hostsim, n):
    A.check_no_mass(hostsim, n, "stratified")


@pytest.mark.parametrize("n", [64, 600])
def test_rows_ess_carry_with_infinities_and_nans(hostsim, n):
    A.check_special_carry(hostsim, n, "multinomial")


def test_integer_ess_against_float64(hostsim):
    A.check_ess_against_float64(hostsim)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    A.check_refusals_of(_hip_library())


def test_mirror_refuses_the_same_arguments_and_sizes_the_same_workspace(hostsim):
    A.check_refusals_of(hostsim.c)
    assert A.workspace_sizes(hostsim.c) == A.workspace_sizes(_hip_library())


@pytest.mark.parametrize("n", A.SW_SIZES)
def test_threshold_above_one_is_the_plain_bank_bit_for_bit(hostsim, n):
    A.check_always_is_the_plain_bank(hostsim, n, specialize=False)


@pytest.mark.parametrize("n", A.SW_SIZES)
def test_mid_threshold_sweep_is_the_composed_definition(hostsim, n):
    A.check_mid_threshold(hostsim, n, specialize=False)


@pytest.mark.parametrize("n", A.SW_SIZES)
def test_rows_resampled_at_every_step_are_the_plain_banks(hostsim, n):
    A.check_rows_resampled_at_every_step(hostsim, n, specialize=False)


@pytest.mark.parametrize("n", A.SW_SIZES)
def test_threshold_zero_never_resamples(hostsim, n):
    A.check_never(hostsim, n, specialize=False)


def test_adaptive_refusals_name_what_they_refuse(hostsim):
    A.check_api_refusals(hostsim)


@pytest.mark.parametrize("tau", [0.5, 0.0])
def test_adaptive_evidence_is_unbiased(hostsim, tau):
    A.check_law(hostsim, specialize=False, tau=tau)
