"""gmx_rows_lag_pairs and smc.BootstrapBank(smooth_lag=L, smooth_pairs=True) on the CPU mirror, and the HIP library's refusals
(tests/lag_pairs_checks.py)."""
import pytest

from tests import lag_pairs_checks as C


@pytest.mark.parametrize("n", C.SIZES)
def test_rows_lag_pairs_step_by_step_against_float64(hostsim, n):
    C.check_size(hostsim, n)


@pytest.mark.parametrize("which", ["mirror", "hip"])
def test_library_refuses_bad_arguments_and_sizes_its_workspace(which):
    C.check_refusals_of(C.library(which).c)


@pytest.mark.parametrize("kw", C.BANKS)
def test_bank_is_unchanged_and_its_smoothed_pairs_are_the_reference(hostsim, kw):
    C.check_bank(hostsim, specialize=False, capture=False, **kw)
