"""gmx_rows_covariance and smc.BootstrapBank(covariance=True) on the CPU mirror, and the HIP library's refusals
(tests/covariance_checks.py)."""
import pytest

from tests import covariance_checks as C


@pytest.mark.parametrize("n", C.SIZES)
def test_rows_covariance_against_float64(hostsim, n):
    C.check_size(hostsim, n)


@pytest.mark.parametrize("which", ["mirror", "hip"])
def test_library_refuses_bad_arguments_and_sizes_its_workspace(which):
    C.check_refusals_of(C.library(which).c)


@pytest.mark.parametrize("kw", C.BANKS)
def test_bank_is_unchanged_and_its_covariance_is_the_reference_and_the_moments(hostsim, kw):
    C.check_bank(hostsim, specialize=False, capture=False, **kw)
