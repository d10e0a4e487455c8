"""gmx_rows_quantiles and smc.BootstrapBank(quantiles=) on the CPU mirror, and the HIP library's refusals (tests/quantile_checks.py)."""
import pytest

from tests import quantile_checks as Q


@pytest.mark.parametrize("n", Q.SIZES)
def test_rows_quantiles_are_the_integer_reference_and_meet_the_float64_definition(hostsim, n):
    Q.check_size(hostsim, n)


@pytest.mark.parametrize("which", ["mirror", "hip"])
def test_library_refuses_bad_arguments(which):
    Q.check_refusals_of(Q.library(which).c)


@pytest.mark.parametrize("kw", Q.BANKS)
def test_bank_is_unchanged_and_its_quantiles_are_the_reference_and_the_history(hostsim, kw):
    Q.check_bank(hostsim, specialize=False, capture=False, **kw)
