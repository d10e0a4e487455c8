"""gmx_rows_moments and smc.BootstrapBank(moments=True) on the CPU mirror, and the HIP library's refusals (tests/moments_checks.py)."""
import pytest

from tests import moments_checks as M


@pytest.mark.parametrize("n", M.SIZES)
def test_rows_moments_against_float64(hostsim, n):
    M.check_size(hostsim, n)


@pytest.mark.parametrize("which", ["mirror", "hip"])
def test_library_refuses_bad_arguments_and_sizes_its_workspace(which):
    M.check_refusals_of(M.library(which).c)


@pytest.mark.parametrize("kw", M.BANKS)
def test_bank_is_unchanged_and_its_moments_are_the_reference_and_the_history(hostsim, kw):
    M.check_bank(hostsim, specialize=False, capture=False, **kw)
