"""gmx_smooth_back and smc.SweepHistory.marginal_smooth on the CPU mirror, and both libraries' refusals (tests/smooth_checks.py)."""
import pytest

from tests import smooth_checks as S


@pytest.mark.parametrize("n", S.SIZES)
def test_smooth_back_against_float64(hostsim, n):
    S.check_size(hostsim, n)


def test_both_libraries_refuse_bad_arguments_alike():
    S.check_refusals_of(S.library("hip").c, S.library("mirror").c)


@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("model", ["lgssm", "tracker"])
def test_marginal_smooth_is_the_float64_recursion(hostsim, model, n):
    S.check_marginal(hostsim, model, n, specialize=False)
