"""gmx_smooth_back's kernels and smc.SweepHistory.marginal_smooth on the GPU (tests/smooth_checks.py)."""
import pytest

from tests import smooth_checks as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", S.SIZES)
def test_smooth_back_against_float64_twice_the_same_bits(gpu, n):
    S.check_size(gpu, n)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("model", ["lgssm", "tracker"])
def test_marginal_smooth_is_the_float64_recursion(gpu, model, n, specialize):
    S.check_marginal(gpu, model, n, specialize)
