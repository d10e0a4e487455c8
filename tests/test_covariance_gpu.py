"""gmx_rows_covariance's kernels and smc.BootstrapBank(covariance=True), captured too, on the GPU (tests/covariance_checks.py)."""
import pytest

from tests import covariance_checks as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", C.SIZES)
def test_rows_covariance_against_float64_and_the_mirror(gpu, n):
    C.check_size(gpu, n)


@pytest.mark.parametrize("kw", C.BANKS)
def test_bank_is_unchanged_and_its_covariance_is_the_reference_and_the_moments(gpu, kw):
    C.check_bank(gpu, specialize=True, capture=True, **kw)
