"""gmx_rows_moments' kernels and smc.BootstrapBank(moments=True), captured too, on the GPU (tests/moments_checks.py)."""
import pytest

from tests import moments_checks as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", M.SIZES)
def test_rows_moments_against_float64_and_the_mirror(gpu, n):
    M.check_size(gpu, n)


@pytest.mark.parametrize("kw", M.BANKS)
def test_bank_is_unchanged_and_its_moments_are_the_reference_and_the_history(gpu, kw):
    M.check_bank(gpu, specialize=True, capture=True, **kw)
