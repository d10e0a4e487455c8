"""gmx_rows_quantiles' kernel and smc.BootstrapBank(quantiles=), captured too, on the GPU (tests/quantile_checks.py)."""
import pytest

from tests import quantile_checks as Q

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", Q.SIZES)
def test_rows_quantiles_are_the_integer_reference_and_meet_the_float64_definition(gpu, n):
    Q.check_size(gpu, n)


@pytest.mark.parametrize("kw", Q.BANKS)
def test_bank_is_unchanged_and_its_quantiles_are_the_reference_and_the_history(gpu, kw):
    Q.check_bank(gpu, specialize=True, capture=True, **kw)
