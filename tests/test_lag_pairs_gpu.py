"""gmx_rows_lag_pairs' kernels and smc.BootstrapBank(smooth_lag=L, smooth_pairs=True), captured too, on the GPU
(tests/lag_pairs_checks.py)."""
import pytest

from tests import lag_pairs_checks as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", C.SIZES)
def test_rows_lag_pairs_step_by_step_against_float64_and_the_mirror(gpu, n):
    C.check_size(gpu, n)


@pytest.mark.parametrize("kw", C.BANKS)
def test_bank_is_unchanged_and_its_smoothed_pairs_are_the_reference(gpu, kw):
    C.check_bank(gpu, specialize=True, capture=True, **kw)
