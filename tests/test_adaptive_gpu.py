"""gmx_resample_rows_ess (k_rows_small_ess) and smc.BootstrapBank(ess_threshold=) through the HIP library on the GPU: the
drivers of tests/adaptive_checks.py, with specialised and interpreted programs, plus the captured form."""
import pytest

from tests import adaptive_checks as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", A.ESS_SIZES)
def test_rows_ess_is_its_definition(gpu, n, kind):
    A.check_case(gpu, "sized", n, kind, need_both=n > 1)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("rows", A.ESS_COUNTS)
def test_rows_ess_row_counts_around_the_packing(gpu, rows, kind):
    A.check_case(gpu, "count", rows, kind, need_both=rows > 1, strides=(None,))


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("name", list(A.SHAPE_CASES))
def test_rows_ess_row_shapes_on_both_sides_of_the_threshold(gpu, name, kind):
    A.check_case(gpu, "shape", name, kind)


@pytest.mark.parametrize("k", ["1", "3", "n"])
@pytest.mark.parametrize("n", [5, 300, 1024])
def test_rows_ess_boundary_is_exact(gpu, n, k):
    A.check_boundary(gpu, n, n if k == "n" else int(k), "systematic")


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", [5, 257, 1024])
def test_rows_ess_never_and_always(gpu, n, kind):
    A.check_extremes(gpu, n, kind)


@pytest.mark.parametrize("n", [64, 513])
def test_rows_ess_row_without_mass(gpu, n):
    A.check_no_mass(gpu, n, "stratified")


@pytest.mark.parametrize("n", [64, 600])
def test_rows_ess_carry_with_infinities_and_nans(gpu, n):
    A.check_special_carry(gpu, n, "multinomial")


def test_integer_ess_against_float64(gpu):
    A.check_ess_against_float64(gpu)


def test_device_refuses_bad_arguments_before_any_launch(gpu):
    A.check_refusals_of(gpu.c)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", A.SW_SIZES)
def test_threshold_above_one_is_the_plain_bank_bit_for_bit(gpu, n, specialize):
    A.check_always_is_the_plain_bank(gpu, n, specialize=specialize)


@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", A.SW_SIZES)
def test_mid_threshold_sweep_is_the_composed_definition(gpu, n, specialize, capture):
    A.check_mid_threshold(gpu, n, specialize=specialize, capture=capture)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", A.SW_SIZES)
def test_rows_resampled_at_every_step_are_the_plain_banks(gpu, n, specialize):
    A.check_rows_resampled_at_every_step(gpu, n, specialize=specialize)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", A.SW_SIZES)
def test_threshold_zero_never_resamples(gpu, n, specialize):
    A.check_never(gpu, n, specialize=specialize)


def test_adaptive_refusals_name_what_they_refuse(gpu):
    A.check_api_refusals(gpu)


@pytest.mark.parametrize("tau", [0.5, 0.0])
def test_adaptive_evidence_is_unbiased(gpu, tau):
    A.check_law(gpu, specialize=True, tau=tau)
