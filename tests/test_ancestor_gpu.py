"""gmx_rows_pin (k_rows_pin), gmx_resample_rows_as (k_rows_small_as; gmx_resample_rows' chain + k_pick_stats + k_pick_row)
and smc.ConditionalBank(ancestor_sampling=True) through the HIP library on the GPU: the drivers of
tests/ancestor_checks.py, with specialised and interpreted programs, plus the captured form."""
import pytest

from tests import ancestor_checks as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 5, 257, 1025])
def test_rows_pin_then_the_multinomial_is_the_pinned_resampler(gpu, n, D):
    A.check_pin_composition(gpu, n, 5, D, stride=(n % 2 == 1))


@pytest.mark.parametrize("n", A.AS_SIZES)
def test_rows_as_is_its_definition_and_the_oracles_per_row_path(gpu, n):
    A.check_as_case(gpu, n, 5)


@pytest.mark.parametrize("rows", A.AS_COUNTS)
@pytest.mark.parametrize("n", A.AS_COUNT_SIZES)
def test_rows_as_row_counts_around_the_packing(gpu, n, rows):
    A.check_as_case(gpu, n, rows, oracle=False)


@pytest.mark.parametrize("n", A.SPECIAL_SIZES)
def test_rows_as_special_ancestor_logits(gpu, n):
    A.check_as_specials(gpu, n)


@pytest.mark.parametrize("n", [200, 1500])
def test_rows_as_counts_the_two_kinds_of_empty_rows_apart(gpu, n):
    A.check_as_no_weight_mass(gpu, n)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", A.AB_SIZES)
def test_only_the_pinned_ancestor_moves(gpu, model, n, specialize):
    A.check_only_the_pinned_ancestor_moves(gpu, model, n, specialize=specialize)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("n", [200, 1500])
def test_the_pinned_ancestor_is_the_defined_draw(gpu, n, specialize):
    A.check_oracle_replay(gpu, specialize=specialize, n=n)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_nothing_retained_is_the_multinomial_bank_bit_for_bit(gpu, model, n):
    A.check_unconditional(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_captured_ancestor_sweep_replays_under_new_keys_and_paths(gpu, model, n):
    A.check_captured(gpu, model, n)


def test_ancestor_sampling_refusals_name_what_they_refuse(gpu):
    A.check_refusals(gpu)


def test_ancestor_sampling_leaves_the_smoothing_distribution_invariant(gpu):
    A.check_law(gpu, specialize=True)


def test_ancestor_sampling_moves_the_start_of_the_trajectory(gpu):
    A.check_mixing(gpu, specialize=True)
