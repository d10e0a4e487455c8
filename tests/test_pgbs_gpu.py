"""gmx_pick_rows_take (k_rows_small_take; k_pick_stats + k_pick_row + k_rows_take) and smc.ConditionalBank.draw(key,
backward=True) through the HIP library on the GPU: the drivers of tests/pgbs_checks.py, with specialised and interpreted
programs, plus the captured form."""
import pytest

from tests import ancestor_checks as A
from tests import pgbs_checks as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", P.TAKE_SIZES)
def test_pick_rows_take_is_its_definition_and_the_oracles_pick(gpu, n):
    P.check_take_case(gpu, n, 5)


@pytest.mark.parametrize("rows", P.TAKE_COUNTS)
@pytest.mark.parametrize("n", P.TAKE_COUNT_SIZES)
def test_pick_rows_take_row_counts_around_the_packing(gpu, n, rows):
    P.check_take_case(gpu, n, rows, oracle=False, full=False)


@pytest.mark.parametrize("n", P.SPECIAL_SIZES)
def test_pick_rows_take_special_logits(gpu, n):
    P.check_take_specials(gpu, n)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("ancestors", [False, True])
@pytest.mark.parametrize("retained", [False, True])
@pytest.mark.parametrize("n", P.PB_SIZES)
def test_backward_draw_is_the_defined_draw(gpu, n, retained, ancestors, specialize):
    P.check_oracle_replay(gpu, specialize=specialize, n=n, retained=retained, ancestors=ancestors)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_backward_draw_ends_where_the_lineage_draw_ends(gpu, model, n):
    P.check_last_state(gpu, model, n, specialize=True)


def test_backward_draw_of_one_step_is_the_draw(gpu):
    P.check_one_step(gpu)


def test_backward_draw_tuple_state_and_refusals(gpu):
    P.check_pair_refusals(gpu)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_retain_takes_a_backward_draw(gpu, model, n):
    P.check_retain(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("n", [200, 1500])
def test_captured_bank_survives_a_backward_draw(gpu, model, n):
    P.check_captured(gpu, model, n)


@pytest.mark.parametrize("n", [200, 1500])
def test_backward_draw_without_mass_names_the_step(gpu, n):
    P.check_no_mass(gpu, n)


@pytest.mark.parametrize("ancestors", [False, True])
def test_backward_simulation_leaves_the_smoothing_distribution_invariant(gpu, ancestors):
    P.check_law(gpu, specialize=True, ancestors=ancestors)


def test_backward_simulation_moves_the_start_of_the_trajectory(gpu):
    P.check_mixing(gpu, specialize=True)
