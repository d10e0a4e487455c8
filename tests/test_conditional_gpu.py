"""gmx_resample_rows_pinned (k_rows_small_pinned; k_rows_pin + k_pick_stats + k_rows_tile + k_rows_mn) and
smc.ConditionalBank through the HIP library on the GPU: the drivers of tests/conditional_checks.py, with specialised
programs, plus the captured form."""
import pytest

from tests import conditional_checks as C

pytestmark = pytest.mark.gpu
MODELS = ["lgssm", "tracker"]


@pytest.mark.parametrize("n", C.PIN_SIZES)
def test_pinned_rows_match_the_oracles_per_row_path_on_the_pinned_weights(gpu, n):
    C.check_pinned_case(gpu, "normal%d" % n)


@pytest.mark.parametrize("rows", C.PIN_COUNTS)
def test_pinned_rows_row_counts_around_the_packing(gpu, rows):
    C.check_pinned_case(gpu, "count%d" % rows, D=3)


@pytest.mark.parametrize("D", C.PIN_DEPTHS)
@pytest.mark.parametrize("stride", [False, True])
@pytest.mark.parametrize("name", ["normal255", "normal1025"])
def test_pinned_rows_layouts_and_state_depths(gpu, name, stride, D):
    C.check_pinned_case(gpu, name, D=D, stride=stride)


@pytest.mark.parametrize("name", ["normal255", "normal2051"])
def test_pinned_rows_special_pins(gpu, name):
    C.check_pinned_specials(gpu, name)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_nothing_retained_is_the_multinomial_bank_bit_for_bit(gpu, model, n):
    C.check_unconditional(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_conditional_sweep_pins_the_last_slot_of_every_chain(gpu, model, n):
    C.check_structure(gpu, model, n, specialize=True)


def test_conditional_sweep_equals_an_oracle_loop_per_chain(gpu):
    C.check_oracle_replay(gpu, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_conditional_rows_are_position_independent(gpu, model, n):
    C.check_position_independence(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_draw_is_a_pick_and_a_walk_through_the_record(gpu, model, n):
    C.check_draw(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_model_computed_weights_are_the_recorded_ones(gpu, model, n):
    C.check_model_weights(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_run_is_the_documented_loop(gpu, model, n):
    C.check_run(gpu, model, n, specialize=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_captured_conditional_sweep_replays_under_new_keys_and_paths(gpu, model, n):
    C.check_captured(gpu, model, n)


def test_conditional_refusals_name_what_they_refuse(gpu):
    C.check_refusals(gpu)


def test_conditional_smc_leaves_the_smoothing_distribution_invariant(gpu):
    C.check_law(gpu, specialize=True)
