"""gmx_resample_rows_pinned and smc.ConditionalBank on the C-ABI's CPU mirror (tests/hostsim), plus the argument refusals of
the entry point on the HIP library itself (no GPU involved).  The drivers are in tests/conditional_checks.py;
tests/test_conditional_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import conditional_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["lgssm", "tracker"]


@pytest.mark.parametrize("n", C.PIN_SIZES)
def test_pinned_rows_match_the_oracles_per_row_path_on_the_pinned_weights(hostsim, n):
    C.check_pinned_case(hostsim, "normal%d" % n)


@pytest.mark.parametrize("rows", C.PIN_COUNTS)
def test_pinned_rows_row_counts_around_the_packing(hostsim, rows):
    C.check_pinned_case(hostsim, "count%d" % rows, D=3)


@pytest.mark.parametrize("D", C.PIN_DEPTHS)
@pytest.mark.parametrize("stride", [False, True])
@pytest.mark.parametrize("name", ["normal255", "normal1025"])
def test_pinned_rows_layouts_and_state_depths(hostsim, name, stride, D):
    C.check_pinned_case(hostsim, name, D=D, stride=stride)


@pytest.mark.parametrize("name", ["normal255", "normal2051"])
def test_pinned_rows_special_pins(hostsim, name):
    C.check_pinned_specials(hostsim, name)


def test_pinned_rows_rejects_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(so)
    lib.gmx_last_error.restype = ctypes.c_char_p
    calls, _keep = C.pinned_refusal_calls()
    for args, names in calls:
        rc = lib.gmx_resample_rows_pinned(*args)
        assert rc != 0, args
        msg = lib.gmx_last_error()
        assert b"gmx_resample_rows_pinned" in msg and names in msg, (msg, names)


def test_pinned_rows_mirror_refuses_the_same_arguments(hostsim):
    calls, _keep = C.pinned_refusal_calls()
    for args, _ in calls:
        assert hostsim.c.gmx_resample_rows_pinned(*args) != 0, args


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_nothing_retained_is_the_multinomial_bank_bit_for_bit(hostsim, model, n):
    C.check_unconditional(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_conditional_sweep_pins_the_last_slot_of_every_chain(hostsim, model, n):
    C.check_structure(hostsim, model, n, specialize=False)


def test_conditional_sweep_equals_an_oracle_loop_per_chain(hostsim):
    C.check_oracle_replay(hostsim, specialize=False)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_conditional_rows_are_position_independent(hostsim, model, n):
    C.check_position_independence(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_draw_is_a_pick_and_a_walk_through_the_record(hostsim, model, n):
    C.check_draw(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_model_computed_weights_are_the_recorded_ones(hostsim, model, n):
    C.check_model_weights(hostsim, model, n, specialize=False)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.CB_SIZES)
def test_run_is_the_documented_loop(hostsim, model, n):
    C.check_run(hostsim, model, n, specialize=False)


def test_conditional_refusals_name_what_they_refuse(hostsim):
    C.check_refusals(hostsim)


def test_conditional_smc_leaves_the_smoothing_distribution_invariant(hostsim):
    C.check_law(hostsim, specialize=False)
