"""gmx_resample_rows, smc.resample on batched collections and smc.BootstrapBank on the C-ABI's CPU mirror (tests/hostsim),
plus the argument refusals of the entry point on the HIP library itself (no GPU involved).  The drivers are in
tests/bank_checks.py; tests/test_bank_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import bank_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = list(K.ROW_KINDS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", K.ROW_SIZES + K.PACKING_SIZES)
def test_resample_rows_matches_the_oracles_per_row_path(hostsim, kind, n):
    K.check_rows_case(hostsim, kind, "normal%d" % n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", K.ROW_SHAPES)
def test_resample_rows_on_gaps_holes_and_single_columns(hostsim, kind, name):
    K.check_rows_case(hostsim, kind, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", K.ROW_COUNTS)
def test_resample_rows_row_counts_around_the_packing(hostsim, kind, rows):
    K.check_rows_case(hostsim, kind, "count%d" % rows)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["normal5", "normal255", "normal1025", "mixed"])
def test_resample_rows_with_padded_rows(hostsim, kind, name):
    """ld = n + 3, poison in the padding: rows start at odd 4-byte boundaries and the padding is never read"""
    K.check_rows_case(hostsim, kind, name, pad=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["count7", "normal1023", "normal2051"])
def test_resample_rows_index_stride_gives_flat_indices(hostsim, kind, name):
    K.check_rows_case(hostsim, kind, name, stride=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["count7", "normal2051"])
def test_resample_rows_counts_a_row_without_mass(hostsim, kind, name):
    K.check_rows_no_mass(hostsim, kind, name)


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(so)
    lib.gmx_last_error.restype = ctypes.c_char_p
    lib.gmx_resample_rows_workspace.restype = ctypes.c_size_t
    lib.gmx_resample_rows_workspace.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
    return lib


def test_resample_rows_rejects_bad_arguments_before_any_launch():
    """the pattern of tests/test_backward_cpu.py: on the HIP library, on a box without a GPU"""
    lib = _hip_library()
    calls, _keep = K.rows_refusal_calls()
    for args, names in calls:
        rc = lib.gmx_resample_rows(*args)
        assert rc != 0, args
        msg = lib.gmx_last_error()
        assert b"gmx_resample_rows" in msg and names in msg, (msg, names)
    # nothing up to one tile; 12 bytes per (row, tile) past it; the iid multinomial adds its [rows, n] u64 CDF
    assert lib.gmx_resample_rows_workspace(0, 4096, 1024) == 16
    assert lib.gmx_resample_rows_workspace(0, 3, 1025) == 80
    assert lib.gmx_resample_rows_workspace(1, 16, 65536) == 16 * 64 * 12
    assert lib.gmx_resample_rows_workspace(2, 3, 1025) == (6 * 12 + 3 * 1025 * 8 + 15) // 16 * 16


def test_resample_rows_mirror_refuses_the_same_arguments(hostsim):
    calls, _keep = K.rows_refusal_calls()
    for args, _ in calls:
        assert hostsim.c.gmx_resample_rows(*args) != 0, args


@pytest.mark.parametrize("kind", KINDS)
def test_resample_batched_equals_the_one_dimensional_calls(hostsim, kind):
    K.check_resample_batched(hostsim, kind)


def test_resample_batched_refusals_name_the_shapes_and_the_kinds(hostsim):
    K.check_resample_batched_refusals(hostsim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["lgssm", "tracker"])
@pytest.mark.parametrize("n", [K.BANK_N, K.BANK_SMALL_N])
def test_bank_rows_equal_single_sweeps_bit_for_bit(hostsim, model, kind, n):
    K.check_bank_against_sweeps(hostsim, model, kind, n, specialize=False)


def test_bank_params_are_per_filter_and_position_independent(hostsim):
    K.check_params(hostsim, specialize=False)


def test_bank_evidence_estimate_is_unbiased(hostsim):
    K.check_law(hostsim, specialize=False)


def test_bank_out_of_scope_options_raise_by_name(hostsim):
    K.check_bank_refusals(hostsim)
