"""gmx_pick_rows and SweepHistory.backward_sample on the C-ABI's CPU mirror (tests/hostsim), plus the argument refusals
of the entry point on the HIP library itself (no GPU involved).  The drivers are in tests/backward_checks.py;
tests/test_backward_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import backward_checks as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", B.PICK_CASES)
def test_pick_rows_matches_the_oracles_per_row_path(hostsim, name):
    B.check_pick_case(hostsim, name)


@pytest.mark.parametrize("name", ["normal5", "normal1025", "mixed"])
def test_pick_rows_with_padded_rows(hostsim, name):
    """ld = n + 3, poison in the padding: rows start at odd 4-byte boundaries and the padding is never read"""
    B.check_pick_case(hostsim, name, pad=3)


def test_pick_rows_counts_a_row_without_mass(hostsim):
    B.check_pick_no_mass(hostsim)


def test_backward_sample_matches_the_oracle_loop_lgssm(hostsim):
    B.check_backward_lgssm(False)


def test_backward_sample_matches_the_oracle_loop_tracker(hostsim):
    B.check_backward_tracker(specialize=False, fuse_resample=False)


def test_backward_sample_follows_the_ffbs_law(hostsim):
    B.check_law()


def test_backward_sample_refusals_name_what_is_missing(hostsim):
    B.check_refusals()


def test_backward_sample_without_mass_is_an_error(hostsim):
    B.check_no_mass_is_an_error(hostsim)


def test_pick_rows_rejects_null_arguments_and_sizes_before_any_launch():
    """the pattern of tests/test_history_cpu.py: on the HIP library, on a box without a GPU"""
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(so)
    lib.gmx_last_error.restype = ctypes.c_char_p
    lib.gmx_pick_rows_workspace.restype = ctypes.c_size_t
    lib.gmx_pick_rows_workspace.argtypes = [ctypes.c_int64, ctypes.c_int64]
    N, i64 = ctypes.c_void_p(0), ctypes.c_int64
    buf = (ctypes.c_int64 * 8)()
    Bp = ctypes.cast(buf, ctypes.c_void_p)
    calls = [
        (N, Bp, i64(2), i64(10), i64(10), Bp, Bp, Bp, N),            # no keys
        (Bp, N, i64(2), i64(10), i64(10), Bp, Bp, Bp, N),            # no logits
        (Bp, Bp, i64(2), i64(10), i64(10), N, Bp, Bp, N),            # no output
        (Bp, Bp, i64(2), i64(10), i64(10), Bp, N, Bp, N),            # no status word
        (Bp, Bp, i64(2), i64(10), i64(10), Bp, Bp, N, N),            # no workspace
        (Bp, Bp, i64(0), i64(10), i64(10), Bp, Bp, Bp, N),           # rows = 0
        (Bp, Bp, i64(2), i64(0), i64(10), Bp, Bp, Bp, N),            # n = 0
        (Bp, Bp, i64(2), i64(2 ** 31), i64(2 ** 31), Bp, Bp, Bp, N),  # n = 2^31
        (Bp, Bp, i64(2), i64(10), i64(9), Bp, Bp, Bp, N),            # ld < n
    ]
    for args in calls:
        rc = lib.gmx_pick_rows(*args)
        assert rc != 0, args
        assert b"gmx_pick_rows" in lib.gmx_last_error(), lib.gmx_last_error()
    # 12 bytes per (row, tile), rounded up to 16
    assert lib.gmx_pick_rows_workspace(3, 1025) == 80 and lib.gmx_pick_rows_workspace(64, 10 ** 6) == 64 * 977 * 12
