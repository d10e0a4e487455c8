"""The small exported kernels of include/genmi.h on the C-ABI's CPU mirror (tests/hostsim): the drivers of
tests/abi_kernel_checks.py and every reference they use, verified on a machine without a GPU.
tests/test_abi_kernels_gpu.py runs the same drivers through the HIP kernels."""
import pytest

from tests import abi_kernel_checks as K


@pytest.mark.parametrize("n", K.MH_SIZES)
def test_mh_accept_matches_log_uniform_below_log_alpha(hostsim, n):
    K.check_mh_accept(hostsim, n)


def test_mh_accept_frequency_follows_p(hostsim):
    K.check_mh_accept_frequency(hostsim)


@pytest.mark.parametrize("n", K.SELECT_SIZES)
def test_select_mixed_element_sizes(hostsim, n):
    K.check_select(hostsim, n, K.MIXED_ELEMS)


@pytest.mark.parametrize("n", K.SELECT_SIZES)
def test_select_33_leaves_take_two_launches(hostsim, n):
    K.check_select(hostsim, n, [4] * 33)


@pytest.mark.parametrize("n,m", K.BITS_SHAPES)
def test_random_bits_match_the_oracle(hostsim, n, m):
    K.check_random_bits(hostsim, n, m)


@pytest.mark.parametrize("n", K.REDUCE_SIZES)
def test_reduce_max(hostsim, n):
    K.check_reduce_max(hostsim, n)


def test_reduce_max_of_signed_zeros_is_plus_zero(hostsim):
    K.check_reduce_max_signed_zeros(hostsim)


@pytest.mark.parametrize("n_out", K.GATHER_N_OUT)
def test_gather_mixed_element_sizes(hostsim, n_out):
    K.check_gather_mixed(hostsim, n_out)


@pytest.mark.parametrize("n_out", K.GATHER_N_OUT)
def test_gather_agrees_across_alignments(hostsim, n_out):
    K.check_gather_alignment(hostsim, n_out)


@pytest.mark.parametrize("n_out", [5, 1023])
@pytest.mark.parametrize("leaves", K.GATHER_LEAF_COUNTS)
def test_gather_more_leaves_than_one_launch(hostsim, leaves, n_out):
    K.check_gather_many_leaves(hostsim, leaves, n_out)


@pytest.mark.parametrize("rows,cols,data", K.lse_cases())
def test_logsumexp_against_float64(hostsim, rows, cols, data):
    K.check_logsumexp(hostsim, rows, cols, data)


@pytest.mark.parametrize("rows,cols", K.LSE_SPECIAL_SHAPES)
@pytest.mark.parametrize("case", list(K.LSE_SPECIAL))
def test_logsumexp_special_rows(hostsim, case, rows, cols):
    K.check_logsumexp_special(hostsim, case, rows, cols)


def test_logsumexp_refuses_too_many_long_rows(hostsim):
    K.check_refusal(hostsim, "gmx_logsumexp", 65_536, 4097)


@pytest.mark.parametrize("rows,cols", K.SUM_SHAPES)
def test_sum_rows_in_the_fixed_tree(hostsim, rows, cols):
    K.check_sum_rows(hostsim, rows, cols)


def test_sum_rows_refuses_too_many_rows(hostsim):
    K.check_refusal(hostsim, "gmx_sum_rows", 65_536, 2)


@pytest.mark.parametrize("rows,cols", K.CAT_SHAPES)
def test_categorical_rows_match_the_oracle(hostsim, rows, cols):
    K.check_categorical(hostsim, rows, cols)


def test_categorical_rows_follow_the_softmax(hostsim):
    K.check_categorical_law(hostsim)
