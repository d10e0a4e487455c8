"""The small exported kernels of include/genmi.h on the MI355X: k_mh_accept, k_select, k_random_bits, k_reduce_max,
k_gather / k_gather4, k_lse_rows / k_lse_tiles / k_lse_final, k_sum_tiles / k_sum_final and k_categorical_rows through
the raw C-ABI, with the drivers of tests/abi_kernel_checks.py (tests/test_abi_kernels_cpu.py runs the same ones on the
CPU mirror)."""
import pytest

from tests import abi_kernel_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", K.MH_SIZES)
def test_mh_accept_matches_log_uniform_below_log_alpha(gpu, n):
    K.check_mh_accept(gpu, n)


def test_mh_accept_frequency_follows_p(gpu):
    K.check_mh_accept_frequency(gpu)


@pytest.mark.parametrize("n", K.SELECT_SIZES)
def test_select_mixed_element_sizes(gpu, n):
    K.check_select(gpu, n, K.MIXED_ELEMS)


@pytest.mark.parametrize("n", K.SELECT_SIZES)
def test_select_33_leaves_take_two_launches(gpu, n):
    K.check_select(gpu, n, [4] * 33)


@pytest.mark.parametrize("n,m", K.BITS_SHAPES)
def test_random_bits_match_the_oracle(gpu, n, m):
    K.check_random_bits(gpu, n, m)


@pytest.mark.parametrize("n", K.REDUCE_SIZES)
def test_reduce_max(gpu, n):
    K.check_reduce_max(gpu, n)


def test_reduce_max_of_signed_zeros_is_plus_zero(gpu):
    K.check_reduce_max_signed_zeros(gpu)


@pytest.mark.parametrize("n_out", K.GATHER_N_OUT)
def test_gather_mixed_element_sizes(gpu, n_out):
    K.check_gather_mixed(gpu, n_out)


@pytest.mark.parametrize("n_out", K.GATHER_N_OUT)
def test_gather_agrees_across_alignments(gpu, n_out):
    K.check_gather_alignment(gpu, n_out)


@pytest.mark.parametrize("n_out", [5, 1023])
@pytest.mark.parametrize("leaves", K.GATHER_LEAF_COUNTS)
def test_gather_more_leaves_than_one_launch(gpu, leaves, n_out):
    K.check_gather_many_leaves(gpu, leaves, n_out)


@pytest.mark.parametrize("rows,cols,data", K.lse_cases())
def test_logsumexp_against_float64(gpu, rows, cols, data):
    K.check_logsumexp(gpu, rows, cols, data)


@pytest.mark.parametrize("rows,cols", K.LSE_SPECIAL_SHAPES)
@pytest.mark.parametrize("case", list(K.LSE_SPECIAL))
def test_logsumexp_special_rows(gpu, case, rows, cols):
    K.check_logsumexp_special(gpu, case, rows, cols)


def test_logsumexp_refuses_too_many_long_rows(gpu):
    K.check_refusal(gpu, "gmx_logsumexp", 65_536, 4097)


@pytest.mark.parametrize("rows,cols", K.SUM_SHAPES)
def test_sum_rows_in_the_fixed_tree(gpu, rows, cols):
    K.check_sum_rows(gpu, rows, cols)


def test_sum_rows_refuses_too_many_rows(gpu):
    K.check_refusal(gpu, "gmx_sum_rows", 65_536, 2)


@pytest.mark.parametrize("rows,cols", K.CAT_SHAPES)
def test_categorical_rows_match_the_oracle(gpu, rows, cols):
    K.check_categorical(gpu, rows, cols)


def test_categorical_rows_follow_the_softmax(gpu):
    K.check_categorical_law(gpu)
