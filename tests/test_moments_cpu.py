"""gmx_rows_moments and smc.BootstrapBank(moments=True) on the CPU mirror, and the HIP library's refusals (tests/moments_checks.py)."""
import pytest

from tests import moments_checks as M


@pytest.mark.parametrize("n", M.SIZES)
def test_rows_moments_against_float64(hostsim, n):
    M.check_size(hostsim, n)


@pytest.mark.parametrize("which", ["mirror", "hip"])
def test_library_refuses_bad_arguments_and_sizes_its_workspace(which):
    M.check_refusals_of(M.library(which).c)


def test_row_moments_refuses_a_wrong_out_as_its_siblings_do(hostsim):
    """out= of the wrong dtype or too narrow is refused in Python (row_covariance's and row_quantiles' check), a fitting one is used"""
    import torch
    from genjax_amd.inference import smc
    lw, x = torch.zeros((2, 5)), torch.arange(10.0).reshape(2, 5)
    for bad in (torch.empty((2, 3), dtype=torch.float32), torch.empty((2, 2), dtype=torch.float64), torch.empty((3, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"row_moments: out is a float64 \[R, >= 1 \+ 2 D\] = \[2, >= 3\] matrix"):
            smc.row_moments(lw, x, out=bad)
    out = torch.empty((2, 4), dtype=torch.float64)
    got = smc.row_moments(lw, x, out=out)
    assert got.mean.data_ptr() == out[:, 1:].data_ptr() and got.mean.tolist() == [2.0, 7.0] and got.ess.tolist() == [5.0, 5.0]


@pytest.mark.parametrize("kw", M.BANKS)
def test_bank_is_unchanged_and_its_moments_are_the_reference_and_the_history(hostsim, kw):
    M.check_bank(hostsim, specialize=False, capture=False, **kw)
