"""gmx_pmmh_propose, gmx_pmmh_accept and smc.ParticleMH on the C-ABI's CPU mirror (tests/hostsim), plus the argument
refusals of the two entry points on the HIP library itself (no GPU involved).  The drivers are in tests/pmmh_checks.py;
tests/test_pmmh_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import pmmh_checks as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    return ctypes.CDLL(so)


@pytest.mark.parametrize("case", list(M.CASES))
def test_propose_is_its_definition(hostsim, case):
    M.check_propose(hostsim, case)


@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("shape", [(5, 3, 2, 8), (300, 2, 2, 4), (6, 5, 1, 16), (3, 1, 2, 100)])
def test_accept_is_its_definition(hostsim, shape, with_flags):
    R, T, P, n = shape
    M.check_accept(hostsim, R, T, P, n, with_flags)


def test_log64_against_numpy(hostsim):
    M.check_log64(hostsim)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    M.refusal_messages(_hip_library())


def test_mirror_refuses_the_same_arguments_with_the_same_messages(hostsim):
    assert M.refusal_messages(hostsim.c) == M.refusal_messages(_hip_library())


@pytest.mark.parametrize("case", list(M.CASES))
def test_chain_is_the_composition_of_public_parts(hostsim, case):
    M.check_chain_is_the_composition(hostsim, case, specialize=False)


def test_api_refusals_name_what_they_refuse(hostsim):
    M.check_api_refusals(hostsim)

