"""gmx_pmmh_propose (k_pmmh_propose), gmx_pmmh_accept (k_pmmh_accept) and smc.ParticleMH through the HIP library on the
GPU: the drivers of tests/pmmh_checks.py with specialised and interpreted programs, the captured form, the device against
the CPU mirror bit for bit, and the law."""
import pytest

from tests import pmmh_checks as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(M.CASES))
def test_propose_is_its_definition(gpu, case):
    M.check_propose(gpu, case)


@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("shape", [(5, 3, 2, 8), (300, 2, 2, 4), (6, 5, 1, 16), (3, 1, 2, 100)])
def test_accept_is_its_definition(gpu, shape, with_flags):
    R, T, P, n = shape
    M.check_accept(gpu, R, T, P, n, with_flags)


def test_log64_against_numpy(gpu):
    M.check_log64(gpu)


def test_device_refuses_bad_arguments_before_any_launch(gpu):
    M.refusal_messages(gpu.c)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("case", list(M.CASES))
def test_chain_is_the_composition_of_public_parts(gpu, case, specialize):
    M.check_chain_is_the_composition(gpu, case, specialize=specialize)


@pytest.mark.parametrize("case", list(M.CASES))
def test_captured_run_is_the_uncaptured_run(gpu, case):
    M.check_captured(gpu, case, specialize=True)


@pytest.mark.parametrize("case", list(M.CASES))
def test_device_is_the_mirror_bit_for_bit(gpu, case):
    M.check_device_is_the_mirror(gpu, case)


def test_chains_sample_the_exact_posterior(gpu):
    M.check_law(gpu)
