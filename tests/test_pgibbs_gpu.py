"""gmx_pg_open (k_pg_open), gmx_pg_propose (k_pg_propose), gmx_pg_accept (k_pg_accept) and smc.ParticleGibbs through the
HIP library on the GPU: the drivers of tests/pgibbs_checks.py with specialised and interpreted programs, the captured
sweep, the device against the CPU mirror bit for bit, and the law."""
import pytest

from tests import pgibbs_checks as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(G.CASES))
def test_open_is_its_definition(gpu, case):
    G.check_open(gpu, case)


@pytest.mark.parametrize("case", list(G.CASES))
def test_propose_is_its_definition(gpu, case):
    G.check_propose(gpu, case)


@pytest.mark.parametrize("shape", [(5, 3, 2), (300, 2, 2), (6, 1, 1), (2, 5, 8)])
def test_accept_is_its_definition(gpu, shape):
    G.check_accept(gpu, *shape)


def test_device_refuses_bad_arguments_before_any_launch(gpu):
    G.refusal_messages(gpu.c)


@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("chain", G.CHAINS, ids=G.chain_id)
def test_chain_is_the_composition_of_public_parts(gpu, chain, specialize):
    G.check_chain_is_the_composition(gpu, chain, specialize=specialize)


@pytest.mark.parametrize("chain", G.CHAINS, ids=G.chain_id)
def test_captured_sweep_is_the_uncaptured_run(gpu, chain):
    G.check_captured(gpu, chain)


@pytest.mark.parametrize("chain", G.CHAINS, ids=G.chain_id)
def test_device_is_the_mirror_bit_for_bit(gpu, chain):
    G.check_device_is_the_mirror(gpu, chain)


def test_chains_sample_the_exact_posterior(gpu):
    G.check_law(gpu)
