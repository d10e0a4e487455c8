"""gmx_pg_open, gmx_pg_propose, gmx_pg_accept and smc.ParticleGibbs on the C-ABI's CPU mirror (tests/hostsim), plus the
argument refusals of the three entry points on the HIP library itself (no GPU involved) and the float64 numpy particle
Gibbs the law test's design was checked with.  The drivers are in tests/pgibbs_checks.py; tests/test_pgibbs_gpu.py runs
the same ones through the HIP kernels."""
import ctypes
import os

import pytest

from tests import pgibbs_checks as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_library():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    return ctypes.CDLL(so)


@pytest.mark.parametrize("case", list(G.CASES))
def test_open_is_its_definition(hostsim, case):
    G.check_open(hostsim, case)


@pytest.mark.parametrize("case", list(G.CASES))
def test_propose_is_its_definition(hostsim, case):
    G.check_propose(hostsim, case)


@pytest.mark.parametrize("shape", [(5, 3, 2), (300, 2, 2), (6, 1, 1), (2, 5, 8)])
def test_accept_is_its_definition(hostsim, shape):
    G.check_accept(hostsim, *shape)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """on the HIP library, on a box without a GPU"""
    G.refusal_messages(_hip_library())


def test_mirror_refuses_the_same_arguments_with_the_same_messages(hostsim):
    assert G.refusal_messages(hostsim.c) == G.refusal_messages(_hip_library())


@pytest.mark.parametrize("chain", G.CHAINS, ids=G.chain_id)
def test_chain_is_the_composition_of_public_parts(hostsim, chain):
    G.check_chain_is_the_composition(hostsim, chain, specialize=False)


def test_vector_and_tuple_states(hostsim):
    G.check_state_shapes(hostsim)


def test_api_refusals_name_what_they_refuse(hostsim):
    G.check_api_refusals(hostsim)


def test_numpy_particle_gibbs_samples_the_exact_posterior():
    G.check_numpy_reference()
