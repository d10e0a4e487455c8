"""genjax_amd/autodiff.py through the HIP library on the GPU: the drivers of tests/grad_checks.py, every gradient program run on
the interpreter (the default at these sizes) AND as a hiprtc-specialised kernel, the two equal bit for bit and both held to
torch.float64 autograd; the program the 31-register interpreter cannot hold runs specialised only — the path
Compiled._cross_check skips — and is held to float64 by the same bound."""
import pytest

from tests import grad_checks as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", D.RULE_NAMES)
def test_rule_against_float64_autograd_interpreted_and_specialised(gpu, name):
    D.check_rule_specialised(gpu, name)


@pytest.mark.parametrize("name", D.EDGE_NAMES)
def test_edge_is_pinned_interpreted_and_specialised(gpu, name):
    D.check_edge_specialised(gpu, name)


def test_hmc_through_a_saturated_flip_stays_finite(gpu):
    D.check_hmc_through_a_saturated_flip(gpu)
    with D.every_program_specialised(gpu):
        D.check_hmc_through_a_saturated_flip(gpu)


def test_lgamma_and_beta_are_refused_by_name(gpu):
    D.check_not_differentiable_by_name(gpu)


def test_value_and_grad_cache_key_sees_defaults(gpu):
    D.check_cache_key_sees_defaults(gpu)


def test_rejuvenate_argument_mappings_that_differ_in_a_default(gpu):
    D.check_rejuvenate_argument_mappings_that_differ_in_a_default(gpu)


def test_constant_and_zero_gradients_are_tensors(gpu):
    D.check_constant_gradients_are_tensors(gpu)


@pytest.mark.parametrize("n_obs,density", D.HMC_CASES)
def test_hmc_step_weight_reconstructed_in_float64_interpreted_and_specialised(gpu, n_obs, density):
    D.check_hmc_step_specialised(gpu, n_obs, density)
