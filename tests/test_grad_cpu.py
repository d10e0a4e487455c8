"""genjax_amd/autodiff.py on the C-ABI's CPU mirror (tests/hostsim): every derivative rule against torch.float64 autograd, the
edges pinned, the classification of every op, `value_and_grad` as an API and HMC through the non-normal densities.  The
drivers and the reasoning behind every tolerance are in tests/grad_checks.py; tests/test_grad_gpu.py runs the same ones
through the HIP kernels, interpreted and specialised."""
import pytest

from tests import grad_checks as D


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("name", D.RULE_NAMES)
def test_rule_against_float64_autograd(hostsim, name, n):
    D.check_rule(hostsim, name, n)


@pytest.mark.parametrize("name", D.RULE_NAMES)
def test_replay_errors_are_the_recorded_ones(name):
    """the last column of RULES is what the hand-written float32 replay measures against float64 (within a factor of two:
    the column is rounded to two digits and libm may move a last bit)"""
    got, col = D.replay_error(name), D.RULE[name].measured
    print(name, "replay error", got, "recorded", col)
    assert 0.5 * col <= got <= 2.0 * col, (name, got, col)


@pytest.mark.parametrize("name", D.EDGE_NAMES)
def test_edge_is_pinned(hostsim, name):
    D.check_edge(hostsim, name)


def test_hmc_through_a_saturated_flip_stays_finite(hostsim):
    D.check_hmc_through_a_saturated_flip(hostsim)


def test_every_op_is_differentiable_or_zero_gradient_or_refused_by_name(hostsim):
    D.check_classification()


def test_lgamma_and_beta_are_refused_by_name(hostsim):
    D.check_not_differentiable_by_name(hostsim)


def test_fnkey_tells_defaults_apart():
    D.check_fnkey()


def test_value_and_grad_cache_key_sees_defaults(hostsim):
    D.check_cache_key_sees_defaults(hostsim)


def test_rejuvenate_argument_mappings_that_differ_in_a_default(hostsim):
    D.check_rejuvenate_argument_mappings_that_differ_in_a_default(hostsim)


def test_constant_and_zero_gradients_are_tensors(hostsim):
    D.check_constant_gradients_are_tensors(hostsim)


@pytest.mark.parametrize("n_obs,density", D.HMC_CASES)
def test_hmc_step_weight_reconstructed_in_float64(hostsim, n_obs, density):
    D.check_hmc_step(hostsim, n_obs, density)
