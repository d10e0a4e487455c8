"""The tail of the normal draw and gmx_logf on the C-ABI's CPU mirror (tests/hostsim compiles the product's own headers):
the select-free exponent / mantissa split (csrc/gmx_math.h gmx_log_split) and the clamp as one max (csrc/gmx_rng.h) give
the oracle's numbers — every one of the 2^23 inputs a draw can have, and the log over the set of
tests/normal_tail_checks.py.  (The device-only division of gmx_neg_log1m_sq is held by tests/test_normal_tail_gpu.py.)"""
from tests import normal_tail_checks as C


def test_every_normal_draw_matches_the_oracle(hostsim):
    C.hold_normal(hostsim, lambda t: t)


def test_vm_log_matches_the_oracle_on_the_fixed_set(hostsim):
    C.hold_log(lambda t: t)
