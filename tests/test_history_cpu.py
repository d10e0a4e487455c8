"""BootstrapSweep(history=True), gmx_history_record and gmx_lineage on the C-ABI's CPU mirror (tests/hostsim), plus the
null-argument rejection of the two entry points on the HIP library itself (no GPU involved).  The drivers are in
tests/history_checks.py; tests/test_history_gpu.py runs the same ones through the HIP kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import history_checks as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (fuse_resample, noise_ahead, specialize, resample): the forms the mirror has (no graph capture on the host)
SWEEP_FORMS = [
    (True, True, True, "systematic"),
    (True, False, True, "systematic"),
    (False, False, False, "systematic"),
    (False, False, False, "stratified"),
    (False, True, True, "multinomial_tiled"),
    (False, False, False, "multinomial_sorted"),
]


@pytest.mark.parametrize("fuse,noise_ahead,specialize,resample", SWEEP_FORMS)
def test_sweep_record_matches_oracle(hostsim, fuse, noise_ahead, specialize, resample):
    sw, h = H.check_lgssm_record(fuse, noise_ahead, False, specialize, resample)
    if resample == "systematic":
        H.check_end_to_end(sw, h)
        H.check_filter_mean(h)


@pytest.mark.parametrize("which", ["vector", "tuple"])
@pytest.mark.parametrize("fuse", [False, True])
def test_vector_and_tuple_state_record(hostsim, which, fuse):
    sw = H.check_state_record(which, specialize=fuse, fuse_resample=fuse)
    assert sw.fuse == fuse
    H.check_filter_mean(sw.history())


def test_history_needs_the_argument_and_refuses_rejuvenate(hostsim):
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    init, step = workloads.make_lgssm(G)
    with pytest.raises(NotImplementedError, match="rejuvenate"):
        BootstrapSweep(init, step, 64, 3, rejuvenate=object(), history=True)
    sw = BootstrapSweep(init, step, 64, 3, specialize=False).prepare(G.key(1), torch.from_numpy(workloads.lgssm_data(3)))
    sw.launch()
    with pytest.raises(RuntimeError, match="history=True"):
        sw.history()


def test_stale_tagged_word_condemns_the_history(hostsim):
    """a recorded word with another step's tag sets the status word: history() refuses until reset_status()"""
    sw = H.run_lgssm(True, True, False, False, True, "systematic")
    sw.history()
    sw.anc.fill_(3 | (9 << 24))
    sw._record(1, tagged=True)           # step 1's words carry tag 2
    with pytest.raises(RuntimeError, match="stale"):
        sw.history()
    sw.reset_status()
    sw.launch()
    sw.history()


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("mode", ["plain", "tagged", "stale"])
def test_history_record_alone(hostsim, D, n, mode):
    H.check_record_alone(hostsim, D, n, mode)


@pytest.mark.parametrize("T,D,n,m", [(1, 1, 5, 1), (7, 1, 5, 1027), (7, 3, 1027, 1027), (5, 2, 4099, 64)])
def test_lineage_matches_numpy_walk(hostsim, T, D, n, m):
    H.check_lineage(hostsim, T, D, n, m)


def test_lineage_counts_and_clamps_out_of_range_starts(hostsim):
    H.check_lineage_out_of_range(hostsim)


def test_lineage_out_of_range_reads_nothing_outside_under_asan():
    """the same validation under AddressSanitizer (the mirror's sanitized build, in a child process as
    tests/test_sanitizers.py does): a start of n or -1 must not read outside the slabs"""
    import tests.hostsim as hs
    hs_so = hs.build_sanitized()
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", PYTHONMALLOC="malloc", OMP_NUM_THREADS="2",
               GENMI_HOSTSIM_SO=hs_so)
    code = ("import sys; sys.path.insert(0, %r); import tests.hostsim as hs; from tests import history_checks as H; "
            "be = hs.install(); H.check_lineage_out_of_range(be); H.check_lineage(be, 7, 3, 1027, 1027); "
            "H.check_record_alone(be, 3, 1027, 'stale'); print('history under asan ok')") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    bad = [ln for ln in r.stderr.splitlines() if "AddressSanitizer" in ln or "runtime error:" in ln]
    assert r.returncode == 0 and not bad, (r.returncode, bad[:5], r.stderr[-3000:])
    assert "history under asan ok" in r.stdout


def test_filter_mean_tracks_the_kalman_filter(hostsim):
    """n = 4096, T = 20 on the linear-Gaussian model: every step's filter mean within 5 standard errors of the exact
    filtered mean (a float64 Kalman filter, the recursion of workloads.kalman_log_ml).  The standard error is the
    self-normalised importance-sampling estimator's, from the RECORDED weights: se_t^2 = sum_i w_i^2 (x_i - mean_t)^2
    with w = softmax(lw_t) (the delta-method variance of sum_i w_i x_i; Owen, Monte Carlo theory, methods and
    examples, eq. 9.8)."""
    import math
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.smc import BootstrapSweep
    n, T = 4096, 20
    ys = workloads.lgssm_data(T)
    init, step = workloads.make_lgssm(G)
    sw = BootstrapSweep(init, step, n, T, specialize=False, history=True).prepare(G.key(20240), torch.from_numpy(ys))
    sw.launch()
    h = sw.history()
    got = h.filter_mean().numpy()
    p = workloads.LGSSM
    a, q, r = p["a"], p["sx"] ** 2, p["sy"] ** 2
    m, P, exact = 0.0, p["s0"] ** 2, []
    for t, y in enumerate(np.asarray(ys, dtype=np.float64)):
        if t > 0:
            m, P = a * m, a * a * P + q
        K = P / (P + r)
        m, P = m + K * (y - m), (1 - K) * P
        exact.append(m)
    exact = np.array(exact)
    w = torch.softmax(h.log_weights.double(), dim=1).numpy()
    x = h.x.double().numpy()
    se = np.sqrt(np.sum(w ** 2 * (x - got[:, None]) ** 2, axis=1))
    z = np.abs(got - exact) / se
    print("filter mean, |error| in standard errors per step:", np.round(z, 2))
    assert math.isfinite(float(z.max())) and np.all(z <= 5.0), z


def test_history_entry_points_reject_null_arguments_before_any_launch():
    """the pattern of tests/test_abi.py: null pointers / non-positive sizes return non-zero and name the entry point —
    on the HIP library, on a box without a GPU"""
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(so)
    lib.gmx_last_error.restype = ctypes.c_char_p
    calls, _keep = H.history_refusal_calls()
    for name, args, why in calls:
        rc = getattr(lib, name)(*args)
        assert rc != 0, (name, args)
        assert name.encode() in lib.gmx_last_error() and why in lib.gmx_last_error(), (name, why, lib.gmx_last_error())
