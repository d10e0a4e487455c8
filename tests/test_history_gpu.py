"""BootstrapSweep(history=True), gmx_history_record (k_history_record) and gmx_lineage (k_lineage) on the MI355X: the
drivers of tests/history_checks.py through the HIP library, plus what only the device has — captured graphs replayed
twice, the looped one-launch form past 2^20 particles and element offsets past 2^31."""
import numpy as np
import pytest
import torch

from tests import history_checks as H

pytestmark = pytest.mark.gpu

# (fuse_resample, noise_ahead, capture, specialize, resample); the first is the default form of the headline sweep
SWEEP_FORMS = [
    (True, True, True, True, "systematic"),
    (True, False, False, True, "systematic"),
    (False, False, True, False, "systematic"),
    (False, True, True, True, "stratified"),
    (False, False, False, False, "multinomial_tiled"),
    (False, True, False, True, "multinomial_sorted"),
]


@pytest.mark.parametrize("fuse,noise_ahead,capture,specialize,resample", SWEEP_FORMS)
def test_sweep_record_matches_oracle(gpu, fuse, noise_ahead, capture, specialize, resample):
    sw, h = H.check_lgssm_record(fuse, noise_ahead, capture, specialize, resample)
    if resample == "systematic":
        H.check_end_to_end(sw, h)
        H.check_filter_mean(h)


@pytest.mark.parametrize("which", ["vector", "tuple"])
@pytest.mark.parametrize("form", ["interpreted", "default"])
def test_vector_and_tuple_state_record(gpu, which, form):
    """interpreted, two launches per step, eager; and the sweep's default form (specialised, one launch per step where
    the programs allow it, noise ahead), captured and replayed twice"""
    if form == "interpreted":
        sw = H.check_state_record(which, specialize=False, fuse_resample=False)
        assert not sw.fuse
    else:
        sw = H.check_state_record(which, capture=True)
    H.check_filter_mean(sw.history())


def test_looped_one_launch_form_records_what_the_two_launch_form_does(gpu):
    """n = 2^20 + 1027: the one-launch form LOOPS over tiles there; its history equals the two-launch form's at the same
    key (the form pinned to the oracle above: an oracle sweep of this size does not fit a few seconds)"""
    n, T = 2 ** 20 + 1027, 3
    one = H.run_lgssm(True, True, True, False, True, "systematic", n=n, T=T)
    two = H.run_lgssm(True, False, True, False, True, "systematic", n=n, T=T)
    a, b = one.history(), two.history()
    for t in range(T):
        assert torch.equal(a.x[t].view(torch.int32), b.x[t].view(torch.int32)), t
        assert torch.equal(a.log_weights[t].view(torch.int32), b.log_weights[t].view(torch.int32)), t
        assert torch.equal(a.ancestors[t], b.ancestors[t]), t
    assert one.log_ml() == two.log_ml()
    assert torch.equal(a.lineage(), b.lineage())


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("mode", ["plain", "tagged", "stale"])
def test_history_record_alone(gpu, D, n, mode):
    H.check_record_alone(gpu, D, n, mode)


@pytest.mark.parametrize("T,D,n,m", [(1, 1, 5, 1), (7, 1, 5, 1027), (7, 3, 1027, 1027), (5, 2, 4099, 64), (4, 5, 300, 777)])
def test_lineage_matches_numpy_walk(gpu, T, D, n, m):
    """(the last shape: D = 5 takes the kernel's any-D form, the others its unrolled ones)"""
    H.check_lineage(gpu, T, D, n, m)


def test_lineage_counts_and_clamps_out_of_range_starts(gpu):
    H.check_lineage_out_of_range(gpu)


def test_lineage_offsets_past_two_to_the_31(gpu):
    """T = 5, D = 1, n = 2^29 + 3: row 4 of either slab starts at element 4 n > 2^31.  The slabs are allocated, never
    filled; only the entries on four hand-made paths are written.  32-bit offset arithmetic reads other words."""
    T, D, n, m = 5, 1, 2 ** 29 + 3, 4
    dev = gpu.device
    try:
        ancs = torch.empty((T, n), dtype=torch.int32, device=dev)
        xs = torch.empty((T, D, n), dtype=torch.float32, device=dev)
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:       # noqa: PERF203
        pytest.skip(f"two {T * n * 4 / 1e9:.1f} GB slabs do not fit this device: {e}")
    # path j visits hops[j][t] at level t (distinct entries, so no path overwrites another's)
    hops = np.array([[7, n - 2, 3, n - 5, n - 1],
                     [n - 1, 11, n - 3, 2 ** 28 + 1, 0],
                     [2 ** 29 - 1, 2 ** 29 - 2, 2 ** 29 - 3, 5, 2 ** 27],
                     [1, 2, 4, 8, 16]], dtype=np.int64)
    assert all(len(set(hops[:, t].tolist())) == m for t in range(T))
    vals = (np.arange(m * T, dtype=np.float32).reshape(m, T) + 0.5)
    for j in range(m):
        for t in range(T):
            xs[t, 0, int(hops[j, t])] = float(vals[j, t])
            if t:
                ancs[t - 1, int(hops[j, t])] = int(hops[j, t - 1])
    start = torch.tensor(hops[:, T - 1], dtype=torch.int32, device=dev)
    paths = torch.zeros((T, m), dtype=torch.int32, device=dev)
    traj = torch.zeros((T, D, m), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    rc = gpu.c.gmx_lineage(gpu.ptr(ancs), gpu.ptr(xs), T, D, n, gpu.ptr(start), m, gpu.ptr(paths), gpu.ptr(traj),
                           gpu.ptr(status), gpu.stream())
    assert rc == 0, gpu.c.gmx_last_error()
    assert int(status.item()) == 0
    assert np.array_equal(paths.cpu().numpy(), hops.T.astype(np.int32))
    assert np.array_equal(traj.cpu().numpy()[:, 0, :], vals.T)
