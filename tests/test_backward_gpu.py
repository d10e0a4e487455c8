"""gmx_pick_rows (k_pick_stats, k_pick_row) and SweepHistory.backward_sample on the MI355X: the drivers of
tests/backward_checks.py through the HIP library, plus what only the device has — a captured, twice-replayed sweep and
element offsets past 2^31."""
import numpy as np
import pytest
import torch

from tests import backward_checks as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", B.PICK_CASES)
def test_pick_rows_matches_the_oracles_per_row_path(gpu, name):
    B.check_pick_case(gpu, name)


@pytest.mark.parametrize("name", ["normal5", "normal1025", "mixed"])
def test_pick_rows_with_padded_rows(gpu, name):
    """ld = n + 3, poison in the padding: rows start at odd 4-byte boundaries and the padding is never read"""
    B.check_pick_case(gpu, name, pad=3)


def test_pick_rows_counts_a_row_without_mass(gpu):
    B.check_pick_no_mass(gpu)


def test_pick_rows_offsets_past_two_to_the_31(gpu):
    """rows = 3, n = 1025, ld = 2^30 + 8: row 2 starts at element 2^31 + 16.  The matrix is allocated, never filled; only
    the row heads are written.  32-bit offset arithmetic reads other words."""
    rows, n, ld = 3, 1025, 2 ** 30 + 8
    dev = gpu.device
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 16 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GB free on this device: the {rows * ld * 4 / 2 ** 30:.1f} GB matrix needs 16")
    heads = B.pick_case("normal1025")[:rows]
    keys = B.pick_keys(rows)
    logits = torch.empty((rows, ld), dtype=torch.float32, device=dev)
    logits[:, :n] = torch.from_numpy(np.array(heads)).to(dev)
    logits[:, n:n + 64] = float(B.POISON)
    k_d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(rows, 2)).to(dev)
    out = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = torch.empty(((gpu.c.gmx_pick_rows_workspace(rows, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = gpu.c.gmx_pick_rows(gpu.ptr(k_d), gpu.ptr(logits), rows, n, ld, gpu.ptr(out), gpu.ptr(status), gpu.ptr(ws),
                             gpu.stream())
    assert rc == 0, gpu.c.gmx_last_error()
    assert int(status.item()) == 0
    assert out.cpu().tolist() == [B.oracle_pick(heads[r], keys[r]) for r in range(rows)]


@pytest.mark.parametrize("capture", [False, True])
def test_backward_sample_matches_the_oracle_loop_lgssm(gpu, capture):
    """a plain sweep, and a captured one replayed twice"""
    B.check_backward_lgssm(capture)


@pytest.mark.parametrize("form", ["interpreted", "default"])
def test_backward_sample_matches_the_oracle_loop_tracker(gpu, form):
    if form == "interpreted":
        B.check_backward_tracker(specialize=False, fuse_resample=False)
    else:
        B.check_backward_tracker()


def test_backward_sample_follows_the_ffbs_law(gpu):
    B.check_law()


def test_backward_sample_refusals_name_what_is_missing(gpu):
    B.check_refusals()


def test_backward_sample_without_mass_is_an_error(gpu):
    B.check_no_mass_is_an_error(gpu)
