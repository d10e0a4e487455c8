"""gmx_resample_rows (k_rows_small, k_pick_stats + k_rows_tile, k_rows_mn), smc.resample on batched collections and
smc.BootstrapBank on the MI355X: the drivers of tests/bank_checks.py through the HIP library, plus what only the device
has — element offsets past 2^31 and a captured, replayed bank."""
import numpy as np
import pytest
import torch

from tests import bank_checks as K

pytestmark = pytest.mark.gpu
KINDS = list(K.ROW_KINDS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", K.ROW_SIZES + K.PACKING_SIZES)
def test_resample_rows_matches_the_oracles_per_row_path(gpu, kind, n):
    K.check_rows_case(gpu, kind, "normal%d" % n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", K.ROW_SHAPES)
def test_resample_rows_on_gaps_holes_and_single_columns(gpu, kind, name):
    K.check_rows_case(gpu, kind, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", K.ROW_COUNTS)
def test_resample_rows_row_counts_around_the_packing(gpu, kind, rows):
    K.check_rows_case(gpu, kind, "count%d" % rows)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["normal5", "normal255", "normal1025", "mixed"])
def test_resample_rows_with_padded_rows(gpu, kind, name):
    """ld = n + 3, poison in the padding: rows start at odd 4-byte boundaries and the padding is never read"""
    K.check_rows_case(gpu, kind, name, pad=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["count7", "normal1023", "normal2051"])
def test_resample_rows_index_stride_gives_flat_indices(gpu, kind, name):
    K.check_rows_case(gpu, kind, name, stride=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["count7", "normal2051"])
def test_resample_rows_counts_a_row_without_mass(gpu, kind, name):
    K.check_rows_no_mass(gpu, kind, name)


def test_resample_rows_offsets_past_two_to_the_31(gpu):
    """rows = 3, n = 1025, ld = 2^30 + 8: row 2 starts at element 2^31 + 16.  The matrix is allocated, never filled; only
    the row heads are written.  32-bit offset arithmetic reads other words."""
    rows, n, ld = 3, 1025, 2 ** 30 + 8
    dev = gpu.device
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 16 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GB free on this device: the {rows * ld * 4 / 2 ** 30:.1f} GB matrix needs 16")
    heads = K.row_case("normal1025")[:rows]
    keys = K.row_keys(4)[:rows]
    lw = torch.empty((rows, ld), dtype=torch.float32, device=dev)
    lw[:, :n] = torch.from_numpy(np.array(heads)).to(dev)
    lw[:, n:n + 64] = float(K.B.POISON)
    k_d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(rows, 2)).to(dev)
    anc = torch.full((rows, n), -7, dtype=torch.int32, device=dev)
    mx = torch.zeros((rows,), dtype=torch.float32, device=dev)
    total = torch.zeros((rows,), dtype=torch.int64, device=dev)
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    kind = K.ROW_KINDS["systematic"]
    ws = torch.empty(((gpu.c.gmx_resample_rows_workspace(kind, rows, n) + 7) // 8,), dtype=torch.int64, device=dev)
    rc = gpu.c.gmx_resample_rows(kind, gpu.ptr(k_d), gpu.ptr(lw), rows, n, ld, 0, gpu.ptr(mx), gpu.ptr(total), gpu.ptr(anc),
                                 gpu.ptr(status), gpu.ptr(ws), gpu.stream())
    assert rc == 0, gpu.c.gmx_last_error()
    assert int(status.item()) == 0
    got = (anc.cpu().numpy(), mx.cpu().numpy(), [int(v) for v in total.cpu().tolist()], 0)
    K.assert_rows_equal(got, K.oracle_rows("systematic", "normal1025")[:rows], 0, n, "past 2^31")


@pytest.mark.parametrize("which", K.CHUNK_CALLS)
def test_rows_past_one_grid_of_65535_rows(gpu, which):
    """rows = 65537, n = 1025: the launches over (tile, row) go out in two chunks of rows; every row is one of three"""
    K.check_rows_chunks(gpu, which)


@pytest.mark.parametrize("kind", KINDS)
def test_resample_batched_equals_the_one_dimensional_calls(gpu, kind):
    K.check_resample_batched(gpu, kind)


def test_resample_batched_refusals_name_the_shapes_and_the_kinds(gpu):
    K.check_resample_batched_refusals(gpu)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["lgssm", "tracker"])
@pytest.mark.parametrize("n", [K.BANK_N, K.BANK_SMALL_N])
def test_bank_rows_equal_single_sweeps_bit_for_bit(gpu, model, kind, n):
    K.check_bank_against_sweeps(gpu, model, kind, n, specialize=True)


@pytest.mark.parametrize("model,kind,n", [("lgssm", "systematic", K.BANK_N), ("tracker", "stratified", K.BANK_SMALL_N),
                                          ("lgssm", "multinomial", K.BANK_N)])
def test_bank_captured_and_replayed_twice_equals_eager(gpu, model, kind, n):
    K.check_bank_against_sweeps(gpu, model, kind, n, specialize=True, capture=True)


def test_bank_params_are_per_filter_and_position_independent(gpu):
    K.check_params(gpu, specialize=True)


def test_bank_evidence_estimate_is_unbiased(gpu):
    K.check_law(gpu, specialize=True)


def test_bank_out_of_scope_options_raise_by_name(gpu):
    K.check_bank_refusals(gpu)
