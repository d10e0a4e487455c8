"""What the batched row-wise draw buys and what backward simulation costs.  Two JSON lines, appended to --out:

  pick_rows        gmx_pick_rows at rows = 64, n = 1e6 (two launches, no CDF array) against a loop of 64 calls of the
                   per-row path (gmx_logsumexp + gmx_weight_cdf + gmx_ancestors, one index each), alternated: the median
                   and the min / max of --reps windows of --launches calls after a warm-up, the rate of the
                   rows x n x 4 bytes the statistics pass must read, outputs asserted equal
  backward_sample  SweepHistory.backward_sample at n = 1e5, T = 100, m = 64: time per step, and the distinct step-0
                   particles on the m trajectories against lineage()'s on m of the survivors

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: ROWS, N (pick_rows), BN, BT,
BM (backward_sample).  Needs the MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_uint32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import genjax_amd as G
from genjax_amd import _lib, workloads
from genjax_amd.inference import smc
from genjax_amd.random import split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=10, help="calls per timed window of the kernel comparison")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_time_backward.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_backward.py measures on the GPU only"
be = _lib.get()
dev = be.device
common = {"label": args.label, "reps": args.reps, "device": torch.cuda.get_device_name(0),
          "library": os.path.basename(_lib.LIB_PATH)}


def timed(fn, launches=1):
    """seconds per call over a window of `launches` back-to-back calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / launches


def emit(rec):
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


# ---- (a) the kernel -------------------------------------------------------------------------------------------------------
rows, n = int(os.environ.get("ROWS", 64)), int(os.environ.get("N", 1_000_000))
gen = torch.Generator(device="cuda").manual_seed(11)
logits = torch.randn((rows, n), device=dev, generator=gen) * 3.0
keys = split(G.key(7), rows)
keys_d = keys.data()
keys_h = keys.host()
out_b = torch.empty((rows,), dtype=torch.int32, device=dev)
out_l = torch.empty((rows,), dtype=torch.int32, device=dev)
status = torch.zeros((1,), dtype=torch.int64, device=dev)
ws = torch.empty(((be.c.gmx_pick_rows_workspace(rows, n) + 7) // 8,), dtype=torch.int64, device=dev)


def batched():
    be.check(be.c.gmx_pick_rows(be.ptr(keys_d), be.ptr(logits), rows, n, n, be.ptr(out_b), be.ptr(status), be.ptr(ws),
                                be.stream()), "gmx_pick_rows")


def per_row():
    for r in range(rows):
        cdf, total, _, _ = smc.weight_cdf(logits[r])
        kk = (c_uint32 * 2)(int(keys_h[r, 0]), int(keys_h[r, 1]))
        be.check(be.c.gmx_ancestors(smc.MULTINOMIAL, kk, be.ptr(cdf), n, 0, be.ptr(total), 1, 0, 1, be.ptr(out_l[r:]),
                                    be.stream()), "gmx_ancestors")


batched(), per_row()
torch.cuda.synchronize()
assert torch.equal(out_b, out_l), "gmx_pick_rows and the per-row path disagree"
assert int(status.item()) == 0
tb, tl = [], []
for _ in range(args.reps):                      # alternated: both forms see the same neighbours on the machine
    tb.append(timed(batched, args.launches))
    tl.append(timed(per_row, args.launches))
nbytes = rows * n * 4
emit(dict(common, tool="time_backward", what="pick_rows", rows=rows, n=n, launches_per_window=args.launches,
          gmx_pick_rows_ms={"median": 1e3 * statistics.median(tb), "min": 1e3 * min(tb), "max": 1e3 * max(tb)},
          per_row_loop_ms={"median": 1e3 * statistics.median(tl), "min": 1e3 * min(tl), "max": 1e3 * max(tl)},
          speedup=statistics.median(tl) / statistics.median(tb),
          separated_beyond_spread=bool(max(tb) < min(tl)),
          stats_pass_bytes=nbytes, GBps_of_stats_bytes=nbytes / statistics.median(tb) / 1e9, outputs_equal=True))
del logits

# ---- (b) end to end ---------------------------------------------------------------------------------------------------------
bn, bT, bm = int(os.environ.get("BN", 100_000)), int(os.environ.get("BT", 100)), int(os.environ.get("BM", 64))
init, step = workloads.make_lgssm(G)
sw = smc.BootstrapSweep(init, step, bn, bT, history=True).prepare(G.key(314159), torch.from_numpy(workloads.lgssm_data(bT)))
sw.launch()
h = sw.history()
run = lambda: h.backward_sample(G.key(99), bm, return_paths=True)
run()                                           # warm: traces (and specialises) the density programs
ts = [timed(run) for _ in range(args.reps)]
paths = run()[0]
lin = h.lineage(h.ancestors[bT - 1][:bm])
emit(dict(common, tool="time_backward", what="backward_sample", n=bn, T=bT, m=bm,
          rows_per_launch=max(1, min(smc.BACKWARD_ROWS_MAX, bm, smc.BACKWARD_CHUNK_BYTES // (4 * bn), 40)),
          total_ms={"median": 1e3 * statistics.median(ts), "min": 1e3 * min(ts), "max": 1e3 * max(ts)},
          us_per_step=1e6 * statistics.median(ts) / (bT - 1),
          distinct_step0={"backward_sample": int(torch.unique(paths[0]).numel()),
                          "lineage_of_m_survivors": int(torch.unique(lin[0]).numel()),
                          "lineage_of_all_n_survivors": int(torch.unique(h.lineage()[0]).numel())}))
