"""What resampling many rows in one call buys, and what a bank of filters buys over a loop of sweeps.  JSON lines, appended
to --out:

  resample_rows   systematic, (rows, n) in {(4096, 256), (1024, 1024), (256, 4096), (16, 65536)}: gmx_resample_rows against
                  the loop of `rows` calls of gmx_resample on the same buffers (what there was before), alternated: the
                  median and the min / max of --reps windows after a warm-up, outputs asserted equal, and the rate of the
                  row bytes read plus the ancestors written (rows x n x 8 bytes) over the single call's median
  bank            BootstrapBank(R = 1024, n = 1024, T = 100) on the LGSSM of bench.py's config, captured, against
                  sequential captured BootstrapSweep(n = 1024) replays — SWEEPS of them (different keys, each captured
                  beforehand, untimed) replayed one after the other, the time SCALED by R / SWEEPS

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: SHAPES ("rows:n,..."), BR, BN,
BT, SWEEPS.  Needs the MI355X: there is no CPU path."""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
ap.add_argument("--skip-bank", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_time_resample_rows.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_resample_rows.py measures on the GPU only"
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


def spread(ts, scale=1e3):
    return {"median": scale * statistics.median(ts), "min": scale * min(ts), "max": scale * max(ts)}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


# ---- (a) the kernel -------------------------------------------------------------------------------------------------------
shapes = [tuple(int(v) for v in s.split(":")) for s in
          os.environ.get("SHAPES", "4096:256,1024:1024,256:4096,16:65536").split(",")]
kind = smc.SYSTEMATIC
for rows, n in shapes:
    gen = torch.Generator(device="cuda").manual_seed(11)
    lw = torch.randn((rows, n), device=dev, generator=gen) * 3.0
    keys = split(G.key(7), rows)
    keys_d, keys_h = keys.data(), keys.host()
    kk = [(c_uint32 * 2)(int(keys_h[r, 0]), int(keys_h[r, 1])) for r in range(rows)]
    shift = smc.cdf_shift(n)
    anc_b, anc_l = (torch.empty((rows, n), dtype=torch.int32, device=dev) for _ in range(2))
    mx_b, mx_l = (torch.empty((rows,), dtype=torch.float32, device=dev) for _ in range(2))
    tot_b, tot_l = (torch.empty((rows,), dtype=torch.int64, device=dev) for _ in range(2))
    status = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws_b = torch.empty(((be.c.gmx_resample_rows_workspace(kind, rows, n) + 7) // 8,), dtype=torch.int64, device=dev)
    ws_l = torch.empty(((be.c.gmx_resample_workspace(n) + 7) // 8,), dtype=torch.int64, device=dev)
    P, st = be.ptr, be.stream()
    rows_lw = [P(lw[r]) for r in range(rows)]
    rows_out = [(P(mx_l[r:]), P(tot_l[r:]), P(anc_l[r])) for r in range(rows)]

    def batched():
        be.check(be.c.gmx_resample_rows(kind, P(keys_d), P(lw), rows, n, n, 0, P(mx_b), P(tot_b), P(anc_b), P(status), P(ws_b),
                                        st), "gmx_resample_rows")

    def per_row():
        for r in range(rows):
            m_, t_, a_ = rows_out[r]
            be.check(be.c.gmx_resample(kind, kk[r], rows_lw[r], n, shift, None, 0, m_, t_, a_, P(ws_l), st), "gmx_resample")

    batched(), per_row()
    torch.cuda.synchronize()
    assert torch.equal(anc_b, anc_l) and torch.equal(tot_b, tot_l) and torch.equal(mx_b, mx_l), \
        "gmx_resample_rows and the per-row loop disagree"
    assert int(status.item()) == 0
    t1 = timed(batched, 10)
    per_window = max(10, min(2000, int(0.05 / max(t1, 1e-7))))          # ~50 ms of single calls per window
    loops = max(1, min(10, int(0.2 / max(timed(per_row), 1e-6))))
    tb, tl = [], []
    for _ in range(args.reps):                      # alternated: both forms see the same neighbours on the machine
        tb.append(timed(batched, per_window))
        tl.append(timed(per_row, loops))
    nbytes = rows * n * 8
    emit(dict(common, tool="time_resample_rows", what="resample_rows", kind="systematic", rows=rows, n=n,
              calls_per_window=per_window, loops_per_window=loops,
              gmx_resample_rows_us=spread(tb, 1e6), per_row_loop_us=spread(tl, 1e6),
              speedup=statistics.median(tl) / statistics.median(tb), separated_beyond_spread=bool(max(tb) < min(tl)),
              bytes_rows_read_plus_ancestors_written=nbytes, GBps=nbytes / statistics.median(tb) / 1e9, outputs_equal=True))
    del lw, anc_b, anc_l

# ---- (b) the sweep ----------------------------------------------------------------------------------------------------------
if not args.skip_bank:
    R, n, T = int(os.environ.get("BR", 1024)), int(os.environ.get("BN", 1024)), int(os.environ.get("BT", 100))
    K = int(os.environ.get("SWEEPS", 32))
    init, step = workloads.make_lgssm(G)
    ys = torch.from_numpy(workloads.lgssm_data(T))
    keys = split(G.key(314159), R)
    bank = smc.BootstrapBank(init, step, n, R, T).prepare(keys, ys).capture()
    sweeps = [smc.BootstrapSweep(init, step, n, T).prepare(keys[r], ys).capture() for r in range(K)]

    def loop():
        for sw in sweeps:
            sw.launch()

    bank.launch(), loop()
    torch.cuda.synchronize()
    ref = bank.log_ml()
    assert all(ref[r] == sweeps[r].log_ml() for r in range(K)), "the bank and the single sweeps disagree"
    tb, tl = [], []
    for _ in range(args.reps):
        tb.append(timed(bank.launch, 3))
        tl.append(timed(loop, 3))
    scale = R / K
    emit(dict(common, tool="time_resample_rows", what="bank", R=R, n=n, T=T, resample="systematic",
              bank_ms=spread(tb), loop_of_sweeps_timed=K, loop_of_K_sweeps_ms=spread(tl),
              loop_of_R_sweeps_ms_SCALED=statistics.median(tl) * scale * 1e3,
              note="the loop's time is the replay of K captured single sweeps, scaled by R / K; their prepare() and capture() "
                   "are not in it",
              sweep_form={"noise_ahead": bool(sweeps[0].noise_ahead), "fuse": bool(sweeps[0].fuse)},
              speedup=statistics.median(tl) * scale / statistics.median(tb),
              us_per_step_bank=1e6 * statistics.median(tb) / T,
              particle_steps_per_s_bank=R * n * T / statistics.median(tb), log_ml_equal=True))
