"""What the fixed-lag smoother costs a bank's sweep, beside what the moments cost.  JSON lines, appended to --out:

  sweep   R = 256, T = 100, (model, n) in {(lgssm, 1024): D = 1; (tracker, 1024), (tracker, 4096): D = 2, position and
          velocity}; three captured sweeps alternated in one process:
            plain       BootstrapBank(...)                       the sweep as it is without a keyword
            moments     BootstrapBank(..., moments=True)         plus gmx_rows_moments per step
            smooth_lag  BootstrapBank(..., smooth_lag=8)         plus gmx_rows_lag_moments per step (n = 1024: one launch, seven
                                                                 ancestor tables in LDS; n = 4096: two, the walk in global memory)
          The three are asserted equal in state and log_ml.  Microseconds per step: the median and min / max of --reps
          alternated windows of --window sweeps after a warm-up; `added_us_per_step` is each keyword's median minus the plain
          median — the cost of the launch IN the captured chain (launch gap included), not a kernel time.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: LT_SHAPES ("model:R:n,..."), LT_T, LT_LAG.
Needs the MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import genjax_amd as G
from genjax_amd import workloads
from genjax_amd.inference import smc
from genjax_amd.random import split
from tests import bank_checks

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lag_time.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_lag.py measures on the GPU only"
T = int(os.environ.get("LT_T", "100"))
LAG = int(os.environ.get("LT_LAG", "8"))
shapes = [(s.split(":")[0],) + tuple(int(v) for v in s.split(":")[1:])
          for s in os.environ.get("LT_SHAPES", "lgssm:256:1024,tracker:256:1024,tracker:256:4096").split(",")]


def window(fn, launches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / launches


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


ys = torch.from_numpy(workloads.lgssm_data(T))
for model, R, n in shapes:
    init, step = bank_checks._models(model)
    banks = {}
    for name, kw in (("plain", {}), ("moments", {"moments": True}), ("smooth_lag", {"smooth_lag": LAG})):
        b = smc.BootstrapBank(init, step, n, R, T, **kw).prepare(split(G.key(7), R), ys)
        b.capture()
        b.launch()
        banks[name] = b
    torch.cuda.synchronize()
    sp = bank_checks._np_state(banks["plain"].state())
    for b in banks.values():
        sb = bank_checks._np_state(b.state())
        assert all(np.array_equal(u, v) for u, v in zip(sp, sb)) and np.array_equal(banks["plain"].log_ml(), b.log_ml())
    for b in banks.values():                             # warm-up of the timed form
        window(b.launch, args.window)
    us = {k: [] for k in banks}
    for _ in range(args.reps):
        for k, b in banks.items():
            us[k].append(window(b.launch, args.window) / T * 1e6)
    med = {k: statistics.median(v) for k, v in us.items()}
    smo = banks["smooth_lag"].smoothed_mean().reshape(T, R, -1)
    rec = {"label": args.label, "tool": "time_lag", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "window": args.window, "model": model, "R": R, "n": n, "T": T, "D": banks["smooth_lag"].store.D, "lag": LAG,
           "us_per_step": {k: stats(v) for k, v in us.items()},
           "added_us_per_step": {k: med[k] - med["plain"] for k in ("moments", "smooth_lag")},
           "mean_smoothed_first_step": [float(v) for v in smo[0].mean(dim=0)]}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
