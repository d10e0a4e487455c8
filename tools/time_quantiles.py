"""What recording the filtering quantiles costs a bank's sweep, beside what the moments cost.  JSON lines, appended to --out:

  sweep   R = 256, D = 1 (LGSSM), T = 100, n in {256, 1024}; three captured sweeps alternated in one process:
            plain      BootstrapBank(...)                                     the sweep as it is without a keyword
            moments    BootstrapBank(..., moments=True)                       plus gmx_rows_moments per step
            quantiles  BootstrapBank(..., quantiles=(0.025, 0.5, 0.975))      plus gmx_rows_quantiles per step (n = 256: a row
                                                                              sorts inside one wave; n = 1024: four waves)
          The three are asserted equal in state and log_ml.  Microseconds per step: the median and min / max of --reps
          alternated windows of --window sweeps after a warm-up; `added_us_per_step` is each keyword's median minus the plain
          median — the cost of the launch IN the captured chain (launch gap included), not a kernel time.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: QT_SHAPES ("R:n,..."), QT_T.
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantiles_time.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_quantiles.py measures on the GPU only"
T = int(os.environ.get("QT_T", "100"))
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("QT_SHAPES", "256:256,256:1024").split(",")]
PROBS = (0.025, 0.5, 0.975)


def window(fn, launches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / launches


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


init, step = workloads.make_lgssm(G)
ys = torch.from_numpy(workloads.lgssm_data(T))
for R, n in shapes:
    banks = {}
    for name, kw in (("plain", {}), ("moments", {"moments": True}), ("quantiles", {"quantiles": PROBS})):
        b = smc.BootstrapBank(init, step, n, R, T, **kw).prepare(split(G.key(7), R), ys)
        b.capture()
        b.launch()
        banks[name] = b
    torch.cuda.synchronize()
    sp = banks["plain"].state()
    for b in banks.values():
        assert all(torch.equal(u, v) for u, v in zip(sp, b.state())) and np.array_equal(banks["plain"].log_ml(), b.log_ml())
    for b in banks.values():                             # warm-up of the timed form
        window(b.launch, args.window)
    us = {k: [] for k in banks}
    for _ in range(args.reps):
        for k, b in banks.items():
            us[k].append(window(b.launch, args.window) / T * 1e6)
    med = {k: statistics.median(v) for k, v in us.items()}
    band = banks["quantiles"].filter_quantiles()[T - 1]
    rec = {"label": args.label, "tool": "time_quantiles", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "window": args.window, "R": R, "n": n, "T": T, "D": banks["quantiles"].store.D, "levels": PROBS,
           "us_per_step": {k: stats(v) for k, v in us.items()},
           "added_us_per_step": {k: med[k] - med["plain"] for k in ("moments", "quantiles")},
           "mean_band_last_step": [float(v) for v in band.double().mean(dim=0)]}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
