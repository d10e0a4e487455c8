"""What recording the filtering moments costs a bank's sweep.  JSON lines, appended to --out:

  sweep   R = 256, D = 1 (LGSSM), T = 100, n in {1024, 4096}; two captured sweeps alternated in one process:
            plain     BootstrapBank(...)                 the sweep as it is without the keyword
            moments   BootstrapBank(..., moments=True)   the same sweep plus gmx_rows_moments per step (n = 1024: one launch,
                                                         n = 4096: two)
          The two are asserted equal in state and log_ml.  Microseconds per step: the median and min / max of --reps
          alternated windows of --window sweeps after a warm-up; `added_us_per_step` is the difference of the medians and
          `moments_bytes_per_s` the launch's algorithmic bytes, R n 4 (1 + D) read + R 8 (1 + 2 D) written, over it — the
          cost of the launch IN the captured chain (launch gap included), not a kernel time.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: MO_SHAPES ("R:n,..."), MO_T.
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
from genjax_amd import _lib, workloads
from genjax_amd.inference import smc
from genjax_amd.random import split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_time.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_moments.py measures on the GPU only"
be = _lib.get()
T = int(os.environ.get("MO_T", "100"))
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("MO_SHAPES", "256:1024,256:4096").split(",")]


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
    for name, kw in (("plain", {}), ("moments", {"moments": True})):
        b = smc.BootstrapBank(init, step, n, R, T, **kw).prepare(split(G.key(7), R), ys)
        b.capture()
        b.launch()
        banks[name] = b
    torch.cuda.synchronize()
    sp, sm = banks["plain"].state(), banks["moments"].state()
    assert all(torch.equal(a, b) for a, b in zip(sp, sm)) and np.array_equal(banks["plain"].log_ml(), banks["moments"].log_ml())
    for b in banks.values():                             # warm-up of the timed form
        window(b.launch, args.window)
    us = {k: [] for k in banks}
    for _ in range(args.reps):
        for k, b in banks.items():
            us[k].append(window(b.launch, args.window) / T * 1e6)
    D = banks["moments"].store.D
    added = statistics.median(us["moments"]) - statistics.median(us["plain"])
    nbytes = R * n * 4 * (1 + D) + R * 8 * (1 + 2 * D)
    rec = {"label": args.label, "tool": "time_moments", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "window": args.window, "R": R, "n": n, "T": T, "D": D, "us_per_step": {k: stats(v) for k, v in us.items()},
           "added_us_per_step": added, "moments_bytes": nbytes,
           "moments_bytes_per_s": nbytes / (added * 1e-6) if added > 0 else None,
           "mean_ess_last_step": float(banks["moments"].ess()[T - 1].mean())}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
