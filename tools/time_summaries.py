"""What recording one of a bank's per-step summaries costs its sweep, beside what the moments cost.  JSON lines, appended to --out
(default profiles/<summary>_time.jsonl; the lines carry the fields and the "tool" name of the four scripts this one replaced —
time_moments, time_quantiles, time_covariance, time_lag — so they stay comparable with the recorded ones):

  --summary moments     BootstrapBank(..., moments=True)                    gmx_rows_moments per step (two launches past n = 1024)
            quantiles   BootstrapBank(..., quantiles=(0.025, 0.5, 0.975))   gmx_rows_quantiles per step (n = 256: a row sorts inside
                                                                            one wave; n = 1024: four waves)
            covariance  BootstrapBank(..., covariance=True)                 gmx_rows_covariance per step (n = 1024: one launch, the
                                                                            Gram matrix on the float64 matrix instruction; past it: two)
            smooth_lag  BootstrapBank(..., smooth_lag=8)                    gmx_rows_lag_moments per step (n = 1024: one launch, the
                                                                            ancestor tables in LDS; past it: two, the walk in global memory)
            smooth_pairs  BootstrapBank(..., smooth_lag=8, smooth_pairs=True)   gmx_rows_lag_pairs after it, from step 8 on (three Gram
                                                                            matrices gathered along the walk); timed beside
                                                                            smooth_lag=8 and covariance=True, whose work it does

  sweep   R = 256, T = 100, per shape three captured sweeps alternated in one process (two for --summary moments):
            plain       BootstrapBank(...)                   the sweep as it is without a keyword
            moments     BootstrapBank(..., moments=True)
            <summary>   the chosen keyword
          They are asserted equal in state and log_ml.  Microseconds per step: the median and min / max of --reps alternated
          windows of --window sweeps after a warm-up; `added_us_per_step` is each keyword's median minus the plain median — the
          cost of the launch IN the captured chain (launch gap included), not a kernel time.  Default shapes (model:R:n; lgssm:
          D = 1, tracker: D = 2, position and velocity):
            moments                 lgssm:256:1024,lgssm:256:4096     (with the launch's algorithmic bytes, R n 4 (1 + D) read +
                                                                      R 8 (1 + 2 D) written, over the added time)
            quantiles               lgssm:256:256,lgssm:256:1024
            covariance, smooth_lag, smooth_pairs  lgssm:256:1024,tracker:256:1024,tracker:256:4096

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: TS_SHAPES ("model:R:n,..."), TS_T,
TS_LAG.  Needs the MI355X: there is no CPU path."""
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

T = int(os.environ.get("TS_T", "100"))
LAG = int(os.environ.get("TS_LAG", "8"))
PROBS = (0.025, 0.5, 0.975)
WIDE = "lgssm:256:1024,tracker:256:1024,tracker:256:4096"


def moments_fields(b, R, n, added):
    nbytes = R * n * 4 * (1 + b.store.D) + R * 8 * (1 + 2 * b.store.D)
    return {"added_us_per_step": added["moments"], "moments_bytes": nbytes,
            "moments_bytes_per_s": nbytes / (added["moments"] * 1e-6) if added["moments"] > 0 else None,
            "mean_ess_last_step": float(b.ess()[T - 1].mean())}


# per summary: the old script's name, the keyword, the default shapes, the fields the old script wrote before us_per_step
# (besides R, n, T, D) and the ones after it
SUMMARIES = {
    "moments": ("time_moments", {"moments": True}, "lgssm:256:1024,lgssm:256:4096", lambda model: {}, moments_fields),
    "quantiles": ("time_quantiles", {"quantiles": PROBS}, "lgssm:256:256,lgssm:256:1024", lambda model: {"levels": PROBS},
                  lambda b, R, n, added: {"mean_band_last_step": [float(v) for v in b.filter_quantiles()[T - 1].double().mean(dim=0)]}),
    "covariance": ("time_covariance", {"covariance": True}, WIDE, lambda model: {"model": model},
                   lambda b, R, n, added: {"mean_cov_last_step": [float(v) for v in b.filter_cov()[T - 1].mean(dim=0).reshape(-1)]}),
    "smooth_lag": ("time_lag", {"smooth_lag": LAG}, WIDE, lambda model: {"model": model, "lag": LAG},
                   lambda b, R, n, added: {"mean_smoothed_first_step": [float(v) for v in b.smoothed_mean().reshape(T, R, -1)[0].mean(dim=0)]}),
    "smooth_pairs": ("time_lag", {"smooth_lag": LAG, "smooth_pairs": True}, WIDE, lambda model: {"model": model, "lag": LAG},
                     lambda b, R, n, added: {"mean_cross_first_pair": [float(v) for v in b.smoothed_pairs().cross[0].mean(dim=0).reshape(-1)]}),
}
# the keywords a summary is timed beside, in the same alternation (besides plain and moments)
BESIDE = {"smooth_pairs": {"smooth_lag": {"smooth_lag": LAG}, "covariance": {"covariance": True}}}

ap = argparse.ArgumentParser()
ap.add_argument("--summary", required=True, choices=sorted(SUMMARIES))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
tool, keyword, default_shapes, shape_fields, result_fields = SUMMARIES[args.summary]
out_path = args.out or os.path.join(ROOT, "profiles", f"{tool[5:]}_time.jsonl")
assert torch.cuda.is_available(), "tools/time_summaries.py measures on the GPU only"
shapes = [(s.split(":")[0],) + tuple(int(v) for v in s.split(":")[1:]) for s in os.environ.get("TS_SHAPES", default_shapes).split(",")]


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
    for name, kw in {"plain": {}, "moments": {"moments": True}, **BESIDE.get(args.summary, {}), args.summary: keyword}.items():
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
    added = {k: med[k] - med["plain"] for k in banks if k != "plain"}
    rec = {"label": args.label, "tool": tool, "device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window,
           "R": R, "n": n, "T": T, "D": banks[args.summary].store.D, **shape_fields(model),
           "us_per_step": {k: stats(v) for k, v in us.items()}, "added_us_per_step": added,
           **result_fields(banks[args.summary], R, n, added)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as fh:
        fh.write(line + "\n")
