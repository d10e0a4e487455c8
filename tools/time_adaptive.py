"""What deciding the resampling per row costs.  JSON lines, appended to --out:

  sweep   (R, n) in {(4096, 256), (1024, 1024)}, T = 100, LGSSM, captured sweeps alternated in one process:
            plain            BootstrapBank without ess_threshold= (gmx_resample_rows per step: the sweep as it was)
            fused_always     BootstrapBank(ess_threshold=inf): gmx_resample_rows_ess, every row resampled — the same work
                             as `plain` plus the carry row's load and store, the three sums and the decision
            composed_always  the same step from separate launches (a subclass here): lw += carry (one elementwise launch),
                             plain gmx_resample_rows, one elementwise gating launch that writes the carry.  It computes NO
                             decision and gates no ancestors (at "always" neither changes a value), so it is a FLOOR for a
                             composed adaptive step
            fused_mid        BootstrapBank(ess_threshold=0.5), for the record: the rows that are not resampled skip their
                             slot searches
          `plain`, `fused_always` and `composed_always` are asserted equal in state and log_ml.  Microseconds per step:
          the median and min / max of --reps alternated windows; `spread_over_median`: (max - min) / median of each form's
          windows — the fused / composed ratio is read against the plain bank's.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: AD_SHAPES ("R:n,..."), AD_T.
Needs the MI355X: there is no CPU path."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import genjax_amd as G
from genjax_amd import _lib, workloads
from genjax_amd.inference import smc
from genjax_amd.random import split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--label", default="")
ap.add_argument("--kind", default="systematic")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_time_adaptive.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_adaptive.py measures on the GPU only"
be = _lib.get()
common = {"label": args.label, "reps": args.reps, "device": torch.cuda.get_device_name(0), "kind": args.kind,
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
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


class ComposedAlwaysBank(smc.BootstrapBank):
    """ess_threshold=inf with gmx_resample_rows_ess replaced by separate launches (see the module docstring)"""

    def prepare(self, keys, ys):
        super().prepare(keys, ys)
        self.keep = torch.zeros((self.R, 1), dtype=torch.float32, device=self.lw.device)      # "always": nothing is kept
        self.flags.fill_(1)
        return self

    def _resample(self, t):
        R, n = self.R, self.n
        lw, carry = self.lw.reshape(R, n), self.carry.reshape(R, n)
        torch.add(lw, carry, out=lw)
        smc.resample_rows(self.kind, self.step_keys[t][1], lw, index_stride=n,
                          out=(self.anc, self.totals[t], self.maxs[t], self.status), workspace=self.ws)
        torch.mul(lw, self.keep, out=carry)


T = int(os.environ.get("AD_T", 100))
init, step = workloads.make_lgssm(G)
ys = torch.from_numpy(workloads.lgssm_data(T))
for R, n in [tuple(int(v) for v in s.split(":")) for s in os.environ.get("AD_SHAPES", "4096:256,1024:1024").split(",")]:
    keys = split(G.key(314159), R)
    banks = {"plain": smc.BootstrapBank(init, step, n, R, T, resample=args.kind),
             "fused_always": smc.BootstrapBank(init, step, n, R, T, resample=args.kind, ess_threshold=math.inf),
             "composed_always": ComposedAlwaysBank(init, step, n, R, T, resample=args.kind, ess_threshold=math.inf),
             "fused_mid": smc.BootstrapBank(init, step, n, R, T, resample=args.kind, ess_threshold=0.5)}
    for b in banks.values():
        b.prepare(keys, ys).capture()
    forms = {name: b.launch for name, b in banks.items()}
    for _ in range(3):                              # warm-up
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    pl = banks["plain"]
    for name in ("fused_always", "composed_always"):
        b = banks[name]
        assert torch.equal(b.lw, pl.lw) and torch.equal(b.anc, pl.anc), name + " and the plain bank disagree"
        assert (b.log_ml() == pl.log_ml()).all(), name + " and the plain bank disagree in log_ml"
    resampled_mid = float(banks["fused_mid"].resampled().float().mean())
    ts = {name: [] for name in forms}
    for _ in range(args.reps):                      # alternated: every form sees the same neighbours on the machine
        for name, f in forms.items():
            ts[name].append(timed(f, 3))
    med = {name: statistics.median(v) for name, v in ts.items()}
    emit(dict(common, tool="time_adaptive", what="sweep", R=R, n=n, T=T,
              us_per_step={name: {"median": 1e6 * med[name] / T, "min": 1e6 * min(v) / T, "max": 1e6 * max(v) / T}
                           for name, v in ts.items()},
              spread_over_median={name: (max(v) - min(v)) / med[name] for name, v in ts.items()},
              fused_over_composed=med["fused_always"] / med["composed_always"],
              fused_over_plain=med["fused_always"] / med["plain"],
              launches_per_step={"plain": 2, "fused_always": 2, "composed_always": 4, "fused_mid": 2},
              resampled_fraction_mid=resampled_mid, always_equals_plain=True))
    del banks, forms, pl
