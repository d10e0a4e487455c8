"""What one particle-MH iteration costs on the device, against the same iteration driven from the host and against the bank
sweep inside it.  JSON lines, appended to --out:

  iteration   (R, n, T) from PM_SHAPES, the LGSSM with two unknown parameters and uniform priors, alternated in one process:
                captured     smc.ParticleMH, one iteration = one graph replay (gmx_pmmh_propose, the prior program, the
                             bank's sweep, gmx_pmmh_accept); nothing is read on the host
                host         the same iteration composed on the host around the SAME captured bank sweep: the T x R key
                             tables re-derived on the host and uploaded, the proposals drawn in numpy and the parameter
                             leaves uploaded, the sweep replayed, BootstrapBank.log_ml() read back (synchronises), the
                             prior and the decision in numpy
                plain_sweep  the captured BootstrapBank sweep alone at the same R x n x T (smc.BootstrapBank is the parent
                             commit's, line for line: this change does not touch it)
              Microseconds per iteration: the median and min / max of --reps alternated windows; `spread_over_median`:
              (max - min) / median of each form's windows — a ratio is read against it.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: PM_SHAPES ("R:n:T,...").
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
from genjax_amd.random import Key, _derive_host, split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=int, default=20, help="iterations per timed window")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pmmh_time.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_pmmh.py measures on the GPU only"
be = _lib.get()
common = {"label": args.label, "reps": args.reps, "window": args.window, "device": torch.cuda.get_device_name(0),
          "library": os.path.basename(_lib.LIB_PATH)}

P0 = workloads.LGSSM
PRIOR = ((0.5, 0.99), (0.2, 1.0))
STEP_SIZE = (0.05, 0.1)


@G.gen
def init(a, sx):
    x = G.normal(0.0, P0["s0"]) @ "x"
    _ = G.normal(x, P0["sy"]) @ "y"
    return x


@G.gen
def step(x_prev, a, sx):
    x = G.normal(a * x_prev, sx) @ "x"
    _ = G.normal(x, P0["sy"]) @ "y"
    return x


@G.gen
def prior():
    a = G.uniform(*PRIOR[0]) @ "a"
    _ = G.uniform(*PRIOR[1]) @ "sx"
    return a


def timed(fn, calls):
    """seconds per call over a window of `calls` back-to-back calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


class HostPMMH:
    """the iteration composed on the host around a captured bank sweep (see the module docstring)"""

    def __init__(self, R, n, T, ys, theta0, key):
        self.R, self.n, self.key = R, n, np.asarray(key.host(), np.uint32)
        self.bank = smc.BootstrapBank(init, step, n, R, T, params=tuple(torch.from_numpy(v.copy()) for v in theta0))
        self.bank.prepare(split(key, R), ys).capture()
        self.theta, self.ll, self.lp = theta0.copy(), np.full((R,), -np.inf), np.zeros((R,))
        self.rng = np.random.default_rng(1)
        self.j = 0

    def iterate(self):
        b, R = self.bank, self.R
        ks = _derive_host(_derive_host(self.key, np.uint64(self.j))[None, :], np.arange(3, dtype=np.uint64))
        prop, res = b._key_tables(Key(host=_derive_host(ks[0][None, :], np.arange(R, dtype=np.uint64))))
        b.keys_prop.copy_(torch.from_numpy(prop), non_blocking=True)
        b.keys_res.copy_(torch.from_numpy(res), non_blocking=True)
        th = self.theta if self.j == 0 else \
            (self.theta + np.asarray(STEP_SIZE, np.float32)[:, None] * self.rng.normal(size=self.theta.shape)).astype(np.float32)
        for p in range(th.shape[0]):
            b.params_full[p].copy_(torch.from_numpy(np.repeat(th[p], self.n)), non_blocking=True)
        b.launch()
        ll_new = b.log_ml()                                              # synchronises
        inside = np.all([(th[p] >= PRIOR[p][0]) & (th[p] <= PRIOR[p][1]) for p in range(th.shape[0])], axis=0)
        lp_new = np.where(inside, -sum(np.log(hi - lo) for lo, hi in PRIOR), -np.inf)
        with np.errstate(invalid="ignore", divide="ignore"):
            take = np.log(self.rng.uniform(size=(R,))) < (ll_new - self.ll) + (lp_new - self.lp)
        self.theta = np.where(take[None, :], th, self.theta)
        self.ll, self.lp = np.where(take, ll_new, self.ll), np.where(take, lp_new, self.lp)
        self.j += 1


for R, n, T in [tuple(int(v) for v in s.split(":")) for s in os.environ.get("PM_SHAPES", "1024:64:8,256:256:25").split(",")]:
    ys = torch.from_numpy(workloads.lgssm_data(T))
    rng = np.random.default_rng(R)
    theta0 = np.stack([rng.uniform(lo + 0.05, hi - 0.05, size=(R,)) for lo, hi in PRIOR]).astype(np.float32)
    budget = 8 + (args.reps + 3) * args.window
    pm = smc.ParticleMH(init, step, prior, n, R, T, ("a", "sx"), STEP_SIZE)
    pm.prepare(G.key(2718), ys, tuple(torch.from_numpy(v.copy()) for v in theta0), budget).capture()
    host = HostPMMH(R, n, T, ys, theta0, G.key(2718))
    plain = smc.BootstrapBank(init, step, n, R, T, params=tuple(torch.from_numpy(v.copy()) for v in theta0))
    plain.prepare(split(G.key(2718), R), ys).capture()
    forms = {"captured": pm.launch, "host": host.iterate, "plain_sweep": plain.launch}
    for f in forms.values():                            # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in forms}
    for _ in range(args.reps):                          # alternated: every form sees the same neighbours on the machine
        for name, f in forms.items():
            ts[name].append(timed(f, args.window))
    assert int(pm.status.item()) == 0 and int(pm.it[0].item()) == 3 + args.reps * args.window
    med = {name: statistics.median(v) for name, v in ts.items()}
    emit(dict(common, tool="time_pmmh", what="iteration", R=R, n=n, T=T,
              us_per_iteration={name: {"median": 1e6 * med[name], "min": 1e6 * min(v), "max": 1e6 * max(v)} for name, v in ts.items()},
              spread_over_median={name: (max(v) - min(v)) / med[name] for name, v in ts.items()},
              captured_over_host=med["captured"] / med["host"], captured_over_plain_sweep=med["captured"] / med["plain_sweep"]))
    del pm, host, plain, forms
