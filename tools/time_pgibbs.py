"""What one particle-Gibbs iteration costs, against the same iteration driven from the host and against the conditional sweep
inside it.  JSON lines, appended to --out:

  iteration   (R, n, T) from PG_SHAPES, the LGSSM with the transition coefficient and the observation scale unknown and
              uniform priors, alternated in one process, every form around a captured conditional sweep:
                pg          smc.ParticleGibbs, one iteration: gmx_pg_open, the sweep, draw, retain, gmx_pg_propose, the
                            prior program, the T score programs, gmx_pg_accept
                host        the same iteration composed on the host: ConditionalBank.rekey() (the 3 T R keys derived in numpy
                            and uploaded), the parameter leaves uploaded, the sweep, draw, retain, the proposal, the scores
                            and the decision in numpy on the drawn paths, ConditionalBank.set_retained() for the pinned
                            weights under the accepted parameters (its host loop of importance + project)
                sweep_only  launch(); draw(); retain() on a ConditionalBank of the same shape
              Microseconds per iteration: the median and min / max of --reps alternated windows; `spread_over_median`:
              (max - min) / median of each form's windows — a ratio is read against it.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: PG_SHAPES ("R:n:T,...").
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
from genjax_amd.random import fold_in, split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--window", type=int, default=10, help="iterations per timed window")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgibbs_time.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_pgibbs.py measures on the GPU only"
be = _lib.get()
common = {"label": args.label, "reps": args.reps, "window": args.window, "device": torch.cuda.get_device_name(0),
          "library": os.path.basename(_lib.LIB_PATH)}

P0 = workloads.LGSSM
PRIOR = ((0.5, 0.99), (0.5, 2.0))
STEP_SIZE = (0.05, 0.1)


@G.gen
def init(a, sy):
    x = G.normal(0.0, P0["s0"]) @ "x"
    _ = G.normal(x, sy) @ "y"
    return x


@G.gen
def step(x_prev, a, sy):
    x = G.normal(a * x_prev, P0["sx"]) @ "x"
    _ = G.normal(x, sy) @ "y"
    return x


@G.gen
def prior():
    a = G.uniform(*PRIOR[0]) @ "a"
    _ = G.uniform(*PRIOR[1]) @ "sy"
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


def conditional_bank(R, n, T, ys, theta0, key):
    """a ConditionalBank with a retained path (one unconditional sweep drawn and retained), its conditional sweep captured"""
    bank = smc.ConditionalBank(init, step, n, R, T, params=tuple(torch.from_numpy(v.copy()) for v in theta0))
    bank.prepare(split(key, R), ys).launch()
    bank.draw(key)
    bank.retain()
    return bank.capture()


class SweepOnly:
    def __init__(self, R, n, T, ys, theta0, key):
        self.bank, self.key, self.j = conditional_bank(R, n, T, ys, theta0, key), key, 0

    def iterate(self):
        b = self.bank
        b.launch()
        b.draw(fold_in(self.key, self.j))
        b.retain()
        self.j += 1


class HostPG:
    """the iteration composed on the host (see the module docstring)"""

    def __init__(self, R, n, T, ys, theta0, key):
        self.R, self.n, self.T, self.key = R, n, T, key
        self.bank = conditional_bank(R, n, T, ys, theta0, key)
        self.ys = np.asarray(ys, np.float64)
        self.theta = theta0.copy()
        self.rng = np.random.default_rng(1)
        self.j = 0

    def log_joint(self, th, x):
        a, sy = th[0].astype(np.float64)[:, None], th[1].astype(np.float64)[:, None]
        out = (-0.5 * ((self.ys[None, :] - x) / sy) ** 2 - np.log(sy)).sum(axis=1)
        return out + (-0.5 * ((x[:, 1:] - a * x[:, :-1]) / P0["sx"]) ** 2).sum(axis=1)

    def iterate(self):
        b, R = self.bank, self.R
        ks = split(fold_in(self.key, self.j), 2)
        b.rekey(split(ks[0], R))
        for p in range(2):
            b.params_full[p].copy_(torch.from_numpy(np.repeat(self.theta[p], self.n)), non_blocking=True)
        b.launch()
        x_d = b.draw(ks[1])                                              # synchronises
        b.retain()
        x = x_d.cpu().numpy().astype(np.float64)
        th = (self.theta + np.asarray(STEP_SIZE, np.float32)[:, None] * self.rng.normal(size=self.theta.shape)).astype(np.float32)
        inside = np.all([(th[p] >= PRIOR[p][0]) & (th[p] <= PRIOR[p][1]) for p in range(2)], axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            log_alpha = np.where(inside, self.log_joint(th, x) - self.log_joint(self.theta, x), -np.inf)
            take = np.log(self.rng.uniform(size=(R,))) < log_alpha
        self.theta = np.where(take[None, :], th, self.theta)
        b.params = tuple(torch.from_numpy(self.theta[p].copy()) for p in range(2))
        b.set_retained(x_d)                                              # the pinned weights under the accepted parameters
        self.j += 1


for R, n, T in [tuple(int(v) for v in s.split(":")) for s in os.environ.get("PG_SHAPES", "1024:8:8,1024:64:8,256:256:25").split(",")]:
    ys = torch.from_numpy(workloads.lgssm_data(T))
    rng = np.random.default_rng(R)
    theta0 = np.stack([rng.uniform(lo + 0.05, hi - 0.05, size=(R,)) for lo, hi in PRIOR]).astype(np.float32)
    budget = 8 + (args.reps + 3) * args.window
    pg = smc.ParticleGibbs(init, step, prior, n, R, T, ("a", "sy"), STEP_SIZE)
    pg.prepare(G.key(2718), ys, tuple(torch.from_numpy(v.copy()) for v in theta0), budget)
    pg.run(1)
    pg.capture()
    host = HostPG(R, n, T, ys, theta0, G.key(2718))
    sweep = SweepOnly(R, n, T, ys, theta0, G.key(2718))
    forms = {"pg": lambda: pg.run(1), "host": host.iterate, "sweep_only": sweep.iterate}
    for f in forms.values():                            # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in forms}
    for _ in range(args.reps):                          # alternated: every form sees the same neighbours on the machine
        for name, f in forms.items():
            ts[name].append(timed(f, args.window))
    assert pg.done == 4 + args.reps * args.window and pg.bank.graph is not None and host.bank.graph is not None
    med = {name: statistics.median(v) for name, v in ts.items()}
    emit(dict(common, tool="time_pgibbs", what="iteration", R=R, n=n, T=T,
              us_per_iteration={name: {"median": 1e6 * med[name], "min": 1e6 * min(v), "max": 1e6 * max(v)} for name, v in ts.items()},
              spread_over_median={name: (max(v) - min(v)) / med[name] for name, v in ts.items()},
              pg_over_host=med["pg"] / med["host"], pg_over_sweep_only=med["pg"] / med["sweep_only"],
              move_share_of_pg=(med["pg"] - med["sweep_only"]) / med["pg"]))
    del pg, host, sweep, forms
