"""What the marginal smoother costs beside backward simulation.  One JSON line per (model, n), appended to --out:

  SweepHistory.marginal_smooth() against SweepHistory.backward_sample(key, m = n) of the same history — the same n^2 transition
  densities a step, summed instead of sampled — alternated: the median and the min / max of --reps runs after a warm-up.  The
  smoother's own parts are timed apart, each as a window of one step's calls: the gmx_smooth_back calls alone on a filled slab
  (the kernel's share, with its rate in float64 multiply-adds and in bytes of logits), and the density launches alone.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: T (steps, default 9), NS (sizes,
default "1024,4096").  Needs the MI355X: there is no CPU path."""
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
from genjax_amd import numpy as jnp
from genjax_amd.inference import smc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_smooth.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_smooth.py measures on the GPU only"
be = _lib.get()
dev = be.device
T = int(os.environ.get("T", 9))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ms(ts):
    return {"median": 1e3 * statistics.median(ts), "min": 1e3 * min(ts), "max": 1e3 * max(ts)}


def tracker():
    @G.gen
    def init():
        p = G.normal(0.0, 1.0) @ "p"
        v = G.normal(0.0, 0.5) @ "v"
        G.normal(p, 0.3) @ "y"
        return jnp.stack([p, v])

    @G.gen
    def step(s):
        p = G.normal(s[..., 0] + 0.1 * s[..., 1], 0.05) @ "p"
        v = G.normal(s[..., 1], 0.1) @ "v"
        G.normal(p, 0.3) @ "y"
        return jnp.stack([p, v])
    return init, step


for model in ("lgssm", "tracker"):
    for n in (int(v) for v in os.environ.get("NS", "1024,4096").split(",")):
        if model == "lgssm":
            (init, step), ys, sites = workloads.make_lgssm(G), workloads.lgssm_data(T), None
        else:
            (init, step), ys, sites = tracker(), np.random.default_rng(31).normal(size=T).astype(np.float32), ("p", "v")
        sw = smc.BootstrapSweep(init, step, n, T, history=True).prepare(G.key(314159), torch.from_numpy(ys))
        sw.launch()
        h = sw.history()
        D, C = h.D, 1 + h.D
        smooth = lambda: h.marginal_smooth(state_sites=sites)
        sample = lambda: h.backward_sample(G.key(99), n, state_sites=sites)
        # one step's parts on their own: the slab filled as the method fills it, then the contraction
        R = max(1, min(smc.BACKWARD_ROWS_MAX, n, 40 // D))
        slab = torch.empty((n, n), dtype=torch.float32, device=dev)
        u = torch.rand((C, n), dtype=torch.float64, device=dev)
        out = torch.empty((C, n), dtype=torch.float64, device=dev)
        status = torch.zeros((1,), dtype=torch.int64, device=dev)
        ws = smc._workspace(be.c.gmx_smooth_back_workspace(n, n, C), dev)

        def fill():
            for r0 in range(0, n, R):
                smc._backward_logits(h._step, sites or (h._state_addr,), h._obs_addr, h._step_state(0), (),
                                     [h._xs[1, d, r0:r0 + R] for d in range(D)], h._ys[1], h.log_weights[0], slab[r0:r0 + R],
                                     who="tools/time_smooth.py")

        def contract():
            for _ in range(10):
                smc.smooth_back(slab, u, out, status=status, workspace=ws)
        smooth(), sample(), fill(), contract()                   # warm: traces the density programs, loads the code objects
        t_smooth, t_sample, t_fill, t_kernel = [], [], [], []
        for _ in range(args.reps):                               # alternated: every form sees the same neighbours on the machine
            t_smooth.append(timed(smooth))
            t_sample.append(timed(sample))
            t_fill.append(timed(fill))
            t_kernel.append(timed(contract) / 10)
        k = statistics.median(t_kernel)
        rec = dict(tool="time_smooth", label=args.label, reps=args.reps, device=torch.cuda.get_device_name(0),
                   library=os.path.basename(_lib.LIB_PATH), model=model, n=n, T=T, D=D, rows_per_density_launch=R,
                   marginal_smooth_ms=ms(t_smooth), backward_sample_m_eq_n_ms=ms(t_sample),
                   smooth_over_sample=statistics.median(t_smooth) / statistics.median(t_sample),
                   per_step_ms={"densities_alone": ms(t_fill), "gmx_smooth_back_alone": ms(t_kernel),
                                "marginal_smooth": 1e3 * statistics.median(t_smooth) / (T - 1)},
                   kernel_share_of_smoother=k * (T - 1) / statistics.median(t_smooth),
                   kernel_rate={"f64_GFMAs_per_s": 16 * n * n / k / 1e9, "useful_f64_GFMAs_per_s": C * n * n / k / 1e9,
                                "logit_GB_per_s_two_passes": 2 * 4 * n * n / k / 1e9, "Gexp_per_s": n * n / k / 1e9})
        line = json.dumps(rec)
        print(line)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
