"""What BootstrapSweep(history=True) costs and what the lineage kernel buys, at config 2's size (n = 1e6, T = 100,
captured graph).  One JSON line:

  us_per_step          history=False and history=True, alternated: median over --reps windows of --launches replays each
  record               the difference per step, and the rate of the 8 D + 16 bytes per particle-step it moves
  record_alone         gmx_history_record on its own (device events, median): its roofline row
  trajectories         SweepHistory.trajectories() for m = n: one gmx_lineage launch (median, with its status read)
  torch_loop           the same trajectories by T steps of index_select on the recorded slabs; outputs asserted equal

Clocks as found; every timed shape is warmed first; a host clock around work that ends in a device synchronise.
Environment: N, T (sizes; the defaults are config 2's).  Needs the MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import genjax_amd as G
from genjax_amd import _lib, workloads
from genjax_amd.inference.smc import BootstrapSweep

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "tools/time_history.py measures on the GPU only"

n, T = int(os.environ.get("N", 1_000_000)), int(os.environ.get("T", 100))
ys = torch.from_numpy(workloads.lgssm_data(T))
init, step = workloads.make_lgssm(G)


def sync():
    torch.cuda.synchronize()


def window(fn, launches):
    sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    sync()
    return (time.perf_counter() - t0) / launches


sweeps = {}
for name, hist in (("plain", False), ("history", True)):
    sw = BootstrapSweep(init, step, n, T, history=hist).prepare(G.key(314159), ys).capture()
    for _ in range(3):
        sw.launch()
    sync()
    sweeps[name] = sw
times = {k: [] for k in sweeps}
for _ in range(args.reps):                      # alternated: both forms see the same neighbours on the machine
    for name, sw in sweeps.items():
        times[name].append(window(sw.launch, args.launches))
us = {k: 1e6 * statistics.median(v) / T for k, v in times.items()}
spread = {k: [1e6 * min(v) / T, 1e6 * max(v) / T] for k, v in times.items()}
sw, plain = sweeps["history"], sweeps["plain"]
assert sw.log_ml() == plain.log_ml()
assert all(torch.equal(a, b) for a, b in zip(sw.state(), plain.state()))
D = sw.hist_xs.shape[1]
step_bytes = (8 * D + 16) * n

# the record on its own: one mid-sweep step's rows into its slab rows, plain ancestors
be = _lib.get()
t_mid = T // 2
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
alone = []
for i in range(5 + 4 * args.reps):
    ev[0].record()
    sw._record(t_mid)
    ev[1].record()
    sync()
    if i >= 5:
        alone.append(ev[0].elapsed_time(ev[1]) * 1e3)
sw.launch()                                     # (the slabs again hold one whole sweep)
sync()

h = sw.history()
h.trajectories()                                # warm
lin = [window(h.trajectories, 1) for _ in range(args.reps)]
traj = h.trajectories()


def walk_in_torch(hist, first, out):
    """the obvious way: T index_selects per slab (into a preallocated [T, m] buffer, the kernel's own layout), an int64
    copy of every ancestor row"""
    p = first.long()
    for t in range(T - 1, -1, -1):
        torch.index_select(hist.x[t], 0, p, out=out[t])
        if t:
            p = torch.index_select(hist.ancestors[t - 1], 0, p).long()
    return out.t()


buf = torch.empty((T, n), dtype=torch.float32, device="cuda")
torch_loop = lambda: walk_in_torch(h, h.ancestors[T - 1], buf)
ref = torch_loop()
assert torch.equal(traj.view(torch.int32), ref.view(torch.int32)), "the lineage kernel and the torch loop disagree"
loop = [window(torch_loop, 1) for _ in range(args.reps)]
distinct = [int(torch.unique(h.lineage()[t]).numel()) for t in (0, T // 2, T - 1)]
del traj, ref

# the walk where nothing coalesces: ancestors uniform at random (a sweep's own lineages merge within a few steps, so most
# of its lanes end up reading the same few cache lines; this is the kernel's worst case)
from genjax_amd.inference.smc import SweepHistory
gen = torch.Generator(device="cuda").manual_seed(7)
h_rand = SweepHistory(torch.randn((T, 1, n), device="cuda", generator=gen), torch.zeros((T, n), device="cuda"),
                      torch.randint(0, n, (T, n), device="cuda", generator=gen, dtype=torch.int32))
start = torch.arange(n, device="cuda", dtype=torch.int32)
traj = h_rand.trajectories(start)
torch_loop_rand = lambda: walk_in_torch(h_rand, start, buf)
ref = torch_loop_rand()
assert torch.equal(traj.view(torch.int32), ref.view(torch.int32)), "random ancestors: kernel and torch loop disagree"
lin_r = [window(lambda: h_rand.trajectories(start), 1) for _ in range(args.reps)]
loop_r = [window(torch_loop_rand, 1) for _ in range(args.reps)]

out = {
    "tool": "time_history", "label": args.label, "n": n, "T": T, "D": int(D), "reps": args.reps,
    "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0),
    "library": os.path.basename(_lib.LIB_PATH),
    "us_per_step": {"history_false": us["plain"], "history_true": us["history"], "min_max": spread},
    "record": {"us_per_step_in_sweep": us["history"] - us["plain"], "bytes_per_step": step_bytes,
               "GBps_in_sweep": step_bytes / max(us["history"] - us["plain"], 1e-9) / 1e3},
    "record_alone": {"us_median": statistics.median(alone), "us_min": min(alone),
                     "GBps_median": step_bytes / statistics.median(alone) / 1e3},
    "trajectories_m_eq_n": {"gmx_lineage_ms": 1e3 * statistics.median(lin), "min_ms": 1e3 * min(lin),
                            "torch_loop_ms": 1e3 * statistics.median(loop), "torch_loop_min_ms": 1e3 * min(loop),
                            "speedup": statistics.median(loop) / statistics.median(lin),
                            "outputs_equal": True, "distinct_ancestors_at_t0_mid_last": distinct},
    "trajectories_random_ancestors": {"gmx_lineage_ms": 1e3 * statistics.median(lin_r), "min_ms": 1e3 * min(lin_r),
                                      "torch_loop_ms": 1e3 * statistics.median(loop_r),
                                      "speedup": statistics.median(loop_r) / statistics.median(lin_r),
                                      "outputs_equal": True},
    "log_ml": sw.log_ml(), "fuse": bool(sw.fuse), "noise_ahead": bool(sw.noise_ahead),
}
print(json.dumps(out))
