"""What pinning a slot costs, and what sampling its ancestor costs.  JSON lines, appended to --out:

  pinned_rows   (rows, n) in {(1024, 256), (256, 1024), (64, 4096)}, D in {1, 3}: gmx_resample_rows_pinned against
                gmx_resample_rows(GMX_RESAMPLE_MULTINOMIAL) on the same weights, alternated: the median and the min / max
                of --reps windows after a warm-up.  With --parent-lib the unpinned call is ALSO timed from that library (a
                build of the commit before the pinned entry point existed): the kernel as it was.  The pinned call's
                unpinned slots are asserted equal to the unpinned call's on the pinned weights.
  sweep         ConditionalBank(R = 1024, n = 256, T = 100) on the LGSSM with a retained path, captured, against the
                captured BootstrapBank(resample="multinomial") of the same shape (which records no history), and against
                the ConditionalBank with nothing retained (which does)
  ancestors     (R, n) in {(4096, 256), (64, 16384)}, T = 100, LGSSM with a retained path, three captured sweeps alternated
                in one process: the plain conditional sweep; ConditionalBank(ancestor_sampling=True), whose resampling is
                gmx_resample_rows_as; and the same sweep with that call COMPOSED from gmx_rows_pin + gmx_resample_rows +
                gmx_pick_rows + an index copy (a subclass here).  The two ancestor forms are asserted equal, record for
                record.  `spread_over_median`: (max - min) / median of each form's windows, the run-to-run spread the
                fused / composed ratio is read against.

  backward      (--backward: this section alone) (R, n, T) in {(2048, 8, 32), (64, 1024, 32), (16, 4096, 32)}, LGSSM, a
                conditional sweep with a retained path, then three forms of ONE draw alternated: draw(key), the walk through
                the recorded ancestors; draw(key, backward=True), per step the logits program and gmx_pick_rows_take; and the
                backward draw COMPOSED from the entry points the library had before — gmx_rows_pin's broadcast, the program,
                gmx_pick_rows, an index add and two index-selects per step.  The two backward forms are asserted equal in
                paths, states and weights.  Each figure is per draw, its final synchronisation included.

Clocks as found; a host clock around work that ends in a device synchronise.  Environment: SHAPES ("rows:n,..."), BR, BN,
BT, AS_SHAPES ("R:n,..."), AT, BW_SHAPES ("R:n:T,...").  Needs the MI355X: there is no CPU path."""
import argparse
import ctypes
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
from genjax_amd.inference import smc
from genjax_amd.random import split

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
ap.add_argument("--skip-sweep", action="store_true")
ap.add_argument("--skip-kernel", action="store_true")
ap.add_argument("--skip-ancestors", action="store_true")
ap.add_argument("--backward", action="store_true", help="time draw(key, backward=True) and nothing else")
ap.add_argument("--parent-lib", default="", help="a build of the library without the pinned entry point")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_time_conditional.jsonl"))
args = ap.parse_args()
if args.backward:
    args.skip_kernel = args.skip_sweep = args.skip_ancestors = True
assert torch.cuda.is_available(), "tools/time_conditional.py measures on the GPU only"
be = _lib.get()
dev = be.device
common = {"label": args.label, "reps": args.reps, "device": torch.cuda.get_device_name(0),
          "library": os.path.basename(_lib.LIB_PATH)}
parent = None
if args.parent_lib:
    parent = ctypes.CDLL(args.parent_lib)
    parent.gmx_resample_rows.argtypes = be.c.gmx_resample_rows.argtypes
    assert not hasattr(parent, "gmx_resample_rows_pinned"), "--parent-lib has the pinned entry point: not the parent's build"


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
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", "1024:256,256:1024,64:4096").split(",")]
if args.skip_kernel:
    shapes = []
kind = smc.MULTINOMIAL
for rows, n in shapes:
    for D in (1, 3):
        gen = torch.Generator(device="cuda").manual_seed(11)
        lw = torch.randn((rows, n), device=dev, generator=gen) * 3.0
        pin_lw = torch.randn((rows,), device=dev, generator=gen)
        pin_x = torch.randn((D, rows), device=dev, generator=gen)
        x = torch.zeros((D, rows * n), device=dev)
        keys_d = split(G.key(7), rows).data()
        anc_p, anc_u, anc_o = (torch.empty((rows, n), dtype=torch.int32, device=dev) for _ in range(3))
        mx = torch.empty((rows,), dtype=torch.float32, device=dev)
        tot = torch.empty((rows,), dtype=torch.int64, device=dev)
        status = torch.zeros((1,), dtype=torch.int64, device=dev)
        ws = torch.empty(((be.c.gmx_resample_rows_workspace(kind, rows, n) + 7) // 8,), dtype=torch.int64, device=dev)
        P, st = be.ptr, be.stream()

        def pinned():
            be.check(be.c.gmx_resample_rows_pinned(P(keys_d), P(lw), rows, n, n, n, P(pin_lw), P(pin_x), P(x), D, rows * n, n,
                                                   P(mx), P(tot), P(anc_p), P(status), P(ws), st), "gmx_resample_rows_pinned")

        def plain():
            be.check(be.c.gmx_resample_rows(kind, P(keys_d), P(lw), rows, n, n, n, P(mx), P(tot), P(anc_u), P(status), P(ws), st),
                     "gmx_resample_rows")

        def plain_parent():
            rc = parent.gmx_resample_rows(kind, P(keys_d), P(lw), rows, n, n, n, P(mx), P(tot), P(anc_o), P(status), P(ws), st)
            assert rc == 0, "the parent library refused the call"

        forms = {"pinned": pinned, "plain": plain}
        if parent is not None:
            forms["plain_parent"] = plain_parent
        for f in forms.values():                    # (the pinned call first: the others then see the pinned weights)
            f()
        torch.cuda.synchronize()
        assert torch.equal(anc_p[:, :n - 1], anc_u[:, :n - 1]), "the unpinned slots differ from the unconditional draw"
        assert parent is None or torch.equal(anc_u, anc_o), "this build's and the parent's gmx_resample_rows disagree"
        assert int(status.item()) == 0
        per_window = max(10, min(2000, int(0.05 / max(timed(pinned, 10), 1e-7))))       # ~50 ms of calls per window
        ts = {name: [] for name in forms}
        for _ in range(args.reps):                  # alternated: every form sees the same neighbours on the machine
            for name, f in forms.items():
                ts[name].append(timed(f, per_window))
        med = {name: statistics.median(v) for name, v in ts.items()}
        emit(dict(common, tool="time_conditional", what="pinned_rows", rows=rows, n=n, D=D, calls_per_window=per_window,
                  launches_pinned=1 if n <= 1024 else 4, launches_plain=1 if n <= 1024 else 3,
                  us={name: spread(v, 1e6) for name, v in ts.items()},
                  pinned_over_plain=med["pinned"] / med["plain"],
                  pinned_over_plain_parent=(med["pinned"] / med["plain_parent"]) if parent is not None else None,
                  unpinned_slots_equal=True))
        del lw, x, anc_p, anc_u, anc_o

# ---- (b) the sweep ----------------------------------------------------------------------------------------------------------
if not args.skip_sweep:
    R, n, T = int(os.environ.get("BR", 1024)), int(os.environ.get("BN", 256)), int(os.environ.get("BT", 100))
    init, step = workloads.make_lgssm(G)
    ys = torch.from_numpy(workloads.lgssm_data(T))
    keys = split(G.key(314159), R)
    bank = smc.BootstrapBank(init, step, n, R, T, resample="multinomial").prepare(keys, ys).capture()
    free = smc.ConditionalBank(init, step, n, R, T).prepare(keys, ys).capture()
    cond = smc.ConditionalBank(init, step, n, R, T).prepare(keys, ys)
    cond.launch()
    cond.draw(G.key(1))
    cond.retain()
    cond.capture()
    forms = {"bootstrap_bank": bank.launch, "conditional_nothing_retained": free.launch, "conditional": cond.launch}
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    assert (bank.log_ml() == free.log_ml()).all(), "nothing retained: the bank and the conditional bank disagree"
    ts = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            ts[name].append(timed(f, 3))
    med = {name: statistics.median(v) for name, v in ts.items()}
    emit(dict(common, tool="time_conditional", what="sweep", R=R, n=n, T=T, ms={name: spread(v) for name, v in ts.items()},
              us_per_step={name: 1e6 * m / T for name, m in med.items()},
              conditional_over_bank=med["conditional"] / med["bootstrap_bank"],
              conditional_over_nothing_retained=med["conditional"] / med["conditional_nothing_retained"],
              note="the bootstrap bank records no history; both conditional forms add one gmx_history_record per step",
              history_bytes=T * (cond.D + 2) * R * n * 4))

# ---- (c) ancestor sampling: the fused entry point against its composition ---------------------------------------------------------


class ComposedAncestorBank(smc.ConditionalBank):
    """ancestor_sampling=True with gmx_resample_rows_as replaced by its definition, call for call"""

    def prepare(self, keys, ys, retained=None):
        super().prepare(keys, ys, retained)
        self.as_tmp = torch.zeros((self.R,), dtype=torch.int32, device=self.lw.device)
        self.as_offs = (torch.arange(self.R, dtype=torch.int32, device=self.lw.device) * self.n).contiguous()
        self.as_status = torch.zeros((1,), dtype=torch.int64, device=self.lw.device)
        return self

    def _resample_ancestors(self, t):
        R, n, D = self.R, self.n, self.D
        x = self.store.rows[t % 2]
        P, st = be.ptr, be.stream()
        be.check(be.c.gmx_rows_pin(P(self.lw), R, n, n, P(self.ref_lw[t]), P(self.ref_x[t]), P(x), D, int(x.shape[1]), n,
                                   P(self.ref_x[t + 1]), P(self.next_x), R * n, st), "gmx_rows_pin")
        self._ancestor_logits(t)
        be.check(be.c.gmx_resample_rows(smc.MULTINOMIAL, P(self.step_keys[t][1]), P(self.lw), R, n, n, n, P(self.maxs[t]),
                                        P(self.totals[t]), P(self.anc), P(self.status), P(self.ws), st), "gmx_resample_rows")
        be.check(be.c.gmx_pick_rows(P(self.keys_as[t]), P(self.as_lw), R, n, n, P(self.as_tmp), P(self.as_status),
                                    P(self.pick_ws), st), "gmx_pick_rows")
        torch.add(self.as_tmp, self.as_offs, out=self.anc[:, n - 1])


if not args.skip_ancestors:
    T = int(os.environ.get("AT", 100))
    init, step = workloads.make_lgssm(G)
    ys = torch.from_numpy(workloads.lgssm_data(T))
    for R, n in [tuple(int(v) for v in s.split(":")) for s in os.environ.get("AS_SHAPES", "4096:256,64:16384").split(",")]:
        keys = split(G.key(314159), R)
        seed = smc.ConditionalBank(init, step, n, R, T).prepare(keys, ys)
        seed.launch()
        path = seed.draw(G.key(1)).clone()
        del seed
        banks = {"conditional": smc.ConditionalBank(init, step, n, R, T),
                 "ancestors_fused": smc.ConditionalBank(init, step, n, R, T, ancestor_sampling=True),
                 "ancestors_composed": ComposedAncestorBank(init, step, n, R, T, ancestor_sampling=True)}
        for b in banks.values():
            b.prepare(keys, ys, retained=path).capture()
        forms = {name: b.launch for name, b in banks.items()}
        for _ in range(3):                          # warm-up
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        fu, co, pl = banks["ancestors_fused"], banks["ancestors_composed"], banks["conditional"]
        assert torch.equal(fu.hist_ancs, co.hist_ancs) and torch.equal(fu.hist_xs, co.hist_xs), "fused and composed disagree"
        assert torch.equal(fu.hist_xs, pl.hist_xs) and torch.equal(fu.hist_lws, pl.hist_lws), "ancestor sampling moved a particle"
        moved = int((fu.hist_ancs != pl.hist_ancs).sum().item())
        assert fu.status.tolist() == [0, 0]
        ts = {name: [] for name in forms}
        for _ in range(args.reps):                  # alternated: every form sees the same neighbours on the machine
            for name, f in forms.items():
                ts[name].append(timed(f, 3))
        med = {name: statistics.median(v) for name, v in ts.items()}
        emit(dict(common, tool="time_conditional", what="ancestors", R=R, n=n, T=T, ms={name: spread(v) for name, v in ts.items()},
                  us_per_step={name: 1e6 * m / T for name, m in med.items()},
                  spread_over_median={name: (max(v) - min(v)) / med[name] for name, v in ts.items()},
                  fused_over_composed=med["ancestors_fused"] / med["ancestors_composed"],
                  fused_over_conditional=med["ancestors_fused"] / med["conditional"],
                  launches_per_ancestor_step={"conditional": 3 if n <= 1024 else 6, "ancestors_fused": 5 if n <= 1024 else 9,
                                              "ancestors_composed": 8 if n <= 1024 else 10},
                  pinned_ancestors_moved=moved, fused_equals_composed=True))
        del banks, forms, fu, co, pl

# ---- (d) backward simulation: the fused pick against its composition ---------------------------------------------------------------


def composed_backward_draw(cb, key, bufs):
    """draw(key, backward=True) without gmx_pick_rows_take: per step gmx_rows_pin's broadcast of the chosen state (its
    pins go to scratch), the logits program, gmx_pick_rows, an index add and two index-selects"""
    R, n, T, D = cb.R, cb.n, cb.T, cb.D
    N = R * n
    P, st = be.ptr, be.stream()
    bufs["keys"].copy_(torch.from_numpy(cb._backward_keys(key)))
    status = bufs["status"]
    status.zero_()
    paths = torch.empty((T, R), dtype=torch.int32, device=dev)
    lw_path = torch.empty((T, R), dtype=torch.float32, device=dev)
    traj = torch.empty((T, D, R), dtype=torch.float32, device=dev)
    for t in range(T - 1, -1, -1):
        lw_t = cb.hist_lws[t]
        logits = lw_t
        if t < T - 1:
            be.check(be.c.gmx_rows_pin(P(bufs["pin_lw"]), R, n, n, P(bufs["zeros"]), P(traj[t + 1]), P(bufs["pin_x"]), D, N, n,
                                       P(traj[t + 1]), P(bufs["next"]), N, st), "gmx_rows_pin")
            x_t = cb._views._state_view(cb.hist_xs[t:t + 1], 0)
            x_t = type(x_t)(v[0] for v in x_t) if cb.tuple_state is not None else x_t[0]
            smc._ancestor_logits(cb.step, bufs["sites"], cb.obs_addr, x_t, tuple(cb.step_extra(t + 1)) + cb.tail,
                                 list(bufs["next"]), cb.ys[t + 1], lw_t, bufs["logits"].reshape(1, N), specialize=cb.specialize)
            logits = bufs["logits"]
        be.check(be.c.gmx_pick_rows(P(bufs["keys"][t]), P(logits), R, n, n, P(bufs["k"]), P(status[t:]), P(cb.pick_ws), st),
                 "gmx_pick_rows")
        torch.add(bufs["k"], bufs["offs"], out=paths[t])
        flat = paths[t].long()
        torch.index_select(cb.hist_xs[t], 1, flat, out=traj[t])
        torch.index_select(lw_t, 0, flat, out=lw_path[t])
    assert not any(status.tolist())
    return traj, lw_path, paths


if args.backward:
    import hashlib
    with open(_lib.LIB_PATH, "rb") as fh:
        lib_hash = hashlib.sha256(fh.read()).hexdigest()
    init, step = workloads.make_lgssm(G)
    for R, n, T in [tuple(int(v) for v in s.split(":")) for s in
                    os.environ.get("BW_SHAPES", "2048:8:32,64:1024:32,16:4096:32").split(",")]:
        ys = torch.from_numpy(workloads.lgssm_data(T))
        cb = smc.ConditionalBank(init, step, n, R, T).prepare(split(G.key(314159), R), ys)
        cb.launch()
        cb.draw(G.key(1))
        cb.retain()
        cb.launch()
        D, N = cb.D, R * n
        bufs = dict(sites=(cb.state_addr,), keys=torch.zeros((T, R, 2), dtype=torch.int32, device=dev),
                    status=torch.zeros((T,), dtype=torch.int64, device=dev), k=torch.zeros((R,), dtype=torch.int32, device=dev),
                    offs=(torch.arange(R, dtype=torch.int32, device=dev) * n).contiguous(),
                    next=torch.zeros((D, N), dtype=torch.float32, device=dev), logits=torch.zeros((N,), dtype=torch.float32, device=dev),
                    pin_lw=torch.zeros((N,), dtype=torch.float32, device=dev), pin_x=torch.zeros((D, N), dtype=torch.float32, device=dev),
                    zeros=torch.zeros((R,), dtype=torch.float32, device=dev))
        key = G.key(2)
        forms = {"lineage": lambda: cb.draw(key), "backward_fused": lambda: cb.draw(key, backward=True),
                 "backward_composed": lambda: composed_backward_draw(cb, key, bufs)}
        for _ in range(3):                          # warm-up (the logits program is built and specialised here)
            for f in forms.values():
                f()
        cb.draw(key, backward=True)
        fused = [v.clone() for v in cb._last[:3]]
        comp = composed_backward_draw(cb, key, bufs)
        assert all(torch.equal(a, b) for a, b in zip(fused, comp)), "fused and composed backward draws disagree"
        cb.draw(key)
        moved = int((cb._last[2] != fused[2]).sum().item())
        per_window = max(3, min(400, int(0.2 / max(timed(forms["backward_fused"], 3), 1e-7))))      # ~0.2 s of draws per window
        ts = {name: [] for name in forms}
        for _ in range(args.reps):                  # alternated: every form sees the same neighbours on the machine
            for name, f in forms.items():
                ts[name].append(timed(f, per_window))
        med = {name: statistics.median(v) for name, v in ts.items()}
        emit(dict(common, tool="time_conditional", what="backward", library_sha256=lib_hash, R=R, n=n, T=T,
                  draws_per_window=per_window, ms_per_draw={name: spread(v) for name, v in ts.items()},
                  us_per_step={name: 1e6 * m / T for name, m in med.items()},
                  spread_over_median={name: (max(v) - min(v)) / med[name] for name, v in ts.items()},
                  fused_over_composed=med["backward_fused"] / med["backward_composed"],
                  fused_over_lineage=med["backward_fused"] / med["lineage"],
                  launches_per_backward_step={"backward_fused": 2 if n <= 1024 else 4, "backward_composed": 8},
                  picks_off_the_lineage=moved, fused_equals_composed=True))
        del cb, bufs, forms
