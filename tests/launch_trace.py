"""Shared body of tests/test_launch_trace.py and tests/golden/make_launch_trace.py: WHICH C-ABI calls a sweep or a
one-off resampling issues, in which order, with which integers and which buffers — recorded by a proxy put in place of
`backend.c` (after Backend._proto() has set the prototypes) and compared with a record made at an earlier commit
(tests/golden/launch_trace_{cpu,gpu}.json).  The bit-exact tests say that the results are right; this one says that a
change to the Python that launches (inference/smc.py, inference/sharded.py) left the launches themselves alone.

What is recorded for each `gmx_*` call: the name; every integer argument; a `c_uint32 * 2` key as its two words; a
struct (gmx_run_args, gmx_peer) as its non-zero fields.  Pointers: inside a prepared sweep every buffer is persistent,
so a pointer is recorded as the ordinal of its first appearance in that trace ("p0", "p1", ...: which calls share which
buffers, independent of addresses and attribute names); in a one-off call the buffers are fresh allocations and a
pointer is recorded as "ptr" or "null" only."""
from __future__ import annotations

import ctypes
import gc
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {"cpu": os.path.join(HERE, "golden", "launch_trace_cpu.json"),
          "gpu": os.path.join(HERE, "golden", "launch_trace_gpu.json")}
# (the "state/" and "bank/" cases of the mirror were recorded later, at another parent: a file of their own)
LATER = {"cpu": [os.path.join(HERE, "golden", "launch_trace_cpu_state.json")], "gpu": []}
KINDS = ("systematic", "stratified", "multinomial", "multinomial_tiled", "multinomial_sorted")
TILE_KINDS = ("systematic", "stratified", "multinomial_tiled", "multinomial_sorted")


class Recorder:
    """stands in for Backend.c: every attribute is the library's own; `gmx_*` functions are wrapped"""

    def __init__(self, c):
        self._c, self.calls, self.identity, self._ord = c, None, False, {}

    def __getattr__(self, name):
        f = getattr(self._c, name)
        if not name.startswith("gmx_"):
            return f

        def call(*args):
            if self.calls is not None:
                self.calls.append([name] + [self._arg(a) for a in args])
            return f(*args)
        return call

    def start(self, identity):
        self.calls, self.identity, self._ord = [], identity, {}

    def stop(self):
        out, self.calls = self.calls, None
        return out

    def _ptr(self, v):
        if not v:
            return "null"
        if not self.identity:
            return "ptr"
        return "p%d" % self._ord.setdefault(int(v), len(self._ord))

    def _arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, (bool, int, np.integer)):
            return int(a)
        if isinstance(a, float):
            return float(a).hex()
        if isinstance(a, bytes):
            return a.decode()
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return self._trim([self._ptr(v) for v in a], "null")
            if a._type_ is ctypes.c_uint32 and len(a) == 2:
                return {"key": [int(a[0]), int(a[1])]}
            return self._trim([int(v) for v in a], 0)
        if isinstance(a, ctypes.Structure):
            return self._struct(a)
        if hasattr(a, "_obj"):                    # ctypes.byref(struct)
            return self._arg(a._obj)
        if hasattr(a, "value"):                   # c_int32(3), ...
            return self._arg(a.value)
        return "<%s>" % type(a).__name__

    @staticmethod
    def _trim(vals, empty):
        while vals and vals[-1] == empty:
            vals.pop()
        return vals

    def _struct(self, s):
        out = {}
        for field in s._fields_:
            if field[0].startswith("reserved"):
                continue
            v = getattr(s, field[0])
            v = self._ptr(v) if field[1] is ctypes.c_void_p else self._arg(v)
            if v not in (0, "null", [], {}):
                out[field[0]] = v
        return out


def install(be):
    """put a Recorder in place of be.c (idempotent); returns it"""
    if not isinstance(be.c, Recorder):
        be.c = Recorder(be.c)
    return be.c


def uninstall(be):
    if isinstance(be.c, Recorder):
        be.c = be.c._c


def _key(seed):
    import genjax_amd as G
    return G.key(seed)


# --- sweeps ----------------------------------------------------------------------------------------------------------
def _lgssm(n=3000, T=5, **kw):
    def make():
        import genjax_amd as G
        from genjax_amd import workloads
        from genjax_amd.inference.smc import BootstrapSweep
        init, step = workloads.make_lgssm(G)
        return BootstrapSweep(init, step, n, T, **kw).prepare(_key(2718), torch.from_numpy(workloads.lgssm_data(T)))
    return make


def _nlssm_mh(n=1500, T=5, **kw):
    """the model and the move of tests/parity.check_nlssm_mh_sweep"""
    def make():
        import genjax_amd as G
        from genjax_amd import workloads
        from genjax_amd.inference.smc import BootstrapSweep
        init, step = workloads.make_nlssm(G)
        req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})
        return BootstrapSweep(init, step, n, T, step_extra=lambda t: (float(t),), rejuvenate=req,
                              **kw).prepare(_key(7), torch.from_numpy(workloads.nlssm_data(T)))
    return make


def _without_program_stats(make):
    """the sweep a device builds from programs that cannot leave the CDF tile statistics (interpreted ones; the mirror's
    always can): the resampler then takes its own pass over the log-weights"""
    def patched():
        from genjax_amd import engine
        old = engine.Compiled.writes_tile_stats
        engine.Compiled.writes_tile_stats = lambda self: False
        try:
            sw = make()
        finally:
            engine.Compiled.writes_tile_stats = old
        assert not sw.tile_stats
        return sw
    return patched


def sweep_cases():
    """name -> a function that builds and prepares the sweep; specialize / noise_ahead / fuse_resample always explicit"""
    cases = {}
    for kind in KINDS:
        for na in (False, True):
            cases[f"lgssm/{kind}/na{int(na)}"] = _lgssm(resample=kind, specialize=True, noise_ahead=na, fuse_resample=False)
    for na in (False, True):
        cases[f"lgssm/systematic/fuse/na{int(na)}"] = _lgssm(specialize=True, noise_ahead=na, fuse_resample=True)
    cases["lgssm/systematic/fuse/na1/history"] = _lgssm(specialize=True, noise_ahead=True, fuse_resample=True, history=True)
    cases["lgssm/systematic/na0/history"] = _lgssm(specialize=True, noise_ahead=False, fuse_resample=False, history=True)
    for kind in KINDS:         # interpreted programs leave no tile statistics: gmx_resample, gmx_tile_stats + the kind's own
        cases[f"lgssm/{kind}/interpreted"] = _lgssm(resample=kind, specialize=False, noise_ahead=False, fuse_resample=False)
    for kind in TILE_KINDS:
        cases[f"lgssm/{kind}/no_program_stats"] = _without_program_stats(
            _lgssm(resample=kind, specialize=False, noise_ahead=False, fuse_resample=False))
    cases["lgssm/systematic/n700"] = _lgssm(n=700, specialize=True, noise_ahead=False, fuse_resample=False)
    cases["lgssm/systematic/n1024"] = _lgssm(n=1024, specialize=True, noise_ahead=False, fuse_resample=False)
    # (n >= MULTINOMIAL_GUIDED_MIN: the iid multinomial through its guide table)
    cases["lgssm/multinomial/n9000"] = _lgssm(n=9000, T=3, resample="multinomial", specialize=True, noise_ahead=False,
                                              fuse_resample=False)
    cases["nlssm_mh/chained"] = _nlssm_mh(specialize=True, noise_ahead=False, fuse_resample=False, chain_mh=True)
    cases["nlssm_mh/two_launches"] = _nlssm_mh(specialize=True, noise_ahead=False, fuse_resample=False, chain_mh=False)
    cases["nlssm_mh/chained/na1"] = _nlssm_mh(specialize=True, noise_ahead=True, fuse_resample=False, chain_mh=True)
    return cases


def _state_sweep(which, n=1500, T=3, **kw):
    """a vector state [n, 2] (history_checks.make_tracker) / a tuple of two scalars (make_pair): D = 2 rows of the store"""
    def make():
        import genjax_amd as G
        from genjax_amd import numpy as jnp
        from genjax_amd.inference.smc import BootstrapSweep
        from tests import history_checks as H
        init, step = H.make_pair(G) if which == "tuple" else H.make_tracker(G, lambda a, b: jnp.stack([a, b]))
        return BootstrapSweep(init, step, n, T, **kw).prepare(_key(17), torch.from_numpy(H.state_data()))
    return make


def state_cases():
    cases = {}
    for which in ("vector", "tuple"):
        for fuse in (False, True):
            cases[f"state/{which}/fuse{int(fuse)}"] = _state_sweep(which, specialize=True, noise_ahead=False, fuse_resample=fuse)
    cases["state/vector/history"] = _state_sweep("vector", specialize=True, noise_ahead=False, fuse_resample=False, history=True)
    cases["state/vector/interpreted"] = _state_sweep("vector", specialize=False, noise_ahead=False, fuse_resample=False)
    return cases


BANK_R, BANK_T = 3, 3


def bank_cases():
    """name -> a function that builds and prepares a BootstrapBank of BANK_R filters"""
    def bank(model, n, **kw):
        def make():
            import genjax_amd as G
            from genjax_amd import numpy as jnp, workloads
            from genjax_amd.inference.smc import BootstrapBank
            from tests import bank_checks as B, history_checks as H
            ys = torch.from_numpy(workloads.lgssm_data(BANK_T))
            if model == "lgssm":
                init, step = workloads.make_lgssm(G)
            elif model == "vector":
                init, step = H.make_tracker(G, lambda a, b: jnp.stack([a, b]))
            elif model == "tuple":
                init, step = H.make_pair(G)
            else:                       # the process-noise scale as a [R] parameter of init and step
                init, step = B.make_lgssm_sx(G, True)
                kw["params"] = (torch.tensor(B.PARAM_SX[:BANK_R], dtype=torch.float32),)
            return BootstrapBank(init, step, n, BANK_R, BANK_T, specialize=True, **kw).prepare(
                G.split(_key(4242), BANK_R), ys)
        return make
    cases = {}
    for kind in ("systematic", "stratified", "multinomial"):
        for n in (200, 1500):
            cases[f"bank/{kind}/n{n}"] = bank("lgssm", n, resample=kind)
    for model in ("vector", "tuple", "params"):
        cases[f"bank/systematic/{model}"] = bank(model, 1500)
    return cases


CAPTURED = ("systematic", "multinomial_tiled")          # (GPU half only: the mirror has no graph capture)


def trace_sweep(be, make):
    """{"enqueue": [...], "skip_vm": [...]} of one prepared sweep, after one untraced enqueue (program upload, first-launch
    checks); `enqueue` is traced twice and must come out the same (a buffer made per launch would show here)"""
    rec = install(be)
    sw = make()
    sw.enqueue()
    out = {}
    for name, kw in (("enqueue", {}), ("enqueue_again", {}), ("skip_vm", {"skip_vm": True})):
        rec.start(identity=True)
        sw.enqueue(**kw)
        out[name] = rec.stop()
    _sync(be)
    assert out["enqueue"] == out.pop("enqueue_again"), "two enqueues of one prepared sweep issued different calls"
    return out


def trace_bank(be, make):
    """{"enqueue": [...]} of one prepared bank, as trace_sweep (a bank has no skip_vm form)"""
    rec = install(be)
    bank = make()
    bank.enqueue()
    out = {}
    for name in ("enqueue", "enqueue_again"):
        rec.start(identity=True)
        bank.enqueue()
        out[name] = rec.stop()
    _sync(be)
    assert out["enqueue"] == out.pop("enqueue_again"), "two enqueues of one prepared bank issued different calls"
    return out


def trace_captured(be, kind):
    """prepare().capture() (the warm-up and the captured enqueue), then two launch()es"""
    rec = install(be)
    sw = _lgssm(resample=kind, specialize=True, noise_ahead=True, fuse_resample=False)()
    rec.start(identity=True)
    sw.capture()
    sw.launch()
    sw.launch()
    out = rec.stop()
    _sync(be)
    sw.log_ml()
    return {"capture_launch_launch": out}


def trace_sharded(be):
    """ShardedBootstrapSweep at world size 1, collectives issued (the fused peer exchange, as tests/parity.check_sweep_verdict)"""
    import genjax_amd as G
    from genjax_amd import workloads
    from genjax_amd.inference.sharded import ShardedBootstrapSweep

    class _Solo:
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def get_world_size(): return 1
    rec = install(be)
    old = os.environ.get("GENMI_COMM")
    os.environ["GENMI_COMM"] = "peer"
    try:
        n, T = 3072, 5
        init, step = workloads.make_lgssm(G)
        sw = ShardedBootstrapSweep(init, step, n, T, _Solo, always_communicate=True, specialize=True,
                                   noise_ahead=be.uses_streams).prepare(_key(3), torch.from_numpy(workloads.lgssm_data(T)))
        sw.launch()
        sw.finish()
        rec.start(identity=True)
        sw.launch()
        sw.finish()
        out = rec.stop()
        assert sw.reruns == 0
        sw.close()
    finally:
        if old is None:
            os.environ.pop("GENMI_COMM", None)
        else:
            os.environ["GENMI_COMM"] = old
    return {"launch_finish": out}


class _Solo:
    @staticmethod
    def get_rank(): return 0
    @staticmethod
    def get_world_size(): return 1


class _comm_env:
    """GENMI_COMM for the duration of a case ("none": unset)"""

    def __init__(self, comm):
        self.comm = comm

    def __enter__(self):
        self.old = os.environ.pop("GENMI_COMM", None)
        if self.comm != "none":
            os.environ["GENMI_COMM"] = self.comm

    def __exit__(self, *exc):
        os.environ.pop("GENMI_COMM", None)
        if self.old is not None:
            os.environ["GENMI_COMM"] = self.old


SHARD_N, SHARD_T = 3072, 4            # three tiles (a table of more than one row, an odd count: the padding); init, the
                                      # first MH step and the steady state


def _sharded_model(model):
    """(init, step, constructor keywords, observations, seed) of the sharded cases' models"""
    import genjax_amd as G
    from genjax_amd import numpy as jnp, workloads
    from tests import parity
    T = SHARD_T
    if model == "lgssm":
        return workloads.make_lgssm(G) + ({}, workloads.lgssm_data(T), 3)
    if model == "nlssm_mh":          # config 3: two routed leaves
        req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.5))})
        return workloads.make_nlssm(G) + (dict(rejuvenate=req, step_extra=lambda t: (float(t),)), workloads.nlssm_data(T), 7)
    if model == "tracker":           # a vector state, D = 2: one routed leaf per component
        return parity.make_tracker(G, lambda a, b: jnp.stack([a, b])) + ({}, parity.tracker_data(T), 5)
    if model == "vec_mh":            # D = 2 and an MH move: 2 * D leaves
        req = G.StaticRequest({"x": G.Rejuvenate(G.normal, lambda chm: (chm.get_value(), 0.2))})
        return parity.make_vec_mh(G, lambda *v: jnp.stack(list(v)), jnp.ones(2)) + (
            dict(rejuvenate=req, step_extra=lambda t: (float(t),)), parity.tracker_data(T), 11)
    raise KeyError(model)


def sharded_cases(backend):
    """name -> (model, GENMI_COMM or "none", ShardedBootstrapSweep keywords, captured); world size 1, the collectives
    issued whenever a communicator is named.  The mirror never specialises or fuses the sharded step, so the one-launch
    step and the chained MH form are in the device's list only — which is short (the GPU suite's time budget)."""
    cases = {}
    if backend == "gpu":
        cases["sharded/lgssm/peer/default"] = ("lgssm", "peer", {}, False)
        cases["sharded/lgssm/peer/fuse_step0"] = ("lgssm", "peer", {"fuse_step": False}, False)
        cases["sharded/nlssm_mh/peer/default"] = ("nlssm_mh", "peer", {}, False)
        cases["sharded/lgssm/p2p/default"] = ("lgssm", "p2p", {}, False)
        cases["sharded/nlssm_mh/p2p/default"] = ("nlssm_mh", "p2p", {}, False)
        cases["sharded/lgssm/none/cdf_form"] = ("lgssm", "none", {"cdf_form": True}, False)
        cases["sharded/lgssm/none/multinomial_sorted"] = ("lgssm", "none", {"resample": "multinomial_sorted"}, False)
        cases["sharded/tracker/none/default"] = ("tracker", "none", {}, False)
        cases["sharded/lgssm/peer/captured"] = ("lgssm", "peer", {}, True)
        return cases
    variants = {"default": {}, "cdf_form": {"cdf_form": True}, "unfused": {"fused": False},
                "stratified": {"resample": "stratified"}, "multinomial_sorted": {"resample": "multinomial_sorted"},
                "na1": {"noise_ahead": True}}
    for comm in ("none", "p2p", "peer"):
        for v, kw in variants.items():
            cases[f"sharded/lgssm/{comm}/{v}"] = ("lgssm", comm, {"noise_ahead": False, **kw}, False)
    for comm, kw in (("none", {}), ("peer", {}), ("none", {"cdf_form": True}), ("p2p", {"cdf_form": True})):
        cases[f"sharded/nlssm_mh/{comm}/{'cdf_form' if kw else 'default'}"] = ("nlssm_mh", comm, {"noise_ahead": False, **kw}, False)
    for comm in ("none", "p2p", "peer"):
        cases[f"sharded/tracker/{comm}/default"] = ("tracker", comm, {"noise_ahead": False}, False)
    cases["sharded/vec_mh/none/default"] = ("vec_mh", "none", {"noise_ahead": False}, False)
    return cases


def trace_sharded_case(be, model, comm, kw, captured):
    """{"form": which exchange form prepare() chose, "launch_finish": [...]} after one untraced run (captured:
    "capture_launch_launch", as trace_captured)"""
    from genjax_amd.inference.sharded import ShardedBootstrapSweep
    rec = install(be)
    with _comm_env(comm):
        init, step, mkw, ys, seed = _sharded_model(model)
        sw = ShardedBootstrapSweep(init, step, SHARD_N, SHARD_T, _Solo, always_communicate=comm != "none", specialize=True,
                                   **mkw, **kw).prepare(_key(seed), torch.from_numpy(ys))
        form = {k: getattr(sw, k) for k in ("tiles_mode", "peer_mode", "fuse_sh", "chain_mh", "noise_ahead", "capacity")}
        sw.launch()
        sw.finish()
        rec.start(identity=True)
        if captured:
            sw.capture()
            sw.launch()
            sw.launch()
        else:
            sw.launch()
        sw.finish()
        out = rec.stop()
        assert sw.reruns == 0
        sw.close()
    return {"form": form, "capture_launch_launch" if captured else "launch_finish": out}


IMPORTANCE_CASES = {"sharded_importance/default": {}, "sharded_importance/cdf_form": {"cdf_form": True},
                    "sharded_importance/multinomial_sorted": {"kind": "multinomial_sorted"}}


def trace_sharded_importance(be, kw):
    """sharded_importance_resample on the 8-schools target of tests/dist_worker.py, 3072 particles on the one rank"""
    import genjax_amd as G
    from genjax_amd import ChoiceMapBuilder as C, numpy as jnp
    from genjax_amd.inference.sharded import sharded_importance_resample
    from tests import parity

    @G.gen
    def schools():
        mu = G.normal(0.0, 5.0) @ "mu"
        log_tau = G.normal(0.0, 1.0) @ "log_tau"
        theta = G.normal(mu * jnp.ones(8), jnp.exp(log_tau) * jnp.ones(8)) @ "theta"
        _ = G.normal(theta, jnp.array(parity.SCHOOL_SIGMA)) @ "y"
        return theta
    target = G.Target(schools, (), C["y"].set(parity.SCHOOL_Y))
    rec = install(be)
    with _comm_env("none"):
        sharded_importance_resample(target, SHARD_N, _key(2), _Solo, **kw)
        info = {}
        rec.start(identity=False)
        sharded_importance_resample(target, SHARD_N, _key(2), _Solo, stats=info, **kw)
        out = rec.stop()
    _sync(be)
    # (a one-off sizes its workspaces between its launches — a prepared sweep does in prepare(), outside the record;
    #  the size queries launch nothing and are left out: WHERE a buffer is sized is not what this record pins)
    out = [c for c in out if not c[0].endswith(("_workspace", "_words", "_bytes"))]
    return {"form": info["form"], "calls": out}


def _sync(be):
    if be.uses_streams:
        torch.cuda.synchronize()


# --- one-off calls ---------------------------------------------------------------------------------------------------
def _weights(be, n, seed=5):
    lw = (np.random.default_rng(seed).normal(size=n) * 1.5).astype(np.float32)
    return torch.from_numpy(lw).to(be.device)


def _with_stats(be, lw):
    """leave on `lw` what a site program leaves (static.run_gfi): (tile maxima, tile sums, shift, n, version)"""
    from genjax_amd.inference import smc
    n = lw.numel()
    tiles, shift = (n + 1023) // 1024, smc.cdf_shift(n)
    tmax = torch.empty((tiles,), dtype=torch.float32, device=lw.device)
    tagg = torch.empty((tiles,), dtype=torch.int64, device=lw.device)
    be.check(be.c.gmx_tile_stats(be.ptr(lw), n, shift, be.ptr(tmax), be.ptr(tagg), be.stream()), "gmx_tile_stats")
    lw._gmx_tile_stats = (tmax, tagg, shift, n, lw._version)
    return lw


def _collection(lw):
    from genjax_amd.inference.smc import ParticleCollection
    from genjax_amd.static import DistributionTrace
    return ParticleCollection(DistributionTrace(None, (), lw.clone(), lw.clone()), lw)


def trace_one_offs(be, n=3000):
    from genjax_amd.inference import smc
    rec = install(be)
    out = {}

    def traced(name, fn):
        rec.start(identity=False)
        fn()
        out[name] = rec.stop()
        _sync(be)
    for kind in TILE_KINDS:
        kid = smc._KINDS[kind]
        lw = _with_stats(be, _weights(be, n))
        traced(f"resample_fused/{kind}/stats", lambda: smc.resample_fused(kid, _key(11), lw))
        lw.add_(0.25)                                   # in place: the statistics on the tensor are stale now
        traced(f"resample_fused/{kind}/stale", lambda: smc.resample_fused(kid, _key(11), lw))
    for kind in KINDS:
        coll = _collection(_weights(be, n))
        traced(f"resample/{kind}", lambda: smc.resample(_key(12), coll, kind))
    coll = _collection(_weights(be, n))
    traced("resample/multinomial/n_out100", lambda: smc.resample(_key(12), coll, "multinomial", n_out=100))
    coll = _collection(_weights(be, 9000))
    traced("resample/multinomial/n9000", lambda: smc.resample(_key(12), coll, "multinomial"))
    big = _weights(be, 2 ** 21 + 1)                     # the smallest size past RS_MAX_TILES tiles: the prefix form
    for kind in ("systematic", "multinomial_sorted"):
        traced(f"resample_fused/{kind}/prefix", lambda: smc.resample_fused(smc._KINDS[kind], _key(13), big))
    return out


# --- the whole record ------------------------------------------------------------------------------------------------
def case_names(backend):
    names = list(sweep_cases()) + ["sharded", "one_offs"]
    if backend == "gpu":
        names += [f"captured/{k}" for k in CAPTURED]
    names += list(sharded_cases(backend)) + (list(IMPORTANCE_CASES) if backend == "cpu" else [])
    return names + list(state_cases()) + list(bank_cases())


def trace_case(be, name):
    gc.collect()                   # programs of earlier sweeps are destroyed (gmx_program_destroy) now, not whenever the
    gc.disable()                   # collector happens to run inside a record
    try:
        if name == "sharded":
            return trace_sharded(be)
        if name.startswith("sharded/"):
            return trace_sharded_case(be, *sharded_cases("gpu" if be.uses_streams else "cpu")[name])
        if name in IMPORTANCE_CASES:
            return trace_sharded_importance(be, IMPORTANCE_CASES[name])
        if name == "one_offs":
            return trace_one_offs(be)
        if name.startswith("captured/"):
            return trace_captured(be, name.split("/", 1)[1])
        if name.startswith("bank/"):
            return trace_bank(be, bank_cases()[name])
        if name.startswith("state/"):
            return trace_sweep(be, state_cases()[name])
        return trace_sweep(be, sweep_cases()[name])
    finally:
        gc.enable()
        uninstall(be)


def load_golden(backend):
    with open(GOLDEN[backend]) as fh:
        record = json.load(fh)
    for path in LATER[backend]:
        with open(path) as fh:
            record["cases"].update(json.load(fh)["cases"])
    return record


def check_case(be, backend, name):
    """the case's record equals the committed one, call for call"""
    want = load_golden(backend)["cases"][name]
    got = json.loads(json.dumps(trace_case(be, name)))
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    if "form" in want:           # a silent change of form is a failure with a name, not a diff of calls
        assert got["form"] == want["form"], f"{name}: form {got['form']}, recorded at the parent: {want['form']}"
    for part in want:
        if part == "form":
            continue
        a, b = got[part], want[part]
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y, f"{name} / {part}: call {i} is {x}, recorded at the parent: {y}"
        assert len(a) == len(b), f"{name} / {part}: {len(a)} calls, recorded at the parent: {len(b)}"
