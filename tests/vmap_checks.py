"""Shared drivers of tests/test_vmap_cpu.py (the C-ABI's CPU mirror) and tests/test_vmap_gpu.py (the HIP library):
the law of `genjax_amd.vmap`,

    vmap(f, in_axes, out_axes)(*args)[i]  ==  f(*instance(args, in_axes, i)),

over a named corpus of mapped functions.  The right-hand side is written here — `instance()` takes element i of every
mapped leaf, the instances' results are stacked in numpy — and never goes through `transforms.vmap`.  (The inner map
of the nested entries is written out on the reference side as well: in numpy for `nested_add` and `nested_mixture_sums`,
as a Python loop over `assess` for `nested_assess_under_keys`.)

Every comparison is bit for bit (float leaves through their uint32 words): both sides run the same float32 arithmetic on
the same inputs.  Where a reduction's batched form could add in another order than the per-instance form (`jnp.sum`,
`mean`, `logsumexp`, `dot`, `cumsum` of a mapped value), `vmap` takes the instances one by one, so the two sides ARE the
same computation; no entry is held to a float64 sum instead.

For the six entries that hand a mapped host array to a generative function the truth is also computed by an oracle twin
of the model (oracle.genjax_oracle), one instance at a time: it does not rest on this package alone."""
from __future__ import annotations

import dataclasses
import warnings
from typing import Any, Callable

import numpy as np
import torch

import genjax_amd as G
from genjax_amd import ChoiceMapBuilder as C, _lib, numpy as jnp
from genjax_amd.core.choice_map import ChoiceMap
from genjax_amd.core.generative import Trace
from genjax_amd.random import Key
from oracle import genjax_oracle as O

from tests import launch_trace as LT


# --- the models (two or three sites: every program stays on the interpreter) -----------------------------------------------
@G.gen
def m(a):
    x = G.normal(a, 1.0) @ "x"
    y = G.normal(x, 1.0) @ "y"
    return y


@O.gen
def om(a):
    x = O.normal(a, np.float32(1.0)) @ "x"
    y = O.normal(x, np.float32(1.0)) @ "y"
    return y


@G.gen
def mv():
    mu = G.normal(0.0, 1.0) @ "mu"
    y = G.normal.vmap(in_axes=(0, None))(jnp.zeros(3), 1.0) @ "y"
    return mu


@G.gen
def ms(scales):
    return G.normal(0.0, scales[1]) @ "x"


@G.gen
def elem(mu, s):
    return G.normal(mu, s) @ "y"


@G.gen
def mp():
    mu = G.normal(0.0, 1.0) @ "mu"
    return elem.vmap(in_axes=(None, 0))(mu, jnp.array([1.0, 2.0, 3.0])) @ "ys"


# --- the corpus ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Entry:
    make: Callable[[torch.device], tuple]     # device -> (f, args)
    in_axes: Any = 0
    out_axes: int = 0
    group: str = "glue"
    fused: bool = False                       # batch polymorphic: ONE call of f, the launches of the batched call
    one_call: bool = False                    # glue the tags let through (elementwise, stored, batch-free): ONE call of f
    reference: Callable = None                # the per-instance truth written out in numpy (else f itself on the instance)
    refuses: Any = None                       # an exception type: vmap must raise it ...
    match: str = ""                           # ... with a message naming the user's construct
    instance_refuses: bool = True             # ... and the per-instance form cannot run either
    max_calls: int = 2
    oracle: Callable[[], list] = None         # the per-instance truth from the oracle twin (a list of B leaf lists)


def keys(b, seed=0):
    return G.split(G.key(seed), b)


def okeys(b, seed=0):
    return O.split(O.key(seed), b)


YS = [0.0, 10.0, 20.0]
F32 = np.float32


def _t(dev, a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def _grid(dev, b, n):
    """[b, n] of distinct, inexact float32 values (a sum's order shows in its last bits)"""
    return _t(dev, (np.arange(b * n, dtype=np.float64).reshape(b, n) * 0.37 + 0.1) ** 1.5 - 3.0)


def _importance_w(k, y):
    return m.importance(k, C["y"].set(y), (0.0,))[1]


def _oracle_importance():
    ks = okeys(3)
    return [[om.importance(ks[i], O.C.kw(y=F32(YS[i])), (F32(0.0),))[1]] for i in range(3)]


def _oracle_importance_trace():
    ks = okeys(3)
    out = []
    for i in range(3):
        tr, w = om.importance(ks[i], O.C.kw(y=F32(YS[i])), (F32(0.0),))
        out.append([tr.get_score(), tr.get_retval(), tr.get_choices()["x"], tr.get_choices()["y"], w])
    return out


def _oracle_assess():
    return [[om.assess(O.C.kw(x=F32(v), y=F32(0.0)), (F32(0.0),))[0]] for v in (0.0, 1.0, 2.0)]


def _oracle_simulate():
    ks = okeys(3)
    return [[om.simulate(ks[i], (F32(YS[i]),)).get_retval()] for i in range(3)]


def _vec_importance(con):
    def f(k, *c):
        tr, w = mv.importance(k, C["y"].set(c[0] if c else con), ())
        return {"y": tr.get_choices()["y"], "w": w, "choices": tr.get_choices()}
    return f


VEC = [0.25, -1.5, 2.0]


def _reduction(name, b, n):
    fn = getattr(jnp, name)

    def make(dev):
        return (lambda v: (fn(v, axis=None), fn(v, axis=0), fn(v, axis=-1))), (_grid(dev, b, n),)
    return Entry(make, group="reductions")


def _refuse_batched_key():
    def user_glue(k):
        if len(k.shape) >= 1:
            raise NotImplementedError("user_glue takes one key at a time")
        return m.simulate(k, (0.0,)).get_retval()
    return user_glue


def _device_error(k):
    raise _lib.GenmiError("user_kernel: launch failed (status 7)")


IDX5 = [0, 1, 1, 3, 2]


def _nested_add_in_numpy(x):
    """instance x of nested_add, the inner map written out: x + i for i = 0..3, in float32"""
    x = F32(x.item())
    return np.stack([F32(x + F32(i)) for i in range(4)])


def _nested_mixture_in_numpy(x):
    """instance x of nested_mixture_sums, the inner map written out: for every cluster i the float32 sum, in element order,
    of the elements of x labelled i (the others count as 0.0)"""
    row = x.detach().cpu().numpy().astype(F32)
    out = []
    for i in range(4):
        acc = F32(0.0)
        for lab, e in zip(IDX5, row):
            acc = F32(acc + (e if lab == i else F32(0.0)))
        out.append(acc)
    return np.stack(out)


CORPUS: dict[str, Entry] = {
    # GFI with mapped host data -----------------------------------------------------------------------------------------
    "gfi_importance_jnp": Entry(lambda dev: (_importance_w, (keys(3), jnp.array(YS))), group="gfi_host", oracle=_oracle_importance),
    "gfi_importance_np": Entry(lambda dev: (_importance_w, (keys(3), np.array(YS, F32))), group="gfi_host", oracle=_oracle_importance),
    "gfi_importance_torch": Entry(lambda dev: (_importance_w, (keys(3), _t(dev, YS))), group="gfi_host", fused=True,
                                  oracle=_oracle_importance),
    "gfi_importance_chm_arg": Entry(lambda dev: ((lambda k, c, a: m.importance(k, c, a)), (keys(3), C["y"].set(jnp.array(YS)), (0.0,))),
                                    in_axes=(0, 0, None), group="gfi_host", oracle=_oracle_importance_trace),
    "gfi_assess_mapped_value": Entry(lambda dev: ((lambda v: m.assess(C["x"].set(v).at["y"].set(0.0), (0.0,))[0]),
                                                  (jnp.array([0.0, 1.0, 2.0]),)), group="gfi_host", oracle=_oracle_assess),
    "gfi_simulate_mapped_arg": Entry(lambda dev: ((lambda k, a: m.simulate(k, (a,)).get_retval()), (keys(3), jnp.array(YS))),
                                     group="gfi_host", oracle=_oracle_simulate),
    # GFI with a vector site ----------------------------------------------------------------------------------------------
    "vec_uniform_b3": Entry(lambda dev: (_vec_importance(jnp.array(VEC)), (keys(3),)), group="gfi_vector", fused=True),
    "vec_uniform_b4": Entry(lambda dev: (_vec_importance(jnp.array(VEC)), (keys(4),)), group="gfi_vector", fused=True),
    "vec_per_instance_b3": Entry(lambda dev: (_vec_importance(None), (keys(3), _grid(dev, 3, 3))), group="gfi_vector", fused=True),
    "vec_per_instance_b4": Entry(lambda dev: (_vec_importance(None), (keys(4), jnp.array(_grid("cpu", 4, 3).numpy()))),
                                 group="gfi_vector"),
    # reductions and shape in glue ------------------------------------------------------------------------------------------
    **{f"reduce_{name}_{b}x{n}": _reduction(name, b, n) for name in ("sum", "mean", "max", "min", "logsumexp")
       for b, n in ((3, 4), (3, 3))},
    "reduce_sum_host_4x3": Entry(lambda dev: ((lambda v: (jnp.sum(v * 2.0), jnp.sum(v, axis=0))), (_grid("cpu", 4, 3).numpy(),)),
                                 group="reductions"),
    "index_3x4": Entry(lambda dev: ((lambda v: (v[0], v[-1], v[1:3])), (_grid(dev, 3, 4),)), group="reductions"),
    "index_3x3": Entry(lambda dev: ((lambda v: (v[0], v[-1], v[1:3])), (_grid(dev, 3, 3),)), group="reductions"),
    "index_host_3x3": Entry(lambda dev: ((lambda v: (v[0], v[-1], v[1:3])), (jnp.array(_grid("cpu", 3, 3).numpy()),)),
                            group="reductions"),
    "shape_len_3x4": Entry(lambda dev: ((lambda v: (v * v.shape[0], len(v), v.ndim)), (_grid(dev, 3, 4),)), group="reductions"),
    "shape_len_4x3": Entry(lambda dev: ((lambda v: (v * v.shape[0], len(v), v.ndim)), (_grid(dev, 4, 3),)), group="reductions"),
    "where_elementwise": Entry(lambda dev: ((lambda v: jnp.where(v > 1, v, 0.0)), (_grid(dev, 3, 4),)), one_call=True, group="reductions"),
    "where_elementwise_host": Entry(lambda dev: ((lambda v: jnp.where(v > 1, v, 0.0) * 2.0), (jnp.array(_grid("cpu", 3, 3).numpy()),)),
                                    one_call=True, group="reductions"),
    "take_mapped_index": Entry(lambda dev: ((lambda i: jnp.take(jnp.array([5.0, 7.0, 11.0]), i)), (jnp.arange(3),)), group="reductions"),
    "dot_unmapped_3x3": Entry(lambda dev: (jnp.dot, (_grid(dev, 3, 3), _t(dev, [0.3, -1.7, 2.9]))), in_axes=(0, None), group="reductions"),
    "dot_unmapped_4x3": Entry(lambda dev: (jnp.dot, (_grid(dev, 4, 3), _t(dev, [0.3, -1.7, 2.9]))), in_axes=(0, None), group="reductions"),
    "cumsum_3x3": Entry(lambda dev: (jnp.cumsum, (_grid(dev, 3, 3),)), group="reductions"),
    "torch_spellings_3x3": Entry(lambda dev: ((lambda v: (v.sum(), v.max(), torch.sum(v, 0))), (_grid(dev, 3, 3),)), group="reductions"),
    "vector_against_mapped_scalar": Entry(lambda dev: ((lambda x, w: x + w), (_grid(dev, 3, 1)[:, 0], _t(dev, [1.0, 2.0, 4.0]))),
                                          in_axes=(0, None), group="reductions"),
    # conversions and truth values: what would read a mapped value as a plain array
    "asarray_then_sum_host": Entry(lambda dev: ((lambda v: jnp.sum(jnp.asarray(v))), (jnp.array(_grid("cpu", 3, 3).numpy()),)),
                                   group="reductions"),
    "asarray_then_sum_tensor": Entry(lambda dev: ((lambda v: jnp.sum(jnp.asarray(v))), (_grid(dev, 3, 3),)), group="reductions"),
    "numpy_conversion_of_float_host": Entry(lambda dev: ((lambda v: np.asarray(v).sum()), (jnp.array(_grid("cpu", 3, 3).numpy()),)),
                                            group="reductions"),
    "all_any_host": Entry(lambda dev: ((lambda v: (jnp.all(v > 4), jnp.any(v > 4))), (jnp.array(np.arange(9.0).reshape(3, 3)),)),
                          group="reductions"),
    "all_any_tensor": Entry(lambda dev: ((lambda v: (jnp.all(v > 4), jnp.any(v > 4))), (_t(dev, np.arange(9.0).reshape(3, 3)),)),
                            group="reductions"),
    "all_any_int_host": Entry(lambda dev: ((lambda v: (jnp.all(v > 4), jnp.any(v > 4), jnp.asarray(v))), (jnp.arange(9).reshape(3, 3),)),
                              group="reductions"),
    "data_of_mapped_tensor": Entry(lambda dev: ((lambda v: v.data.sum()), (_grid(dev, 3, 3),)), group="reductions"),
    "closure_constant_of_length_b": Entry(lambda dev: ((lambda x, w=_t(dev, [1.0, 2.0, 4.0]): x + w), (_grid(dev, 3, 1)[:, 0],)),
                                          group="reductions"),
    "numpy_conversion_of_int_host": Entry(lambda dev: ((lambda v: (np.asarray(v).sum(), torch.as_tensor(v).sum())),
                                                       (jnp.arange(9).reshape(3, 3),)), group="reductions"),
    # a result of the batch's own length that does not depend on the batch (no Key, no generative function in f)
    "fresh_tensor_of_length_b": Entry(lambda dev: ((lambda v: torch.ones(3, device=dev)), (_grid(dev, 3, 3),)), one_call=True,
                                      group="reductions"),
    "closure_constant_returned": Entry(lambda dev: ((lambda v, w=_t(dev, [1.0, 2.0, 4.0]): w), (_grid(dev, 3, 4),)), one_call=True,
                                       group="reductions"),
    # argument plumbing -------------------------------------------------------------------------------------------------------
    "in_axes_none": Entry(lambda dev: ((lambda k, s: ms.simulate(k, (s,)).get_retval()), (keys(3), _t(dev, [0.5, 2.0, 4.0]))),
                          in_axes=(0, None), group="plumbing", fused=True),
    "in_axes_1_out_axes_1": Entry(lambda dev: ((lambda k, l: l * 2.0), (keys(4), _grid(dev, 3, 4))), in_axes=(0, 1), out_axes=1,
                                  group="plumbing", fused=True),
    "nested_tuple_in_axes": Entry(lambda dev: ((lambda k, t: t[0] * 2), (keys(3), (_t(dev, [1.0, 2.0, 3.0]),))), in_axes=(0, (0,)),
                                  group="plumbing"),
    "dict_argument": Entry(lambda dev: ((lambda d: {"s": d["a"] * 2 + d["b"], "a": d["a"]}),
                                        ({"a": _t(dev, [1.0, 2.0, 3.0]), "b": _grid(dev, 3, 1)[:, 0]},)), one_call=True, group="plumbing"),
    "chm_of_host_arrays": Entry(lambda dev: ((lambda c: m.assess(c, (0.0,))[0]),
                                             (C["x"].set(jnp.array([0.0, 1.0, 2.0])).at["y"].set(np.array([0.5, -0.5, 4.0], F32)),)),
                                group="plumbing"),
    "constant_result": Entry(lambda dev: ((lambda k: 1.0), (keys(3),)), one_call=True, group="plumbing"),
    "unmapped_result": Entry(lambda dev: ((lambda k, w: w), (keys(3), _t(dev, [1.0, 2.0, 4.0]))), in_axes=(0, None), one_call=True, group="plumbing"),
    "integer_address": Entry(lambda dev: ((lambda k, i, v: mp.importance(k, C["ys", i, "y"].set(v), ())[1]),
                                          (keys(3), _t(dev, [2, 0, 1], torch.int32), _t(dev, [0.5, -1.0, 2.5]))),
                             group="plumbing", fused=True),
    # two levels ------------------------------------------------------------------------------------------------------------
    "nested_add": Entry(lambda dev: ((lambda x: G.vmap(lambda i: x + i)(jnp.arange(4))), (_t(dev, [0.0, 1.0, 2.0]),)), group="nested",
                        reference=_nested_add_in_numpy),
    "nested_mixture_sums": Entry(lambda dev: ((lambda x: G.vmap(lambda i: jnp.sum(jnp.where(jnp.array(IDX5) == i, x, 0.0)))(jnp.arange(4))),
                                              (_grid(dev, 3, 5),)), group="nested", reference=_nested_mixture_in_numpy),
    "nested_assess_under_keys": Entry(lambda dev: ((lambda k: G.vmap(lambda v: m.assess(C["x"].set(v).at["y"].set(0.0), (0.0,))[0])(
        jnp.array([0.0, 1.0]))), (keys(3),)), group="nested",
        reference=lambda k: torch.stack([m.assess(C["x"].set(v).at["y"].set(0.0), (0.0,))[0] for v in (0.0, 1.0)])),
    # errors: what f raises is f's — raised from the FIRST call, never retried as B single calls (f runs at most twice).
    # The first f refuses a BATCHED key only, so its instances can run (a retry would have hidden the refusal behind
    # B + 1 calls); the second fails always, per instance too ------------------------------------------------------------------
    "refusal_propagates": Entry(lambda dev: (_refuse_batched_key(), (keys(50),)), group="errors", refuses=NotImplementedError,
                                match="user_glue", instance_refuses=False),
    "device_error_propagates": Entry(lambda dev: (_device_error, (keys(50),)), group="errors", refuses=_lib.GenmiError,
                                     match="user_kernel"),
}

GFI_GROUPS = ("gfi_host", "gfi_vector")


# --- the reference side: written here, in numpy --------------------------------------------------------------------------
def instance(a, ax, i):
    """argument `a` of instance i: element i of every mapped leaf along its axis (a Key: key i), numpy arrays and tensors
    alike; unmapped arguments unchanged"""
    if isinstance(ax, (tuple, list)):
        return type(a)(instance(x, k, i) for x, k in zip(a, ax))
    if ax is None:
        return a
    if isinstance(a, Key):
        return a[i]
    if isinstance(a, (torch.Tensor, np.ndarray)):
        return a[(slice(None),) * ax + (i,)]
    if isinstance(a, (tuple, list)):
        return type(a)(instance(x, ax, i) for x in a)
    if isinstance(a, dict):
        return {k: instance(x, ax, i) for k, x in a.items()}
    if isinstance(a, ChoiceMap):
        return a.map_values(lambda v: instance(v, ax, i))
    return a


def leaves(v, path=()):
    """[(path, numpy array)] of a result: tuples, lists, dicts, choice maps, traces (score, return value, choices)"""
    from genjax_amd.engine import materialize
    if isinstance(v, (tuple, list)):
        return [l for k, x in enumerate(v) for l in leaves(x, path + (k,))]
    if isinstance(v, dict):
        return [l for k in sorted(v) for l in leaves(v[k], path + (k,))]
    if isinstance(v, ChoiceMap):
        return [l for a in sorted(v.addresses(), key=repr) for l in leaves(v[a] if a else v.get_value(), path + ("chm",) + tuple(a))]
    if isinstance(v, Trace):
        return leaves(v.get_score(), path + ("score",)) + leaves(v.get_retval(), path + ("retval",)) + \
            leaves(v.get_choices(), path + ("choices",))
    if isinstance(v, torch.Tensor) or hasattr(v, "materialize"):
        return [(path, materialize(v).detach().cpu().numpy())]
    assert isinstance(v, (np.ndarray, np.generic, bool, int, float)), (path, type(v))
    return [(path, np.asarray(v))]


def words(a):
    """a leaf's bits: float32 as uint32 words (a float64 leaf must hold float32 values), integers and bools as int64"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a32 = a.astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), a.astype(np.float64), equal_nan=True), "a float leaf beyond float32"
        return "f", a32.view(np.uint32)
    return ("b" if a.dtype.kind == "b" else "i"), a.astype(np.int64)


def same_leaf(got, want):
    (kg, wg), (kw, ww) = words(got), words(want)
    return kg == kw and wg.shape == ww.shape and bool(np.array_equal(wg, ww))


def batch_of(args, in_axes):
    sizes = set()

    def look(a, ax):
        if isinstance(ax, (tuple, list)):
            for x, k in zip(a, ax):
                look(x, k)
        elif ax is None:
            return
        elif isinstance(a, (Key, torch.Tensor, np.ndarray)):
            sizes.add(int(a.shape[ax]))
        elif isinstance(a, (tuple, list)):
            for x in a:
                look(x, ax)
        elif isinstance(a, dict):
            for x in a.values():
                look(x, ax)
        elif isinstance(a, ChoiceMap):
            for addr in a.addresses():
                look(a[addr], ax)
    axes = in_axes if isinstance(in_axes, (tuple, list)) else (in_axes,) * len(args)
    for a, ax in zip(args, axes):
        look(a, ax)
    assert len(sizes) == 1, sizes
    return sizes.pop(), axes


def per_instance(f, args, axes, b):
    """[leaves of f(instance i)] for every i — the truth"""
    return [leaves(f(*[instance(a, ax, i) for a, ax in zip(args, axes)])) for i in range(b)]


def counted(f):
    calls = [0]

    def g(*a):
        calls[0] += 1
        return f(*a)
    g.__qualname__ = getattr(f, "__qualname__", "f")
    return g, calls


# --- the driver ----------------------------------------------------------------------------------------------------------------
def check_entry(be, name):
    import pytest
    e = CORPUS[name]
    f, args = e.make(be.device)
    b, axes = batch_of(args, e.in_axes)
    g, calls = counted(f)
    if e.refuses is not None:
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # (no loop is taken: nothing warns)
            with pytest.raises(e.refuses, match=e.match):
                G.vmap(g, e.in_axes, e.out_axes)(*args)
        assert calls[0] <= e.max_calls, (name, "f ran", calls[0], "times: the error was retried per instance")
        if e.instance_refuses:
            with pytest.raises(e.refuses, match=e.match):
                f(*[instance(a, ax, 0) for a, ax in zip(args, axes)])
        return None
    want = per_instance(e.reference or f, args, axes, b)
    got = leaves(G.vmap(g, e.in_axes, e.out_axes)(*args))
    print(name, ": B =", b, "; f ran", calls[0], "time(s); leaves", [(p, a.shape) for p, a in got])
    # the tree
    assert [p for p, _ in got] == [p for p, _ in want[0]], (name, "tree", [p for p, _ in got], [p for p, _ in want[0]])
    for i in range(1, b):
        assert [p for p, _ in want[i]] == [p for p, _ in want[0]], (name, "the instances' trees differ")
    for k, (path, leaf) in enumerate(got):
        rows = [want[i][k][1] for i in range(b)]
        ax = e.out_axes if rows[0].ndim >= e.out_axes else 0
        # the batch axis, where out_axes says, with length B
        assert leaf.ndim > ax and leaf.shape[ax] == b, (name, path, "no batch axis of length", b, "at", ax, leaf.shape)
        assert leaf.shape == rows[0].shape[:ax] + (b,) + rows[0].shape[ax:], (name, path, leaf.shape, rows[0].shape)
        # the values, bit for bit
        stacked = np.stack([np.asarray(r) for r in rows], axis=ax)
        assert same_leaf(leaf, stacked), (name, path, "got", leaf, "want", stacked)
    if e.oracle is not None:
        truth = e.oracle()
        for i in range(b):
            assert len(truth[i]) == len(want[i]), (name, "oracle leaves")
            for (path, mine), theirs in zip(want[i], truth[i]):
                assert same_leaf(mine, np.asarray(theirs)), (name, "instance", i, path, "package", mine, "oracle", theirs)
    if e.fused or e.one_call:
        assert calls[0] == 1, (name, "a batch polymorphic function ran", calls[0], "times")
    return got


def parent_arrangement(args, axes):
    """What the map handed a batch polymorphic function before it tagged every mapped leaf — keys and tensors as they
    are with the mapped axis in front, integer tensors tagged as run-time indices, unmapped tensors launch-uniform —
    written out: the launches of `f` on these are the launches a fused map may issue."""
    from genjax_amd.engine import Broadcast, Mapped
    out = []
    for a, ax in zip(args, axes):
        if ax is None:
            out.append(Broadcast(a) if isinstance(a, torch.Tensor) and a.ndim >= 1 else a)
        elif isinstance(a, torch.Tensor):
            t = torch.movedim(a, ax, 0) if ax else a
            out.append(Mapped(t) if t.dtype in (torch.int32, torch.int64) else t)
        else:
            assert isinstance(a, Key), type(a)
            out.append(a)
    return out


def check_fused_launches(be, name):
    """a fused entry issues the C-ABI calls of ONE call of f on the batched values, in the same order"""
    e = CORPUS[name]
    assert e.fused
    f, args = e.make(be.device)
    _, axes = batch_of(args, e.in_axes)
    G.vmap(f, e.in_axes, e.out_axes)(*args)             # (programs are traced and cached by now)
    rec = LT.install(be)
    try:
        rec.start(False)
        G.vmap(f, e.in_axes, e.out_axes)(*args)
        mapped = [c[0] for c in rec.stop()]
        rec.start(False)
        f(*parent_arrangement(args, axes))
        direct = [c[0] for c in rec.stop()]
    finally:
        LT.uninstall(be)
    print(name, ": launches", mapped)
    assert mapped == direct, (name, mapped, direct)


def check_device_is_the_mirror(be, name):
    """the device's leaves of an entry equal the CPU mirror's, bit for bit"""
    import tests.hostsim as hs
    assert be.device.type == "cuda"
    got = check_entry(be, name)
    G.clear_caches()
    mirror = hs.install()
    try:
        want = check_entry(mirror, name)
    finally:
        hs.uninstall()
        G.clear_caches()
        _lib.install(None)
    assert [p for p, _ in got] == [p for p, _ in want]
    for (path, a), (_, c) in zip(got, want):
        assert same_leaf(a, c), (name, path, "device", a, "mirror", c)


def check_loop_warns_above_64(be):
    """taking the loop at more than 64 instances says so once, naming f"""
    import pytest

    def row_sums(v):
        return jnp.sum(v)
    v = _grid(be.device, 65, 2)
    with pytest.warns(UserWarning, match="row_sums") as rec:
        out = G.vmap(row_sums)(v)
    assert len(rec) == 1 and tuple(out.shape) == (65,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        G.vmap(row_sums)(v[:64])


def check_self_check(be, monkeypatch):
    """GENMI_VMAP_CHECK=1, read at call time: a right map passes, a function that is wrong when batched (it hides the
    batch axis from the tags) raises AssertionError"""
    import pytest
    monkeypatch.setenv("GENMI_VMAP_CHECK", "1")
    f, args = CORPUS["gfi_importance_jnp"].make(be.device)
    g, calls = counted(f)
    G.vmap(g)(*args)
    assert calls[0] == 1 + 3                            # the map, then min(B, 4) instances

    def hides_the_axis(k):                              # (what a generative function returns carries no tag)
        return m.simulate(k, (0.0,)).get_retval().sum()
    with pytest.raises(AssertionError, match="vmap check"):
        G.vmap(hides_the_axis)(keys(3))
    monkeypatch.setenv("GENMI_VMAP_CHECK", "0")
    G.vmap(hides_the_axis)(keys(3))


def check_nothing_to_map():
    """a call with no array, tensor or Key leaf to map over is refused (the parent called f on it)"""
    import pytest
    with pytest.raises(ValueError, match="no mapped argument"):
        G.vmap(lambda x: x)([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="no mapped argument"):
        G.vmap(lambda x, y: x, in_axes=(None, None))(torch.ones(3), 2.0)
