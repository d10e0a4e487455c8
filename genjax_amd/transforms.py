"""`jit` / `vmap` shims for inference scripts written against JAX.

`jit` is the identity (programs are compiled and cached per call signature on first use).

`vmap(f, in_axes, out_axes)` holds `vmap(f)(xs)[i] == f(xs[i])`.  The generative-function-interface methods of this
package are batch polymorphic: a batched `Key` (and tensors whose leading axes match it) run as one fused launch over
all particles, so a function that only passes its arguments on to them is called ONCE on the batched values.  The
glue a user writes around them is not batch polymorphic in general — `jnp.sum(v)`, `v[0]`, `v.shape` would act on the
batch axis — so every mapped value carries a tag (engine.Mapped; a host array moves to the device when it is mapped) that
lets elementwise operations through and stops everything else; `f` is then run once per instance and the results are
stacked (`_loop_instances`).  Correct first, fused where the tags can prove it.
Replaces `jax.jit(jax.vmap(...))` in e.g. README.md:95-118 of the reference.
"""
from __future__ import annotations

import itertools
import os
import re
import warnings

import numpy as np
import torch

from . import _glue
from .random import Key


def jit(f=None, **_kw):
    if f is None:
        return lambda g: g
    return f


def _containers(v, fn):
    """fn over the leaves of tuples / lists / dicts / choice maps / masks (anything else is a leaf)"""
    from .engine import _walk
    return _walk(v, fn)


def _map_leaves(v, fn):
    """fn over the TENSOR leaves"""
    return _containers(v, lambda x: fn(x) if isinstance(x, torch.Tensor) else x)


def _is_host_array(a) -> bool:
    return isinstance(a, np.ndarray) and a.dtype != object and a.dtype.kind in "fiub" and np.ndarray.ndim.__get__(a) >= 1


# torch's own words for two operands whose axes do not line up: glue that mixed a batched value with unmapped data
_SIZE_MISMATCH = re.compile(r"must match the size of tensor|must match the existing size|shape mismatch|not broadcastable|"
                            r"doesn't match the broadcast shape|size mismatch|inconsistent tensor size|"
                            r"Dimension out of range|1D tensors expected|mat1 and mat2 shapes")


def _is_size_mismatch(e) -> bool:
    return type(e) in (RuntimeError, IndexError) and _SIZE_MISMATCH.search(str(e)) is not None


_LEVELS = itertools.count(1)


def _instance(a, ax, i):
    """argument `a` of instance i: element i of every mapped leaf, a `Key`'s key i, unmapped arguments as they are"""
    from .engine import Broadcast, Mapped
    if isinstance(ax, (tuple, list)) and isinstance(a, (tuple, list)):
        return type(a)(_instance(x, k, i) for x, k in zip(a, ax))
    if isinstance(ax, dict) and isinstance(a, dict):
        return {k: _instance(x, ax[k], i) for k, x in a.items()}
    if ax is None:
        return _map_leaves(a, lambda t: t.plain if isinstance(t, Broadcast) else t)

    def leaf(t):
        if isinstance(t, Key):
            return t[i]
        if isinstance(t, Mapped) and t._host is None:
            return t.plain[i]
        if isinstance(t, Mapped):                              # lifted from a host array: its own element, as `xs[i]` gives it
            v = np.asarray(t._host)[i]
            if v.ndim:
                return v.view(type(t._host))
            return v.item() if type(t._host) is not np.ndarray else v
        return t
    return _containers(a, leaf)


def _stack(vs, n):
    """the instances' results, stacked along a new leading axis (inside the axis of an enclosing map)"""
    from .core.choice_map import ChoiceMap
    from .core.mask import Mask
    from .engine import Broadcast, Expanded, Mapped
    v0 = vs[0]
    if any(isinstance(v, Mapped) for v in vs):
        # values of an ENCLOSING map (this one ran inside its mapped function): its axis stays in front
        if not all(isinstance(v, Mapped) and v._lvl == v0._lvl for v in vs):
            _glue.refuse("instances that differ in whether an enclosing map's values reach the result")
        return Mapped(torch.stack([v.plain for v in vs], dim=1), v0._lvl)
    if isinstance(v0, torch.Tensor):
        return torch.stack([v.plain if isinstance(v, (Broadcast, Expanded)) else v for v in vs])
    if isinstance(v0, (bool, int, float)):
        return torch.tensor(vs)
    if isinstance(v0, (np.ndarray, np.generic)) and np.asarray(v0).dtype != object:
        from .numpy import array
        return array(np.stack([np.asarray(v) for v in vs]))
    if isinstance(v0, tuple):
        return tuple(_stack([v[k] for v in vs], n) for k in range(len(v0)))
    if isinstance(v0, list):
        return [_stack([v[k] for v in vs], n) for k in range(len(v0))]
    if isinstance(v0, dict):
        return {k: _stack([v[k] for v in vs], n) for k in v0}
    if isinstance(v0, Mask):
        return Mask(_stack([v.value for v in vs], n), _stack([v.flag for v in vs], n))
    if isinstance(v0, ChoiceMap):
        out = ChoiceMap.empty()
        for a in v0.addresses():
            out = out.set(a, _stack([v[a] for v in vs], n)) if a else ChoiceMap.choice(_stack([v.get_value() for v in vs], n))
        return out
    if isinstance(v0, Key):
        from .random import stack_keys
        return stack_keys(list(vs))
    from .core.generative import Trace
    if isinstance(v0, Trace):
        raise TypeError("vmap: the mapped function is not batch polymorphic as written and returns a trace; traces of "
                        "single instances are not stacked — return the trace's choices, score or return value")
    return v0


def _loop_instances(f, args, axes, n):
    """f on the instances one by one — what `vmap` means — for a function that is not batch polymorphic as written"""
    outs = []
    with _glue.mode(True):             # (values of an enclosing map may still reach `f` through its closure)
        for i in range(int(n)):
            outs.append(f(*[_instance(a, ax, i) for a, ax in zip(args, axes)]))
    return _stack(outs, int(n))


def _with_batch_axis(out, lvl, n, trust_shape):
    """The result of ONE call on the batched values, as `jax.vmap` hands it back: this map's tags come off, and a leaf
    that does not depend on the batch (a constant, an unmapped argument) is broadcast along the new axis.  What a
    generative function (or anything computed from a batched `Key`) returns carries no tag: where `f` was handed a Key
    or called a generative function (`trust_shape`), an untagged tensor counts as batched when its leading axis has the
    batch's length — a constant of exactly that length is then mistaken for batched; elsewhere no untagged leaf is."""
    from .core.choice_map import ChoiceMap
    from .engine import Broadcast, Mapped

    def leaf(v, spread=True):
        if isinstance(v, Mapped):
            if v._lvl == lvl:
                return v.plain if v._host is None else v._host      # (a host array handed back untouched: itself)
            p = v.plain                                                      # an enclosing map's value: its axis first
            return Mapped(p.unsqueeze(1).expand(p.shape[:1] + (n,) + p.shape[1:]), v._lvl)
        if not spread:
            return v.plain if isinstance(v, Broadcast) else v
        if isinstance(v, torch.Tensor):
            if isinstance(v, Broadcast):
                v = v.plain
            elif trust_shape and v.ndim >= 1 and v.shape[0] == n:
                return v
            return v.unsqueeze(0).expand((n,) + tuple(v.shape))
        if isinstance(v, (bool, int, float)):
            return torch.tensor([v] * n)
        if isinstance(v, (np.ndarray, np.generic)) and np.asarray(v).dtype != object:
            from .numpy import array
            a = np.asarray(v)
            return array(np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape)))
        return v

    def walk(v):
        if isinstance(v, tuple):
            return tuple(walk(x) for x in v)
        if isinstance(v, list):
            return [walk(x) for x in v]
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        if isinstance(v, ChoiceMap):
            # a choice map a function BUILDS keeps the package's reading of its values: one without the batch axis is
            # launch-uniform, the same for every instance (`C[idx, "z"].set(v)` over host arrays is the plate's map)
            return _containers(v, lambda x: leaf(x, spread=False))
        return _containers(v, leaf)
    return walk(out)


def _leaves(v, out):
    """the array leaves of a result, in order (a trace: its score, its return value, its choices)"""
    from .core.choice_map import ChoiceMap
    from .core.generative import Trace
    from .core.mask import Mask
    from .engine import materialize
    if isinstance(v, (tuple, list)):
        for x in v:
            _leaves(x, out)
    elif isinstance(v, dict):
        for k in v:
            _leaves(v[k], out)
    elif isinstance(v, Mask):
        _leaves(v.value, out), _leaves(v.flag, out)
    elif isinstance(v, ChoiceMap):
        for a in v.addresses():
            _leaves(v[a] if a else v.get_value(), out)
    elif isinstance(v, Trace):
        _leaves((v.get_score(), v.get_retval(), v.get_choices()), out)
    elif isinstance(v, (torch.Tensor, np.ndarray, np.generic, bool, int, float)):
        v = materialize(v) if isinstance(v, torch.Tensor) else v
        out.append(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
    elif hasattr(v, "materialize"):
        out.append(v.materialize().detach().cpu().numpy())
    return out


def _bits(a, narrow):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        if a.dtype == np.float64 and not narrow:
            return a.view(np.uint64)
        return a.astype(np.float32).view(np.uint32)
    return a.astype(np.int64)


def _same_bits(g, w) -> bool:
    """two leaves bit for bit: doubles as doubles; a double against a float32 (a Python constant that a launch read) is
    narrowed first, as the launch narrows it"""
    narrow = not (g.dtype == np.float64 and w.dtype == np.float64)
    return g.shape == w.shape and np.array_equal(_bits(g, narrow), _bits(w, narrow))


def _self_check(f, out, args, axes, n, name):
    """GENMI_VMAP_CHECK=1: the first instances one by one against the rows of the result, bit for bit"""
    got = _leaves(out, [])
    for i in range(min(int(n), 4)):
        with _glue.mode(True):
            one = f(*[_instance(a, ax, i) for a, ax in zip(args, axes)])
        want = _leaves(one, [])
        assert len(want) == len(got), f"vmap check: {name} returns {len(got)} leaves batched, {len(want)} for instance {i}"
        for k, (g, w) in enumerate(zip(got, want)):
            # (a leaf INSIDE a trace that is launch-uniform — a constant return value — is shown without the batch axis:
            #  it must then be what every instance returns)
            row = g[i] if g.ndim >= 1 and g.shape[0] == n and g[i].shape == w.shape else g
            assert _same_bits(row, w), \
                f"vmap check: leaf {k} of {name} differs from instance {i}: {row!r} against {w!r}"


def vmap(f=None, in_axes=0, out_axes=0):
    """Two spellings share this name.  `genjax.vmap(in_axes=...)` with no function (or a generative function) is the
    reference's COMBINATOR decorator (combinators/vmap.py `vmap`): `@genjax.vmap(in_axes=(0,))` above `@genjax.gen`.
    `vmap(f, in_axes, out_axes)` with an ordinary function stands in for `jax.vmap` in inference scripts:
    `vmap(f)(xs)[i] == f(xs[i])`, bit for bit.

    The arguments are arranged first:
      * an argument mapped along axis k != 0 has that axis moved to the front (every array leaf of a tuple / dict /
        ChoiceMap argument; `in_axes` may be nested like the arguments, and is applied leaf-wise);
      * every mapped leaf is tagged engine.Mapped.  A host array (numpy, `jnp.array / arange / ones`) moves to the
        device first, as float32 / int32 / bool (a float64 numpy array is narrowed as `jnp.array` narrows it, so glue on
        it computes in float32 where `f(xs[i])` on the raw array would compute in doubles); the instances of the
        per-instance route are the host array's own elements.  At least one argument must hold an array, a tensor or
        a `Key` to map over (ValueError otherwise);
      * an argument with in_axes None is shared by all instances: its tensors are marked launch-uniform
        (engine.Broadcast), so a vector whose length happens to equal the batch is not mistaken for per-instance data;
      * mapped axis sizes are checked against each other.
    `f` is then called ONCE on these values.  The generative-function-interface methods are batch polymorphic, and so
    is elementwise arithmetic on the mapped values; that call is the whole map (one fused launch per method).  Anything
    else `f` does with a mapped value — a reduction, an index, `.shape`, `len`, `reshape`, `cat`, `matmul`, `cumsum`,
    mixing it with an array of the same rank — would act on the batch axis: the tag raises, and `f` runs once per
    instance instead, the results stacked (a `warnings.warn` above 64 instances).  Only that, and torch's own
    size-mismatch errors, take the loop: any other error of `f` (a refusal, a device error) is `f`'s and propagates.
      * a result leaf that does not depend on the batch is broadcast along the new axis;
      * out_axes != 0 moves the leading axis of every array result there.
    With GENMI_VMAP_CHECK=1 in the environment the first min(B, 4) instances are also run one by one and compared with
    the result bit for bit (AssertionError on a difference)."""
    from .core.generative import GenerativeFunction
    if f is None:
        from .combinators import vmap as _combinator
        return _combinator(in_axes=in_axes)
    if isinstance(f, GenerativeFunction):
        from .combinators import Vmap
        return Vmap(f, in_axes)
    from .engine import Broadcast, Mapped
    name = getattr(f, "__qualname__", None) or repr(f)

    def wrapped(*args):
        axes = in_axes if isinstance(in_axes, (tuple, list)) else (in_axes,) * len(args)
        if len(axes) != len(args):
            raise ValueError("vmap: in_axes does not match the number of arguments")
        sizes, keyed = set(), []
        lvl = next(_LEVELS)

        def tag(a, ax):
            if isinstance(ax, (tuple, list)):
                if not isinstance(a, (tuple, list)) or len(a) != len(ax):
                    raise ValueError("vmap: in_axes does not match the structure of the arguments")
                return type(a)(tag(x, k) for x, k in zip(a, ax))
            if isinstance(ax, dict):
                if not isinstance(a, dict) or set(a) != set(ax):
                    raise ValueError("vmap: in_axes does not match the structure of the arguments")
                return {k: tag(x, ax[k]) for k, x in a.items()}
            if ax is None:
                return _map_leaves(a, lambda t: t if isinstance(t, Mapped) or t.ndim == 0 else Broadcast(t))
            ax = int(ax)

            def leaf(t):
                if isinstance(t, Key):
                    if ax != 0:
                        raise NotImplementedError("vmap: a Key is mapped along its leading axis")
                    sizes.add(int(t.shape[0]))
                    keyed.append(True)
                    return t
                if isinstance(t, Mapped):
                    # a value of an ENCLOSING map, mapped again inside its function: its own axes sit behind that
                    # map's axis — the enclosing map takes its instances one by one
                    _glue.refuse("a mapped value mapped again by an inner vmap")
                if isinstance(t, torch.Tensor):
                    if t.ndim == 0:
                        raise ValueError("vmap: cannot map over a 0-d tensor (use in_axes=None)")
                    sizes.add(int(t.shape[ax]))
                    return Mapped(torch.movedim(t, ax, 0) if ax != 0 else t, lvl)
                if _is_host_array(t):
                    sizes.add(int(t.shape[ax]))
                    host = np.moveaxis(t, ax, 0) if ax != 0 else t
                    from .engine import _host_to_device            # a device tensor from here on
                    return Mapped(_host_to_device(np.asarray(host)), lvl, host)
                return t
            return _containers(a, leaf)
        new = [tag(a, ax) for a, ax in zip(args, axes)]
        if len(sizes) > 1:
            raise ValueError(f"vmap: mapped axis sizes differ ({sorted(sizes)})")
        if not sizes:
            raise ValueError("vmap: no mapped argument has an array, a tensor or a Key to map over")
        n = sizes.pop()
        try:
            called = _glue.entries()
            with _glue.mode(True):
                out = f(*new)
            out = _with_batch_axis(out, lvl, n, trust_shape=bool(keyed) or _glue.entries() != called)
        except BaseException as e:
            # `f` is not batch polymorphic as written — glue that reduces, indexes or measures a mapped value, or that
            # compares a mapped index with unmapped data (`jax.vmap(lambda i: jnp.sum(jnp.where(idx == i, xs, 0)))(jnp.arange(k))`,
            # the mixture notebook's c10): the instances one by one, results stacked along a new leading axis.  Nothing
            # else is retried: a refusal (NotImplementedError), a device error (GenmiError) or a ValueError is `f`'s own
            if not (isinstance(e, _glue.NotBatchPolymorphic) or _is_size_mismatch(e)):
                raise
            if n > 64:
                warnings.warn(f"vmap: {name} is not batch polymorphic as written ({e}); running its {n} instances one by one",
                              stacklevel=2)
            try:
                out = _loop_instances(f, new, axes, n)
            except _glue.NotBatchPolymorphic as inner:
                if _glue.strict():
                    raise                                        # an enclosing map takes ITS instances one by one
                raise RuntimeError(f"vmap: {name} cannot be mapped: {inner}") from None
        if os.environ.get("GENMI_VMAP_CHECK", "0") == "1" and not _glue.strict():
            _self_check(f, out, new, axes, n, name)
        if out_axes not in (0, None):
            def move(t):
                if isinstance(t, torch.Tensor):
                    return torch.movedim(t, 0, int(out_axes)) if t.ndim > int(out_axes) else t
                if _is_host_array(t) and t.ndim > int(out_axes):
                    return type(t)(np.moveaxis(np.asarray(t), 0, int(out_axes))) if type(t) is not np.ndarray else np.moveaxis(t, 0, int(out_axes))
                return t
            out = _containers(out, move)
        return out
    return wrapped
