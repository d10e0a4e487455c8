"""Whose code is running under `transforms.vmap`: the mapped function's own glue, or this package.

`vmap(f)` calls `f` once on batched values.  This package's entry points are batch polymorphic; the glue a user writes
around them (`jnp.sum(v)`, `v[0]`, `v.shape`) is not.  While glue runs ("strict"), the tags `vmap` puts on mapped
values (engine.Mapped) let elementwise operations through and answer anything that would see the
batch axis with `NotBatchPolymorphic`, which `vmap` catches to run the instances one by one.  Inside the package the
tags are inert."""
from __future__ import annotations

import functools
import threading


class NotBatchPolymorphic(BaseException):
    """Raised at an operation on a mapped value that would act on the batch axis.  Caught by `transforms.vmap` alone
    (a BaseException, so that no `except Exception` on the way swallows it and returns numbers for the wrong axis);
    the outermost map hands one it cannot settle on as a RuntimeError, so none reaches the caller as it is."""


class _Stack(threading.local):
    """per thread: two threads that map at once do not see each other's mode"""

    def __init__(self):
        self.modes = [False]
        self.entries = 0          # entry points of the package that glue has called (gfi_entry)


_STATE = _Stack()


class _Top:
    """`STRICT[-1]`, `STRICT.append(v)`, `STRICT.pop()` on the calling thread's stack: the top says whether the
    mapped function's own glue is running"""

    def __getitem__(self, i):
        return _STATE.modes[i]

    def append(self, v):
        _STATE.modes.append(v)

    def pop(self):
        return _STATE.modes.pop()


STRICT = _Top()


def strict() -> bool:
    return STRICT[-1]


def entries() -> int:
    """how many times the glue of this thread has called a generative function so far: a map whose function called none
    (and was handed no Key) holds no batched value that is not tagged"""
    return _STATE.entries


class mode:
    """`with mode(True)`: glue is running; `with mode(False)`: the package's own code is"""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        STRICT.append(self.on)

    def __exit__(self, *exc):
        STRICT.pop()
        return False


def internal(fn):
    """a function of this package that treats mapped values as the plain arrays they are (builders that only store
    them, or that are batch polymorphic by construction)"""
    @functools.wraps(fn)
    def run(*a, **k):
        if not STRICT[-1]:
            return fn(*a, **k)
        STRICT.append(False)
        try:
            return fn(*a, **k)
        finally:
            STRICT.pop()
    return run


def refuse(what: str):
    raise NotBatchPolymorphic(what)


def gfi_entry(method):
    """A generative-function-interface method as the mapped function's glue calls it: the package's own code from here
    on (the tags are inert), on untagged values (engine.untag)."""
    @functools.wraps(method)
    def run(self, *a, **k):
        if not STRICT[-1]:
            return method(self, *a, **k)
        from .engine import untag
        _STATE.entries += 1
        STRICT.append(False)
        try:
            return method(self, *untag(a), **untag(k))
        finally:
            STRICT.pop()
    run._gmx_entry = True
    return run
