"""engine.fit_program — the size ladder run_gfi and run_edit retrace a program through — driven by a fake `trace`."""
import pytest

from genjax_amd.engine import fit_program
from genjax_amd.program import ProgramTooLarge

LADDER = [(False, False), (True, False), (False, True), (True, True)]


def _tracer(fits_at=None, errors=None):
    """a `trace(force, chain)` that records its calls, raises errors[pass] where given (a size error elsewhere) and
    returns ("entry", pass) at pass `fits_at`"""
    calls = []

    def trace(force, chain):
        k = len(calls)
        calls.append((force, chain))
        if k == fits_at:
            return ("entry", k)
        raise (errors or {}).get(k) or ProgramTooLarge(f"pass {k}")
    return trace, calls


def test_fit_program_is_the_size_ladder():
    # the passes in order; every pass fails with a size error: the FIRST one is the report
    trace, calls = _tracer()
    with pytest.raises(ProgramTooLarge) as e:
        fit_program(trace)
    assert calls == LADDER and str(e.value) == "pass 0"
    # ... the other spelling of a size error (the slot limits), later passes failing with anything at all
    first = ValueError("the program exceeds the ABI slot limits (fake)")
    trace, calls = _tracer(errors={0: first, 1: KeyError("x"), 2: RuntimeError("y")})
    with pytest.raises(ValueError) as e:
        fit_program(trace)
    assert calls == LADDER and e.value is first
    # a program that must stay one launch: two passes
    trace, calls = _tracer()
    with pytest.raises(ProgramTooLarge) as e:
        fit_program(trace, one_launch=True)
    assert calls == LADDER[:2] and str(e.value) == "pass 0"
    trace, calls = _tracer(fits_at=1)
    assert fit_program(trace, one_launch=True) == ("entry", 1) and calls == LADDER[:2]
    # an error of the first pass that is not about size propagates unchanged
    for err in (KeyError("address"), ValueError("not a size error")):
        trace, calls = _tracer(errors={0: err})
        with pytest.raises(type(err)) as e:
            fit_program(trace)
        assert e.value is err and calls == LADDER[:1]
    # a pass that succeeds ends the ladder
    for k in range(4):
        trace, calls = _tracer(fits_at=k)
        assert fit_program(trace) == ("entry", k) and calls == LADDER[:k + 1]
