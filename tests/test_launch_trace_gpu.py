"""The C-ABI calls of the sweep forms that only exist with streams — the sharded sweep's specialised programs, its
one-launch step and its chained MH form, captured sweeps, the one-launch single-GPU step, the chained MH program — and
of the state-layout and BootstrapBank cases, on an MI355X, against the record made there at the parent of the commit
that gave the sweeps one state store and one table of step programs (tests/golden/launch_trace_gpu.json, written by
tests/golden/make_launch_trace.py --gpu): same calls, same order, same integers, same sharing of buffers."""
import pytest

from tests import launch_trace as L


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(L.load_golden("gpu")["cases"]))
def test_calls_on_the_device_are_the_recorded_ones(gpu, name):
    L.check_case(gpu, "gpu", name)
