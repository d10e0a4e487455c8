"""`genjax_amd.vmap` through the HIP library on the GPU: the corpus of tests/vmap_checks.py, the launches of the fused
entries, and the device against the CPU mirror bit for bit for the entries that go through a generative function."""
import pytest

from tests import vmap_checks as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [n for n, e in V.CORPUS.items() if e.group not in V.GFI_GROUPS])
def test_vmap_is_the_instances(gpu, name):
    V.check_entry(gpu, name)


@pytest.mark.parametrize("name", [n for n, e in V.CORPUS.items() if e.group in V.GFI_GROUPS])
def test_vmap_is_the_instances_and_the_device_is_the_mirror(gpu, name):
    V.check_device_is_the_mirror(gpu, name)


@pytest.mark.parametrize("name", [n for n, e in V.CORPUS.items() if e.fused])
def test_fused_entries_keep_their_launches(gpu, name):
    V.check_fused_launches(gpu, name)


def test_loop_warns_above_64_instances(gpu):
    V.check_loop_warns_above_64(gpu)
