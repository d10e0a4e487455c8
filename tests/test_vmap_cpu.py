"""`genjax_amd.vmap` on the C-ABI's CPU mirror: vmap(f)(xs)[i] == f(xs[i]) over the corpus of tests/vmap_checks.py, bit for
bit; batch polymorphic functions stay ONE call with the launches of the batched call; errors of f propagate."""
import pytest

from tests import vmap_checks as V


@pytest.mark.parametrize("name", list(V.CORPUS))
def test_vmap_is_the_instances(hostsim, name):
    V.check_entry(hostsim, name)


@pytest.mark.parametrize("name", [n for n, e in V.CORPUS.items() if e.fused])
def test_fused_entries_keep_their_launches(hostsim, name):
    V.check_fused_launches(hostsim, name)


def test_corpus_covers_the_groups():
    groups = [e.group for e in V.CORPUS.values()]
    assert len(V.CORPUS) >= 32
    assert [groups.count(g) >= k for g, k in (("gfi_host", 6), ("gfi_vector", 4), ("reductions", 10), ("plumbing", 7),
                                              ("nested", 3), ("errors", 2))] == [True] * 6
    assert sum(e.oracle is not None for e in V.CORPUS.values()) == 6


def test_loop_warns_above_64_instances(hostsim):
    V.check_loop_warns_above_64(hostsim)


def test_self_check_is_opt_in(hostsim, monkeypatch):
    V.check_self_check(hostsim, monkeypatch)


def test_nothing_to_map_is_refused():
    V.check_nothing_to_map()
