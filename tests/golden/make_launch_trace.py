"""Writes tests/golden/launch_trace_cpu.json (the C-ABI's CPU mirror) or, with --gpu, launch_trace_gpu.json (the HIP
library on an MI355X): the C-ABI calls of every case of tests/launch_trace.py, as issued by the tree it runs in.

The record is the yardstick for a later change to the launching Python, so it is made at the commit BEFORE that change,
never from the tree under test: the generator refuses to write while `git status` shows changes under genjax_amd/.
A tree exported from a commit without its git metadata (`git archive`, a copy to a GPU box) has nothing to ask; there
the commit it was exported from is named with --exported-from and goes into the file.

  python tests/golden/make_launch_trace.py [--gpu] [--exported-from COMMIT] [--out FILE] [--only PREFIX [PREFIX ...]]

--only records the cases whose names start with one of the prefixes and no others (the device record holds the forms
that only exist with streams, the state-layout and the bank cases: the GPU suite's time budget has no room for all).
The mirror's "state/" and "bank/" cases are in a file of their own, made at a later parent than the rest:
  --only state/ bank/ --out tests/golden/launch_trace_cpu_state.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def source_commit(exported_from):
    has_git = os.path.exists(os.path.join(ROOT, ".git"))
    if exported_from:
        if has_git:
            sys.exit("--exported-from is for a tree without git metadata; this one has it: commit or stash instead")
        return exported_from
    if not has_git:
        sys.exit("no git metadata here: name the commit this tree was exported from with --exported-from")
    dirty = subprocess.check_output(["git", "status", "--porcelain", "--", "genjax_amd"], cwd=ROOT, text=True).strip()
    if dirty:
        sys.exit("refusing to write: genjax_amd/ differs from the commit (the record must come from the parent of the "
                 "change it is to check, not from the tree under test):\n" + dirty)
    return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, text=True).strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--exported-from", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs="+", default=[""], metavar="PREFIX")
    a = ap.parse_args()
    commit = source_commit(a.exported_from)
    from tests import launch_trace as L
    backend = "gpu" if a.gpu else "cpu"
    if a.gpu:
        from genjax_amd import _lib
        _lib.install(None)
        be = _lib.get()
    else:
        import tests.hostsim as hs
        be = hs.install()
    cases = {}
    for name in [n for n in L.case_names(backend) if n.startswith(tuple(a.only))]:
        cases[name] = L.trace_case(be, name)
        print(name, {k: len(v) for k, v in cases[name].items()}, flush=True)
    out = a.out or L.GOLDEN[backend]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"commit": commit, "backend": backend, "cases": cases}, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
