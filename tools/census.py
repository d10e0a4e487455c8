#!/usr/bin/env python3
"""Offline (no GPU): the two kernels config 2 of bench.py really launches per step — the noise-hoisted LGSSM step with the
resampling prologue (gmx_jit_kernel) and its NoiseProgram as a background kernel (gmx_jit_background_kernel) — specialised
for gfx950 like tools/dump_isa.py does, and their F / I / X / T histogram (tools/valu_model.py).

    python tools/census.py [label [stem]]  -> profiles/<stem>_<label>.json   (defaults: tree, tile_addressing_census)
                                              /tmp/census_<label>_{chain,background}.s
    GENMI_LIB=<a parent's libgenmi_hip.so> python tools/census.py parent <stem>: the parent's kernels (the library carries
    its own device headers and compile options)

`xi2t` = X + I + 2 T is the number that pays when it falls (an F rides free beside an X).  STATIC
counts over every key mode the kernel carries; what a wave executes is SQ_INSTS_VALU (tools/prof.sh).
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def blobs():
    import numpy as np
    import torch
    import tests.hostsim as hs
    hs.install()
    try:
        import genjax_amd as genjax
        from genjax_amd import workloads
        from genjax_amd.core.choice_map import ChoiceMap
        from genjax_amd.engine import Gathered
        from genjax_amd.static import MinimalGenerate, NoiseProgram
        _, step = workloads.make_lgssm(genjax)
        n = 64
        obs = ChoiceMap.empty().set("y", torch.tensor(0.3))
        p = MinimalGenerate(step, (Gathered(torch.zeros(n), torch.zeros(n, dtype=torch.int32)),), obs, (n,), hoist_noise=True)
        q = NoiseProgram(p.noise, (n,))
        return (np.ascontiguousarray(p.comp.blob, dtype=np.uint32), np.ascontiguousarray(q.comp.blob, dtype=np.uint32))
    finally:
        hs.uninstall()


def census(label="tree"):
    import dump_isa
    import valu_model
    chain, noise = blobs()
    out = {}
    for name, blob, flags in (("chain", chain, "1"), ("background", noise, "2")):
        os.environ["DUMP_ISA_FLAGS"] = flags
        s, meta = dump_isa.compile_blob(blob, f"/tmp/census_{label}_{name}")
        sym, lines = valu_model.kernel_listing(s)
        m = valu_model.model(lines)
        m["xi2t"] = m["X"] + m["I"] + 2 * m["T"]
        m["v_pk"] = sum(1 for ln in lines if re.match(r"\s*v_pk_", str(ln)))
        for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size"):      # (one kernel per code object)
            f = re.search(r"\." + key + r":\s*(\d+)", meta)
            m[key] = int(f.group(1)) if f else None
        out[sym] = m
    out["xi2t_sum"] = sum(v["xi2t"] for v in out.values())
    return out


if __name__ == "__main__":
    label = sys.argv[1] if len(sys.argv) > 1 else "tree"
    stem = sys.argv[2] if len(sys.argv) > 2 else "tile_addressing_census"
    res = census(label)
    path = os.path.join(ROOT, "profiles", f"{stem}_{label}.json")
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res, indent=1))
    print("wrote", path)
