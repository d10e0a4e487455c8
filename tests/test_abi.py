"""The C-ABI library loads without a GPU and exports every symbol
include/genmi.h declares (no compute calls here); the hostsim harness exports
the same set, so host-logic tests exercise the same boundary."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "genmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gmx_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_surveyed_entry_points():
    syms = declared_symbols()
    for name in ("gmx_version", "gmx_last_error", "gmx_split", "gmx_fold_in", "gmx_program_create",
                 "gmx_program_run", "gmx_program_destroy", "gmx_logsumexp", "gmx_weight_cdf", "gmx_ancestors",
                 "gmx_resample", "gmx_gather", "gmx_mh_accept", "gmx_select", "gmx_categorical_rows"):
        assert name in syms


def test_hip_library_exports_every_declared_symbol():
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(so)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    lib.gmx_version.restype = ctypes.c_int
    from genjax_amd import _lib
    assert lib.gmx_version() == _lib.ABI_VERSION == 8
    # pure-host entry point: Threefry known-answer vector (no GPU involved)
    out = (ctypes.c_uint32 * 2)()
    lib.gmx_threefry2x32_host(ctypes.c_uint32(0x13198A2E), ctypes.c_uint32(0x03707344),
                              ctypes.c_uint32(0x243F6A88), ctypes.c_uint32(0x85A308D3), out)
    assert (out[0], out[1]) == (0xC4923A9C, 0x483DF7A0)


def test_hostsim_exports_the_same_boundary():
    import tests.hostsim as hs
    lib = ctypes.CDLL(hs.build())
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_genmi_lib_names_another_build(tmp_path):
    """GENMI_LIB: the product loads the library the switch names (tuning builds) — and says so when it cannot"""
    import shutil
    import subprocess
    import sys
    import __graft_entry__ as g
    other = tmp_path / "libgenmi_other.so"
    shutil.copy(g.HIP_SO, other)
    code = ("from genjax_amd import _lib; import ctypes; assert _lib.LIB_PATH == %r, _lib.LIB_PATH; "
            "lib = ctypes.CDLL(_lib.LIB_PATH); lib.gmx_version.restype = ctypes.c_int; "
            "assert lib.gmx_version() == _lib.ABI_VERSION") % str(other)
    env = dict(os.environ, GENMI_LIB=str(other))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]


def test_environment_switches_are_the_documented_ones():
    """Every GENMI_* switch the code reads is in DESIGN.md section 10's table (15 of them), and nothing else: a new
    switch is a new code path somebody has to keep parity-tested."""
    import re
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 10. Switches"):]
    documented = set(re.findall(r"`(GENMI_[A-Z_]+)`", sec))
    used = set()
    for base, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in (".git", "gpurun_out", "profiles", "__pycache__", "_build", "experiments")]
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".sh", ".c")) and f != "test_abi.py":
                txt = open(os.path.join(base, f), errors="ignore").read()
                used |= set(re.findall(r"GENMI_[A-Z_]+", txt))
    # GENMI_H: the header's include guard
    used -= {"GENMI_", "GENMI_H"}
    assert not any("GENMI_JIT_DEFS" in open(os.path.join(ROOT, "genjax_amd", *f)).read()
                   for f in (("_lib.py",), ("engine.py",), ("csrc", "gmx_rng.h")))      # (the diagnostic short-Threefry build is gone)
    assert used <= documented, sorted(used - documented)
    assert len(documented) <= 20


def test_product_fails_loudly_without_gpu():
    """No CPU fallback: without a HIP device (and without the test harness
    installed) every entry point raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from genjax_amd import _lib
    _lib.install(None)
    import genjax_amd as genjax
    with pytest.raises(_lib.GenmiError):
        genjax.normal.simulate(genjax.key(0), (0.0, 1.0))


def test_specialisation_compiles_offline():
    """gmx_program_specialize's translation unit builds with hiprtc for gfx950
    (no GPU needed for the compile itself)."""
    import numpy as np
    import torch
    import tests.hostsim as hs
    hs.install()
    try:
        import genjax_amd as genjax
        from genjax_amd import workloads
        from genjax_amd.core.choice_map import ChoiceMap
        from genjax_amd.engine import Gathered
        from genjax_amd.static import MinimalGenerate
        _, step = workloads.make_lgssm(genjax)
        n = 64
        p = MinimalGenerate(step, (Gathered(torch.zeros(n), torch.zeros(n, dtype=torch.int32)),),
                            ChoiceMap.empty().set("y", torch.tensor(0.3)), (n,))
        blob = np.ascontiguousarray(p.comp.blob, dtype=np.uint32)
    finally:
        hs.uninstall()
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    lib = ctypes.CDLL(so)
    lib.gmx_specialize_dryrun.restype = ctypes.c_size_t
    lib.gmx_specialize_dryrun.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                          ctypes.c_char_p, ctypes.c_size_t]
    log = ctypes.create_string_buffer(4096)
    size = lib.gmx_specialize_dryrun(blob.ctypes.data, blob.size, log, 4096, None, 0)
    assert size > 0, log.value.decode()


def test_entry_points_reject_null_arguments_before_any_launch():
    """Host-side validation comes first: with null pointers every entry point returns non-zero and leaves
    a message in gmx_last_error() — nothing reaches the GPU (runs on a box without one)."""
    from genjax_amd import _lib
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    lib = ctypes.CDLL(so)
    lib.gmx_last_error.restype = ctypes.c_char_p
    N, i64, i32, u32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
    calls = {
        "gmx_split": (N, i64(10), i64(0), N, N),
        "gmx_split_rows": (N, i64(4), i64(4), N, N),
        "gmx_fold_in": (N, u32(1), i64(10), N, N),
        "gmx_random_bits": (N, i64(4), i64(4), N, N),
        "gmx_logsumexp": (N, i64(3), i64(5), N, N, N, N),
        "gmx_reduce_max": (N, i64(4), N, N),
        "gmx_weight_cdf": (N, i64(10), i32(40), N, i64(0), N, N, N, N, N),
        "gmx_ancestors": (i32(0), N, N, i64(10), ctypes.c_uint64(0), N, i64(10), i64(0), i64(10), N, N),
        "gmx_resample": (i32(0), N, N, i64(10), i32(40), N, i64(0), N, N, N, N, N),
        "gmx_tile_stats": (N, i64(10), i32(40), N, N, N),
        "gmx_resample_tiles": (i32(0), N, N, i64(10), i32(40), N, N, N, N, N, N),
        "gmx_resample_tiles_p": (i32(0), N, N, i64(10), i32(40), N, N, N, N, N, N),
        "gmx_tile_prefix": (N, N, i64(10), N, N),
        "gmx_multinomial_tiled": (N, N, i64(10), i32(40), N, N, N, N, N, N, N, i32(-1), N),
        "gmx_slot_uniforms": (N, i32(1), i64(10), N, i32(0), N),
        "gmx_resample_tiles_u": (i32(1), N, N, i64(10), i32(40), N, N, N, N, N, N, N),
        "gmx_sorted_uniforms": (N, i32(1), i64(10), N, i32(0), N),
        "gmx_resample_sorted": (N, N, i64(10), i32(40), N, N, N, i32(0), N, N, N, N),
        "gmx_shard_totals": (N, i32(2), i64(1024), N, N, N),
        "gmx_shard_step_tiles": (i32(0), N, N, N, N, N, N, N, i32(40), i32(0), i32(2), i64(1024), i64(4), N, N, N, N),
        "gmx_shard_step_fused": (i32(0), N, N, N, N, N, N, i32(40), i32(0), i32(2), i64(1024), i64(4), N, N, N, N),
        "gmx_gather": (N, N, N, ctypes.c_int32(3), N, i64(10), N),
        "gmx_select": (N, N, N, N, N, ctypes.c_int32(1), i64(10), N),
        "gmx_categorical_rows": (N, N, i64(4), i64(4), N, N),
        "gmx_mh_accept": (N, N, i64(4), N, N),
        "gmx_program_create": (N, ctypes.c_size_t(0), N),
        "gmx_program_run": (N, i64(4), N, N),
        "gmx_shard_plan": (i32(0), N, N, i32(0), i32(4), i64(10), N, N),
        "gmx_shard_route": (i32(0), N, N, N, i32(0), i32(4), i64(10), i64(4), N, N, N, N),
        "gmx_shard_step": (i32(0), N, N, N, N, N, i32(0), i32(4), i64(10), i64(4), N, N, N, N),
        "gmx_shard_step_sorted": (N, N, N, N, N, i32(0), i32(4), i64(10), i64(4), N, N, N, N),
        "gmx_peer_put_stats": (N, _lib.Peer(), i64(1024), N),
        "gmx_shard_step_peer": (i32(0), N, N, _lib.Peer(), N, N, N, N, i32(40), i64(1024), N, N, N, N),
        "gmx_peer_bump": (N, ctypes.c_int32(1), N),
        "gmx_sweep_verdict": (N, N, ctypes.c_int32(0), N, N),
        "gmx_graph_launch": (N, N),
        "gmx_capture_end": (N, N),
        "gmx_timer_start": (N, N),
    }
    for name, args in calls.items():
        rc = getattr(lib, name)(*args)
        assert rc != 0, name
        assert name.encode() in lib.gmx_last_error(), (name, lib.gmx_last_error())


def _hip_and_mirror():
    """the HIP library and the CPU mirror, both loaded here (size exports and refusals make no HIP call)"""
    import tests.hostsim as hs
    so = os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build_hip()
    libs = ctypes.CDLL(so), ctypes.CDLL(hs.build())
    for lib in libs:
        lib.gmx_last_error.restype = ctypes.c_char_p
    return libs


def test_mirror_and_hip_library_state_the_same_sizes():
    """every gmx_*_workspace / _bytes / _words export, on both libraries, over sizes around each tile edge: one statement
    (csrc/gmx_sizes.h), so equal everywhere"""
    import itertools
    i64, i32 = ctypes.c_int64, ctypes.c_int
    ns = [0, 1, 1023, 1024, 1025, 4096, 2 ** 21, 2 ** 21 + 1, 10 ** 7]
    shapes = list(itertools.product([0, 1, 31, 32, 65535, 70000], [0, 1, 4096, 4097, 100000]))
    grid = {
        "gmx_logsumexp_workspace": ([i64, i64], shapes),
        "gmx_sum_rows_workspace": ([i64, i64], shapes),
        "gmx_weight_cdf_workspace": ([i64], [(n,) for n in ns]),
        "gmx_multinomial_workspace": ([i64], [(n,) for n in ns]),
        "gmx_multinomial_tiled_workspace": ([i64], [(n,) for n in ns]),
        "gmx_tile_prefix_words": ([i64], [(n,) for n in ns]),
        "gmx_sorted_uniforms_words": ([i64], [(n,) for n in ns]),
        "gmx_resample_workspace": ([i64], [(n,) for n in ns]),
        "gmx_shard_stats_bytes": ([i64], [(n,) for n in ns]),
        "gmx_shard_plan_words": ([i32], [(w,) for w in (0, 1, 2, 8, 64)]),
        "gmx_peer_landing_bytes": ([i32, i64, i64, i32], list(itertools.product((0, 1, 2, 8, 64), ns, (1, 64), (1, 3)))),
        "gmx_pick_rows_workspace": ([i64, i64], list(itertools.product((1, 7), ns))),
        "gmx_resample_rows_workspace": ([i32, i64, i64], list(itertools.product((0, 1, 2), (1, 7), ns))),
    }
    hip, mirror = _hip_and_mirror()
    differ = []
    for name, (argtypes, cases) in grid.items():
        for lib in (hip, mirror):
            getattr(lib, name).restype = ctypes.c_size_t
            getattr(lib, name).argtypes = argtypes
        for args in cases:
            a, b = getattr(hip, name)(*args), getattr(mirror, name)(*args)
            if a != b:
                differ.append((name, args, a, b))
    assert not differ, differ[:10]
    assert hip.gmx_weight_cdf_workspace(1) == 24 and hip.gmx_resample_workspace(1) == 10240      # (the layouts did not move)


def _shard_refusal_cases(B, B4, key):
    """the sharded / peer family (csrc/gmx_sizes.h "sharded resampling and the fused peer exchange"): every distinct refusal
    of each entry point, as (entry point, arguments, the phrase its message carries).  B: a zeroed 16-byte aligned
    buffer (as a host array of leaf pointers: null leaves); B4: B + 4."""
    from genjax_amd import _lib
    N, i64, i32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int
    ok = dict(kind=0, key=key, rank=0, world=2, n=1024, cap=4, shift=40, p=B, lw=B, stats=B, cdf=B)

    def peer(**kw):
        P = _lib.Peer()
        P.land_d, P.tag_base_d, P.status_d = B.value, B.value, B.value
        P.rank, P.world, P.step, P.tiles, P.capacity, P.leaves = 0, 2, 0, 1, 4, 1
        for f, v in kw.items():
            setattr(P, f, v)
        return P

    def call(name, **kw):
        a = dict(ok, **kw)
        k, K, p, n, c = i32(a["kind"]), a["key"], a["p"], i64(a["n"]), i64(a["cap"])
        r, w, sh, lw, st, cdf = i32(a["rank"]), i32(a["world"]), i32(a["shift"]), a["lw"], a["stats"], a["cdf"]
        P = a.get("peer") or peer()
        return {
            "gmx_shard_plan": (k, K, p, r, w, n, p, p, N),
            "gmx_shard_route": (k, K, p, cdf, r, w, n, c, p, p, p, N),
            "gmx_shard_step": (k, K, p, p, p, cdf, r, w, n, c, p, p, p, N),
            "gmx_shard_step_sorted": (cdf, p, p, p, p, r, w, n, c, p, p, p, N),         # (cdf: the table's place)
            "gmx_shard_totals": (st, w, n, p, p, N),
            "gmx_shard_step_tiles": (k, K, p, p, p, lw, st, p, sh, r, w, n, c, p, p, p, N),
            "gmx_shard_step_fused": (k, K, st, p, p, lw, p, sh, r, w, n, c, p, p, p, N),
            "gmx_peer_put_stats": (st, P, n, N),
            "gmx_shard_step_peer": (k, K, st, P, p, p, lw, p, sh, n, a.get("rows", p), a.get("rows", p), p, N),
        }[name]

    cases = []

    def refuse(name, why, **kw):
        cases.append((name, call(name, **kw), why))

    keyed = ("gmx_shard_plan", "gmx_shard_route", "gmx_shard_step", "gmx_shard_step_tiles", "gmx_shard_step_fused")
    for name in keyed:
        refuse(name, b"null key", key=None)
        refuse(name, b"systematic / stratified only", kind=2)
        refuse(name, b"rank / world out of range", world=0)
        refuse(name, b"rank / world out of range", rank=2)
        refuse(name, b"rank / world out of range", world=1025)
        refuse(name, b"n_per_rank out of range", n=0)
        refuse(name, b"n_per_rank out of range", n=2 ** 31)
        refuse(name, b"null argument", p=N)
    for name in keyed[1:] + ("gmx_shard_step_sorted",):
        refuse(name, b"capacity must be in [1, n_per_rank]", cap=0)
        refuse(name, b"capacity must be in [1, n_per_rank]", cap=1025)
    for name in keyed[1:]:
        refuse(name, b"extended state index exceeds int32", n=2 ** 30, cap=2 ** 30)
    refuse("gmx_shard_step", b"cdf_d must be 16-byte aligned", cdf=B4)
    for name in keyed[3:]:
        refuse(name, b"world <= 64", world=65)
        refuse(name, b"shift out of range", shift=0)
        refuse(name, b"shift out of range", shift=63)
        refuse(name, b"lw_d must be 16-byte and stats_", lw=B4)
        refuse(name, b"8-byte aligned", stats=B4)
    refuse("gmx_shard_step_tiles", b"(use gmx_weight_cdf + gmx_shard_step)", world=65)
    refuse("gmx_shard_step_fused", b"n_per_rank too large (<= 2^21)", n=2 ** 21 + 1)
    refuse("gmx_shard_step_sorted", b"null argument", p=N)
    refuse("gmx_shard_step_sorted", b"rank / world out of range", world=0)
    refuse("gmx_shard_step_sorted", b"rank / world out of range", rank=2)
    refuse("gmx_shard_step_sorted", b"n_per_rank * world out of range (< 2^31)", n=2 ** 30, cap=1)
    refuse("gmx_shard_step_sorted", b"n_per_rank * world out of range (< 2^31)", n=0)
    refuse("gmx_shard_step_sorted", b"extended state index exceeds int32", n=2 ** 29, world=3, cap=2 ** 29)
    refuse("gmx_shard_step_sorted", b"table_d must be 16-byte aligned", cdf=B4)
    refuse("gmx_shard_totals", b"null argument", p=N)
    refuse("gmx_shard_totals", b"world out of range", world=0)
    refuse("gmx_shard_totals", b"world out of range", world=1025)
    refuse("gmx_shard_totals", b"n_per_rank out of range (< 2^31)", n=0)
    refuse("gmx_shard_totals", b"n_per_rank out of range (< 2^31)", n=2 ** 31)
    refuse("gmx_shard_totals", b"stats_all_d must be 8-byte aligned", stats=B4)
    # gmx_peer, by value: each condition of the peer check, through both entry points that take one
    refuse("gmx_peer_put_stats", b"null argument", stats=N)
    for name in ("gmx_peer_put_stats", "gmx_shard_step_peer"):
        for field in ("land_d", "tag_base_d", "status_d"):
            refuse(name, b"peer has a null pointer", peer=peer(**{field: None}))
        refuse(name, b"peer rank / world out of range (world <= 64)", peer=peer(world=65))
        refuse(name, b"peer.step is negative", peer=peer(step=-1))
        refuse(name, b"peer.tiles must be ceil(n_per_rank / 1024) <= 2048", peer=peer(tiles=2))
        refuse(name, b"peer.tiles must be ceil(n_per_rank / 1024) <= 2048", peer=peer(tiles=2049), n=2 ** 21 + 1)
        refuse(name, b"peer.capacity must be in [1, n_per_rank]", peer=peer(capacity=0))
        refuse(name, b"peer.capacity must be in [1, n_per_rank]", peer=peer(capacity=1025))
        refuse(name, b"peer.leaves must be in [1, GMX_PEER_MAX_LEAVES = 32]", peer=peer(leaves=0))
        refuse(name, b"peer.leaves must be in [1, GMX_PEER_MAX_LEAVES = 32]", peer=peer(leaves=33))
    refuse("gmx_peer_put_stats", b"peer rank / world out of range (world <= 64)", peer=peer(rank=2))
    refuse("gmx_peer_put_stats", b"peer rank / world out of range (world <= 64)", peer=peer(world=0))
    # (the step's own rank / world check comes first and names them without "peer"; its extended-index check cannot
    #  fire behind the peer check: n_per_rank <= 2^21, world <= 64, capacity <= n_per_rank)
    name = "gmx_shard_step_peer"
    refuse(name, b"null key", key=None)
    refuse(name, b"systematic / stratified only", kind=2)
    refuse(name, b": rank / world out of range", peer=peer(world=0))
    refuse(name, b": rank / world out of range", peer=peer(rank=2))
    refuse(name, b"n_per_rank out of range", n=0)
    refuse(name, b"null argument", p=N)
    refuse(name, b"shift out of range", shift=0)
    refuse(name, b"shift out of range", shift=63)
    refuse(name, b"lw_d must be 16-byte and stats_own_d 8-byte aligned", lw=B4)
    refuse(name, b"lw_d must be 16-byte and stats_own_d 8-byte aligned", stats=B4)
    refuse(name, b"a leaf pointer is null")                                  # (B as the leaves' host arrays: zeros)
    cases += [("gmx_peer_bump", (N, i32(1), N), b"bad argument"),
              ("gmx_peer_bump", (B, i32(0), N), b"bad argument"),
              ("gmx_sweep_verdict", (N, B, i32(1), B, N), b"bad argument (at most 4 status words)"),
              ("gmx_sweep_verdict", (B, B, i32(1), N, N), b"bad argument (at most 4 status words)"),
              ("gmx_sweep_verdict", (B, B, i32(5), B, N), b"bad argument (at most 4 status words)"),
              ("gmx_sweep_verdict", (B, B, i32(-1), B, N), b"bad argument (at most 4 status words)"),
              ("gmx_sweep_verdict", (B, N, i32(1), B, N), b"bad argument (at most 4 status words)")]
    return cases


def _refusal_cases():
    """(entry point, argument tuple, what the message has to name) for the refusals csrc/gmx_sizes.h states: every one is
    decided before a pointer is read, so one small aligned buffer stands for all of them"""
    from tests import bank_checks, conditional_checks, history_checks
    N, i64, i32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int
    buf = (ctypes.c_int64 * 8)()
    at = (ctypes.addressof(buf) + 15) & ~15
    B, B4 = ctypes.c_void_p(at), ctypes.c_void_p(at + 4)
    key = ctypes.cast(B, ctypes.POINTER(ctypes.c_uint32))
    big = 2 ** 21 + 1

    # the tile-form resamplers as (name, args(kind, n, shift, lw, other pointers), a kind the form takes)
    forms = {
        "gmx_tile_stats": lambda kind, n, shift, lw, p: (lw, i64(n), i32(shift), p, p, N),
        "gmx_resample_tiles": lambda kind, n, shift, lw, p: (i32(kind), key if p else None, lw, i64(n), i32(shift), p, p, p, p, p, N),
        "gmx_resample_tiles_u": lambda kind, n, shift, lw, p: (i32(kind), key if p else None, lw, i64(n), i32(shift), p, p, p, p, p, p, N),
        "gmx_resample_tiles_p": lambda kind, n, shift, lw, p: (i32(kind), key if p else None, lw, i64(n), i32(shift), p, p, p, p, p, N),
        "gmx_resample_sorted": lambda kind, n, shift, lw, p: (key if p else None, lw, i64(n), i32(shift), p, p, p, i32(0), p, p, p, N),
        "gmx_resample_sorted_p": lambda kind, n, shift, lw, p: (key if p else None, lw, i64(n), i32(shift), p, p, p, i32(0), p, p, p, N),
        "gmx_multinomial_tiled": lambda kind, n, shift, lw, p: (key if p else None, lw, i64(n), i32(shift), p, p, p, p, p, p, p, i32(-1), N),
    }
    good = {"gmx_resample_tiles_u": 1}
    cases = []
    for name, args in forms.items():
        k = good.get(name, 0)
        cases += [(name, args(k, 0, 40, B, B), b"n must be positive"),
                  (name, args(k, 10, 0, B, B), b"shift out of range"),
                  (name, args(k, 10, 63, B, B), b"shift out of range"),
                  (name, args(k, 1025, 52, B, B), b"shift too large for n"),
                  (name, args(k, 10, 40, B, N), b"null argument"),
                  (name, args(k, 10, 40, B4, B), b"16-byte aligned")]
        if name not in ("gmx_tile_stats", "gmx_resample_tiles_p", "gmx_resample_sorted_p"):
            cases.append((name, args(k, big, 40, B, B), b"n too large for the fused path"))
    cases += [("gmx_resample_tiles", forms["gmx_resample_tiles"](2, 10, 40, B, B), b"kind must be systematic or stratified"),
              ("gmx_resample_tiles_p", forms["gmx_resample_tiles_p"](4, 10, 40, B, B), b"kind must be systematic or stratified"),
              ("gmx_resample_tiles_u", forms["gmx_resample_tiles_u"](0, 10, 40, B, B), b"stratified only"),
              ("gmx_multinomial_tiled", forms["gmx_multinomial_tiled"](0, 10, 40, B, B)[:-2] + (i32(2), N), b"phase is -1, 0 or 1"),
              ("gmx_resample", (i32(9), key, B, i64(10), i32(40), N, i64(0), B, B, B, B, N), b"unknown kind"),
              ("gmx_resample", (i32(0), key, B, i64(0), i32(40), N, i64(0), B, B, B, B, N), b"n out of range"),
              ("gmx_resample", (i32(0), key, N, i64(10), i32(40), N, i64(0), B, B, B, B, N), b"null argument"),
              ("gmx_resample", (i32(0), key, B, i64(10), i32(40), N, i64(0), B, B, B, B4, N), b"workspace_d must be 16-byte aligned")]
    rows, keep1 = bank_checks.rows_refusal_calls()
    pinned, keep2 = conditional_checks.pinned_refusal_calls()
    hist, keep3 = history_checks.history_refusal_calls()
    cases += [("gmx_resample_rows", a, why) for a, why in rows] + [("gmx_resample_rows_pinned", a, why) for a, why in pinned]
    cases += [c for c in hist if c[0] == "gmx_history_record"]
    Bp = ctypes.cast(buf, ctypes.c_void_p)
    cases += [("gmx_pick_rows", (Bp, Bp, i64(2), i64(10), i64(9), Bp, Bp, Bp, N), b"ld = 9"),
              ("gmx_pick_rows", (Bp, Bp, i64(0), i64(10), i64(10), Bp, Bp, Bp, N), b"rows = 0"),
              ("gmx_lineage", hist[-2][1], b"must be positive")]
    cases += _shard_refusal_cases(B, B4, key)
    return cases, (buf, keep1, keep2, keep3)


def test_mirror_refusals_carry_the_entry_points_message():
    """what both libraries refuse alike (csrc/gmx_sizes.h), the mirror refuses in the device library's words: the entry
    point and the reason in gmx_last_error(), the same bytes on both.  The mirror is asked first; the HIP library only
    sees a call the mirror refused (nothing here may reach a launch)."""
    hip, mirror = _hip_and_mirror()
    cases, _keep = _refusal_cases()
    assert len(cases) >= 223
    for name, args, why in cases:
        assert getattr(mirror, name)(*args) != 0, (name, why)
        said = mirror.gmx_last_error()
        assert said.startswith(name.encode() + b":") and why in said, (name, why, said)
        assert getattr(hip, name)(*args) != 0, (name, why)
        assert hip.gmx_last_error() == said, (name, hip.gmx_last_error(), said)


def _mirror_resample(be, kind, key, lw):
    import torch
    n = lw.numel()
    from genjax_amd.inference import smc
    mx, tot = torch.zeros(1), torch.zeros(1, dtype=torch.int64)
    anc = torch.full((n,), -1, dtype=torch.int32)
    ws = torch.zeros(((be.c.gmx_resample_workspace(n) + 7) // 8,), dtype=torch.int64)
    be.check(be.c.gmx_resample(kind, key, be.ptr(lw), n, smc.cdf_shift(n), None, 0, be.ptr(mx), be.ptr(tot), be.ptr(anc),
                               be.ptr(ws), None), "gmx_resample")
    return mx, tot, anc


def _resample_inputs():
    import numpy as np
    import torch
    n = 1025                                  # two tiles, the second holding one particle
    lw = torch.from_numpy(np.random.default_rng(77).normal(size=n).astype(np.float32) * 3.0)
    return n, lw, (ctypes.c_uint32 * 2)(0x1234567, 0x89abcde)


def test_mirror_resample_multinomial_is_weight_cdf_and_ancestors(hostsim):
    """kind MULTINOMIAL through the product's dispatch (gmx_tile_stats + gmx_weight_cdf + gmx_multinomial) gives the
    ancestors of gmx_weight_cdf + gmx_ancestors"""
    import torch
    from genjax_amd.inference import smc
    be = hostsim
    n, lw, key = _resample_inputs()
    mx, tot, anc = _mirror_resample(be, smc.MULTINOMIAL, key, lw)
    m2, t2 = lw.max().reshape(1).clone(), torch.zeros(1, dtype=torch.int64)
    cdf, a2 = torch.zeros(n, dtype=torch.int64), torch.full((n,), -1, dtype=torch.int32)
    ws = torch.zeros(((be.c.gmx_weight_cdf_workspace(n) + 7) // 8,), dtype=torch.int64)
    be.check(be.c.gmx_weight_cdf(be.ptr(lw), n, smc.cdf_shift(n), None, 0, be.ptr(m2), be.ptr(cdf), be.ptr(t2), be.ptr(ws), None),
             "gmx_weight_cdf")
    be.check(be.c.gmx_ancestors(smc.MULTINOMIAL, key, be.ptr(cdf), n, 0, be.ptr(t2), n, 0, n, be.ptr(a2), None), "gmx_ancestors")
    assert torch.equal(anc, a2) and torch.equal(tot, t2) and torch.equal(mx, m2)
    assert int(anc.min()) >= 0 and int(anc.max()) < n and len(set(anc.tolist())) > 10


def test_mirror_resample_multinomial_tiled_is_the_two_stage_form(hostsim):
    """kind MULTINOMIAL_TILED through the product's dispatch gives the ancestors of gmx_tile_stats +
    gmx_multinomial_tiled(phase = -1)"""
    import torch
    from genjax_amd.inference import smc
    be = hostsim
    n, lw, key = _resample_inputs()
    mx, tot, anc = _mirror_resample(be, smc.MULTINOMIAL_TILED, key, lw)
    shift = smc.cdf_shift(n)
    tmax, agg = torch.zeros(2), torch.zeros(2, dtype=torch.int64)
    be.check(be.c.gmx_tile_stats(be.ptr(lw), n, shift, be.ptr(tmax), be.ptr(agg), None), "gmx_tile_stats")
    m2, t2, a2 = torch.zeros(1), torch.zeros(1, dtype=torch.int64), torch.full((n,), -1, dtype=torch.int32)
    ws = torch.zeros(((be.c.gmx_multinomial_tiled_workspace(n) + 7) // 8,), dtype=torch.int64)
    be.check(be.c.gmx_multinomial_tiled(key, be.ptr(lw), n, shift, be.ptr(tmax), be.ptr(agg), None, be.ptr(m2), be.ptr(t2),
                                        be.ptr(a2), be.ptr(ws), -1, None), "gmx_multinomial_tiled")
    assert torch.equal(anc, a2) and torch.equal(tot, t2) and torch.equal(mx, m2)
    assert int(anc.min()) >= 0 and int(anc.max()) < n and len(set(anc.tolist())) > 10


def test_mirror_resample_past_2048_tiles_takes_the_prefix_forms(hostsim):
    """n = 2^21 + 1 (2049 tiles): the dispatch goes through gmx_tile_prefix + gmx_resample_tiles_p, whose mirror checks
    the prefixes against the log-weights — the ancestors of the array form (gmx_weight_cdf + gmx_ancestors)"""
    import numpy as np
    import torch
    from genjax_amd.inference import smc
    be = hostsim
    n = 2 ** 21 + 1
    lw = torch.from_numpy(np.random.default_rng(78).normal(size=n).astype(np.float32))
    key = (ctypes.c_uint32 * 2)(5, 6)
    mx, tot, anc = _mirror_resample(be, smc.SYSTEMATIC, key, lw)
    m2, t2 = lw.max().reshape(1).clone(), torch.zeros(1, dtype=torch.int64)
    cdf, a2 = torch.zeros(n, dtype=torch.int64), torch.full((n,), -1, dtype=torch.int32)
    ws = torch.zeros(((be.c.gmx_weight_cdf_workspace(n) + 7) // 8,), dtype=torch.int64)
    be.check(be.c.gmx_weight_cdf(be.ptr(lw), n, smc.cdf_shift(n), None, 0, be.ptr(m2), be.ptr(cdf), be.ptr(t2), be.ptr(ws), None),
             "gmx_weight_cdf")
    be.check(be.c.gmx_ancestors(smc.SYSTEMATIC, key, be.ptr(cdf), n, 0, be.ptr(t2), n, 0, n, be.ptr(a2), None), "gmx_ancestors")
    assert torch.equal(anc, a2) and torch.equal(tot, t2) and torch.equal(mx, m2)
