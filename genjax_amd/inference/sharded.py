"""Particle ensembles sharded across the GPUs of one node.

One process per GPU (`torch.distributed`; backend "nccl" = RCCL over xGMI on the
GPU box, "gloo" in the CPU tests).  Rank g owns the contiguous block of global
particle indices [g*n, (g+1)*n).  Nothing about the result depends on the
number of ranks:

  * per-particle keys are derived from the GLOBAL index (GMX_KEY_SPLIT with
    index_offset = g*n);
  * weights are exact integers in block floating point over tiles of 1024 consecutive GLOBAL indices
    (include/genmi.h "Resampling"): two numbers per tile (max log-weight, fixed-point weight sum) determine the
    whole integer CDF — shards therefore start on a tile boundary (n % 1024 == 0 when sharded);
  * ONE all-gather of the ranks' tile-statistics blocks (12 bytes per 1024 particles) gives every rank the global
    max, hence the global exponent, and EVERY rank's integer total (gmx_shard_totals) — exact integer sums: any
    partition gives the same CDF;
  * rank r resolves the output slots that fall into ITS mass interval
    [offset_r, offset_r + total_r) — for systematic / stratified resampling a
    contiguous slot range [S_r, E_r) every rank derives from the totals alone.
    Slots it owns itself become ancestor indices for the next step's fused gather; the states for slots other
    ranks own go into fixed-capacity send blocks (gmx_shard_step_tiles, which rebuilds the shard's CDF per tile in
    registers) and ONE equal-split all-to-all delivers them behind the receiver's local states
    (balanced weights keep all but O(sqrt(n)) particles per boundary rank-local).

So per SMC step: 1 all-gather (12 B per 1024 particles per rank) and 1 all-to-all (world * capacity * 4 B per
rank), all enqueued on the stream: the host never waits for the device inside a sweep.  (n > 2^21 per rank or > 64
ranks — `cdf_form=True` forces it: all-reduce MAX, gmx_weight_cdf against the global max, all-gather of the 8-byte
totals, gmx_shard_step, all-to-all.)  The evidence terms and the capacity
overflow flag are read once at the end; an overflow (weights so unbalanced that
a rank must ship more than `capacity` particles to one peer) re-runs the sweep
with capacity = n, which always suffices.  xGMI is point-to-point, so the
all-to-all maps onto direct peer links rather than a ring.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .. import _lib
from ..core.choice_map import ChoiceMap
from ..random import Key, lazy_split, split
from .smc import MULTINOMIAL_SORTED, STRATIFIED, SYSTEMATIC, _StateStore, _Sweep, _key_words, cdf_shift, evidence_terms


def systematic_slot_bounds(offsets, total: int, n_total: int, u0: int):
    """f(c) = #{ j in [0, n_total) : (j*2^23 + u0) * total < c * n_total * 2^23 } for each
    CDF offset c — exact Python-integer arithmetic (the same predicate k_offspring /
    k_ancestors evaluate with 128-bit integers)."""
    out = []
    for c in offsets:
        c = int(c)
        if c <= 0 or total == 0:
            out.append(0)
            continue
        num = c * n_total * (1 << 23) - u0 * total          # j * 2^23 * total < num
        if num <= 0:
            out.append(0)
            continue
        den = (1 << 23) * total
        f = (num + den - 1) // den                          # ceil
        out.append(int(min(max(f, 0), n_total)))
    return out


CDF_TILE = 1024


def stats_views(block, n_per_rank: int):
    """(agg, tmax) of one rank's tile-statistics block — `block`: its gmx_shard_stats_bytes(n_per_rank) bytes — as views:
    agg[tiles_pad] int64, then tmax[tiles_pad] float32, tiles_pad = the tile count rounded up to even (the layout
    csrc/gmx_peer.h states: gmx_stats_block_at)"""
    tiles = (n_per_rank + CDF_TILE - 1) // CDF_TILE
    pad = tiles + (tiles & 1)
    return block[:pad * 8].view(torch.int64), block[pad * 8:].view(torch.float32)


def _check_shard_alignment(n_per_rank: int, world: int):
    """The integer CDF is defined on tiles of 1024 consecutive GLOBAL particle indices (include/genmi.h,
    "Resampling"): a shard must start on a tile boundary or the result would depend on the rank count."""
    if world > 1 and n_per_rank % CDF_TILE != 0:
        raise ValueError(f"particles per rank must be a multiple of {CDF_TILE} when sharded over {world} ranks "
                         f"(got {n_per_rank}): shards start on a tile boundary of the global CDF; "
                         f"use {((n_per_rank + CDF_TILE - 1) // CDF_TILE) * CDF_TILE}")


class _ShardRouter:
    """The exchange of ONE sharded resampling, for the sweep and for the one-off global resample alike — the sharded
    counterpart of smc._Resampler.  form_of() picks the form once; the constructor allocates that form's workspaces and
    no other's; bind() builds that form's argument tuples for one step; launch() issues the chain that follows the site
    program: statistics or CDF, collective or local copy, totals, then per routed leaf the routing launch and its
    all-to-all.  Every C entry point of the exchange has its one call site in launch().

      "tiles"  all-gather of the ranks' CDF tile statistics; gmx_shard_step_fused (one leaf, fused=True), else
               gmx_shard_totals + one gmx_shard_step_tiles per leaf
      "peer"   the tiles form over comm.PeerComm: no collective launch — gmx_shard_step_peer routes every leaf, or
               (deferred=True: the one-launch step) the next step's program does
      "cdf"    all-reduce MAX, gmx_weight_cdf against the global max, all-gather of the 8-byte totals, one gmx_shard_step
               (the sorted multinomial: gmx_shard_step_sorted against the step's table) per leaf

    A leaf is (rows, send, recv): the [n + W*C] row whose first n values are routed (ancestors index into all of it),
    the [W*C] send blocks, and where the all-to-all delivers (rows[n:]; None: the caller ships the blocks itself)."""

    @staticmethod
    def form_of(kind, n_per_rank, world, *, cdf_form=False, peer_capable=False, sweep=True):
        """"peer" | "tiles" | "cdf".  sweep=False (the one-off global resample): any per-rank size takes the tile
        statistics — gmx_shard_totals / gmx_shard_step_tiles stride over the table; a sweep's site program and its fused
        routing hold a tile row per workgroup, hence FUSED_RESAMPLE_MAX per rank."""
        from .smc import FUSED_RESAMPLE_MAX
        if kind == MULTINOMIAL_SORTED:
            # routed against the order-statistics table of all N slots (i32 words), which every rank draws in full
            if sweep and n_per_rank * world >= 1 << 31:
                raise NotImplementedError("resample='multinomial_sorted' across ranks: n_per_rank * world < 2^31")
            return "cdf"
        if cdf_form or world > 64 or (sweep and n_per_rank > FUSED_RESAMPLE_MAX):
            return "cdf"
        return "peer" if peer_capable else "tiles"

    def __init__(self, form, kind, n, rank, world, shift, cx=None, comm=False, fused=True, sets=1):
        """cx: the communicator (destinations of collectives come from it); comm: issue the collectives (else local
        copies); sets=2: two sets of tile statistics (the one-launch step reads step t - 1's while it writes step t's)"""
        be = _lib.get()
        dev, W = be.device, world
        self.form, self.kind, self.n, self.rank, self.world, self.shift = form, kind, int(n), rank, world, shift
        self.cx, self.comm, self.fused = cx, bool(comm), bool(fused)
        self.tiles = (self.n + CDF_TILE - 1) // CDF_TILE
        self.capacity = self.land = self.sorted_tab = self.sorted_keys = None

        def zeros(shape, dt):
            return torch.zeros(shape, dtype=dt, device=dev)
        shared = cx.alloc if cx is not None else zeros
        self.plan = zeros((int(be.c.gmx_shard_plan_words(W)),), torch.int64)
        self.totals_all = shared((W,), torch.int64)
        if form == "cdf":
            self.cdf = zeros((self.n,), torch.int64)
            self.total_d = zeros((1,), torch.int64)
            self.ws = zeros(((be.c.gmx_weight_cdf_workspace(self.n) + 7) // 8,), torch.int64)
            if kind == MULTINOMIAL_SORTED:      # every rank draws the SAME table of the N global slots from the step's key
                self.sorted_tab = zeros((int(be.c.gmx_sorted_uniforms_words(self.n * W)),), torch.int32)
            return
        sb = int(be.c.gmx_shard_stats_bytes(self.n))
        self.stats_own = [zeros((sb,), torch.uint8) for _ in range(sets)]
        self.stats_all = shared((W * sb,), torch.uint8)
        self.tile_agg, self.tile_max = zip(*(stats_views(b_, self.n) for b_ in self.stats_own))
        if form == "peer":
            self.tag, self.status = cx.step_words()

    def set_capacity(self, capacity, max_leaves=1):
        """particles a rank may ship to ONE peer; "peer": the landing block for that many (COLLECTIVE)"""
        self.capacity = int(capacity)
        if self.form == "peer":
            # what crosses ranks lands in the communicator's fine-grained landing block; the extended states (and their
            # tails, filled by this rank's own routing launch) are ordinary memory
            self.land, _ = self.cx.landing(self.n, self.capacity, max_leaves)

    def set_sorted_keys(self, words):
        """the resampling keys ([steps, 2] uint32, host) gmx_sorted_uniforms draws each step's table from"""
        hk = np.ascontiguousarray(words, dtype=np.uint32)
        self.sorted_keys = torch.from_numpy(hk.view(np.int32)).to(_lib.get().device)

    def peer(self, step, leaves):
        """the gmx_peer of `step` routing `leaves`: for that step's own launches, and for the next step's program when it
        routes this one as its prologue"""
        p = _lib.Peer()
        p.land_d, p.tag_base_d, p.status_d = self.land.data_ptr(), self.tag.data_ptr(), self.status.data_ptr()
        p.rank, p.world, p.step, p.tiles = self.rank, self.world, step, self.tiles
        p.capacity, p.leaves = self.capacity, len(leaves)
        return p

    def bind(self, t, key, lw, m, tot, leaves, idx, *, w=0, program_stats=False, pmax=None, pmax_rows=0, deferred=False):
        """The argument tuples of step t's exchange (all buffers persistent): log-weights `lw` -> global max `m`,
        global total `tot`, ancestors `idx`, the leaves routed under resampling key `key`.  w: which set of tile
        statistics; program_stats: the site program left them (and put them to the peers); pmax[:pmax_rows]: the block
        maxima gmx_weight_cdf reduces (None: `m` holds the global max already); deferred: the next step's program
        routes this one."""
        P = _lib.get().ptr
        kk = _key_words(key)
        g, W, n, C = self.rank, self.world, self.n, self.capacity
        b = {"keep": (kk, leaves), "entry": "cdf", "pmax": pmax, "stats": None, "put": None, "peer": None, "peer_step": None,
             "gather": None, "totals": None, "sorted": None, "routes": []}
        if self.form == "cdf":
            # the CDF kernel reduces the (all-reduced) block maxima itself and records the max in `m`
            b["stats"] = (P(lw), n, self.shift, None if pmax is None else P(pmax), pmax_rows, P(m), P(self.cdf),
                          P(self.total_d), P(self.ws))
            b["gather"] = (self.totals_all, self.total_d)                # 8 bytes per rank
            head = (self.kind, kk)
            if self.sorted_tab is not None:
                b["entry"], head = "sorted", (P(self.sorted_tab),)
                b["sorted"] = (P(self.sorted_keys[t]), 1, n * W, P(self.sorted_tab), 0)
            b["routes"] = [(head + (P(self.totals_all), P(self.plan), P(tot), P(self.cdf), g, W, n, C, P(rows), P(send),
                                    P(idx)), recv, send) for rows, send, recv in leaves]
            return b
        so = self.stats_own[w]
        if not program_stats:
            b["stats"] = (P(lw), n, self.shift, P(self.tile_max[w]), P(self.tile_agg[w]))
        if self.form == "peer":
            from ctypes import c_void_p
            peer = b["peer"] = self.peer(t, leaves)
            st_arr = (c_void_p * len(leaves))(*[rows.data_ptr() for rows, _s, _r in leaves])
            tl_arr = (c_void_p * len(leaves))(*[recv.data_ptr() for _r, _s, recv in leaves])
            b["keep"] += (st_arr, tl_arr)
            if not program_stats:
                b["put"] = (P(so), peer, n)
            if not deferred:
                b["peer_step"] = (self.kind, kk, P(so), peer, P(self.plan), P(tot), P(lw), P(m), self.shift, n, st_arr,
                                  tl_arr, P(idx))
            return b
        b["gather"] = (self.stats_all, so)                               # 12 bytes per 1024 particles per rank
        if self.fused and len(leaves) == 1:
            # the one routed leaf derives the totals / global max itself (one launch less in the chain)
            rows, send, recv = leaves[0]
            b["entry"] = "fused"
            b["routes"] = [((self.kind, kk, P(self.stats_all), P(self.plan), P(tot), P(lw), P(m), self.shift, g, W, n, C,
                             P(rows), P(send), P(idx)), recv, send)]
            return b
        b["entry"] = "tiles"
        b["totals"] = (P(self.stats_all), W, n, P(self.totals_all), P(m))     # global max + every rank's total
        b["routes"] = [((self.kind, kk, P(self.totals_all), P(self.plan), P(tot), P(lw), P(so), P(m), self.shift, g, W, n, C,
                         P(rows), P(send), P(idx)), recv, send) for rows, send, recv in leaves]
        return b

    def launch(self, b, route_only=False):
        """issue what bind() bound; route_only: the leaves again (another capacity), statistics and totals as they are"""
        be = _lib.get()
        c, st, ck, form = be.c, be.stream(), be.check, self.form
        if not route_only:
            if form == "cdf":
                if self.comm and b["pmax"] is not None:
                    self.cx.all_reduce_max(b["pmax"])                # element-wise MAX of the block maxima (<= 4 KB)
                ck(c.gmx_weight_cdf(*b["stats"], st), "gmx_weight_cdf")        # global max + local integer CDF against it
            elif b["stats"] is not None:
                ck(c.gmx_tile_stats(*b["stats"], st), "gmx_tile_stats")
            if form == "peer":                  # no collective launch: puts + granule waits inside the two kernels
                if b["put"] is not None:
                    ck(c.gmx_peer_put_stats(*b["put"], st), "gmx_peer_put_stats")
                if b["peer_step"] is not None:  # (None: ONE launch per step — step t is routed by the launch of step t + 1)
                    ck(c.gmx_shard_step_peer(*b["peer_step"], st), "gmx_shard_step_peer")
                return
            if self.comm:
                self.cx.all_gather(*b["gather"])
            else:
                b["gather"][0].copy_(b["gather"][1])
            if b["sorted"] is not None:
                ck(c.gmx_sorted_uniforms(*b["sorted"], st), "gmx_sorted_uniforms")       # the step's table of all N slots
            elif b["totals"] is not None:
                ck(c.gmx_shard_totals(*b["totals"], st), "gmx_shard_totals")
        entry = b["entry"]
        for args, recv, send in b["routes"]:                             # slot boundaries + routing, leaf by leaf
            if entry == "fused":
                ck(c.gmx_shard_step_fused(*args, st), "gmx_shard_step_fused")
            elif entry == "tiles":
                ck(c.gmx_shard_step_tiles(*args, st), "gmx_shard_step_tiles")
            elif entry == "sorted":
                ck(c.gmx_shard_step_sorted(*args, st), "gmx_shard_step_sorted")
            else:
                ck(c.gmx_shard_step(*args, st), "gmx_shard_step")
            if self.comm and recv is not None:
                self.cx.all_to_all(recv, send)                       # block s of recv <- block `me` of rank s


class ShardedBootstrapSweep(_Sweep):
    """smc.BootstrapSweep over `dist.get_world_size()` ranks, n particles per rank.

    Per step (the tile-statistics form): site program -> all-gather of the statistics -> gmx_shard_step_fused (the
    totals, the slot bounds, the routing: one launch) -> all-to-all; which form runs and what it launches is
    _ShardRouter's.  NOISE AHEAD as on one GPU (smc._Sweep): the
    step's normal draws come from background programs on a second stream — keyed by the GLOBAL particle index, so the
    draws are the single-process ones — which matters more here than on one GPU: the chain of a sharded step is
    mostly launch boundaries and collective latency, during which the vector ALUs would idle."""

    chained = property(lambda self: self.chain_mh)
    peer_tag = property(lambda self: self.router.tag)
    peer_status = property(lambda self: self.router.status)

    def __init__(self, init, step, n_per_rank: int, T: int, dist, obs_addr="y", step_extra=None, specialize=True,
                 resample="systematic", capacity=None, always_communicate=False, rejuvenate=None, state_addr="x",
                 noise_ahead=None, cdf_form=False, fused=True, comm=None, fuse_step=None, chain_mh=True):
        """cdf_form=True: the three-collective CDF-array form (what n > 2^21 per rank or > 64 ranks take) instead of
        the tile statistics; fused=False: gmx_shard_totals + gmx_shard_step_tiles as two launches (what a vector
        state / the MH move's second leaf take) instead of gmx_shard_step_fused."""
        from .smc import _KINDS
        self.init, self.step, self.n, self.T, self.dist = init, step, int(n_per_rank), int(T), dist
        self.obs_addr = obs_addr
        self.step_extra = step_extra or (lambda t: ())
        self.specialize = specialize
        self.kind = _KINDS[resample] if isinstance(resample, str) else int(resample)
        if self.kind not in (SYSTEMATIC, STRATIFIED, MULTINOMIAL_SORTED):
            raise NotImplementedError("ShardedBootstrapSweep: the router takes the ORDERED schemes — systematic, stratified, "
                                      "multinomial_sorted (one-GPU sweeps also offer multinomial and multinomial_tiled)")
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.N = self.n * self.world
        _check_shard_alignment(self.n, self.world)
        # particles one rank may ship to ONE peer per step before the slow path kicks in
        # default n/32: the slot boundaries of balanced ranks move by O(sqrt(n)) particles per step, so
        # this is a ~10x margin at n = 1e6 while the all-to-all stays ~125 KB per peer
        # (the same at world size 1, where nothing ever crosses ranks: `bench.py --sharded` then issues the collectives
        # with the message sizes a real multi-GPU step has, not a degenerate n-element all-to-all)
        self.capacity = int(capacity) if capacity else max(4096, self.n // 32)
        self.capacity = max(1, min(self.capacity, self.n))
        self.reruns = 0
        # issue the collectives even at world size 1 (exercises / times the RCCL calls on one GPU)
        self.comm = self.world > 1 or bool(always_communicate)
        self.cx = comm           # a communicator to share (comm.make_comm); None: made in prepare()
        self._own_cx = comm is None
        self.graph = None
        self._finished = True    # nothing launched yet: finish() / log_ml() / state() have nothing to wait for
        # rejuvenate: the MH request of smc.BootstrapSweep(rejuvenate=...) (BASELINE config 3).  The move on
        # a resampled particle needs the particle AND the state it was extended from, so two leaves are
        # routed (two routing launches and two all-to-alls per step instead of one).
        self.rejuvenate, self.state_addr = rejuvenate, state_addr
        self.noise_ahead_req = noise_ahead
        self.cdf_form, self.fused_req = bool(cdf_form), bool(fused)
        self._noise_offset, self._noise_total = self.rank * self.n, self.N
        self.fuse_sh_req, self.fuse_sh = fuse_step, False      # None: one launch per step where it applies (prepare)
        self.chain_mh_req, self.chain_mh = bool(chain_mh), False   # rejuvenate=: the move and the extension as ONE program
        self.router = self.p_mhvm_init = self.p_mhvm_step = None
        self.peer_mode = self.tiles_mode = False

    def _chain_step(self, t, skip_vm=False):
        self._step(t)

    def prepare(self, key: Key, ys: torch.Tensor):
        be = _lib.get()
        n, T, dev, W = self.n, self.T, be.device, self.world
        # noise ahead: on request, or by default on a device with streams (specialised programs)
        want_na = self.noise_ahead_req
        # (with an MH move: the chained move + extension program as ONE launch per step — the fused peer exchange — takes
        #  the move's draws from the background stream, as the single-GPU sweep does; any other MH form draws in place)
        mh_na_ok = bool(self.rejuvenate is None or (self.chain_mh_req and be.uses_streams and self.specialize
                                                    and not self.__dict__.get("_mh_na_failed")))
        if want_na is None:
            want_na = (os.environ.get("GENMI_NOISE_AHEAD", "1") != "0" and be.uses_streams and self.specialize
                       and mh_na_ok)
        if want_na and not mh_na_ok:
            raise NotImplementedError("ShardedBootstrapSweep(noise_ahead=True, rejuvenate=...): needs the chained move + "
                                      "extension program as the one-launch sharded step (the fused peer exchange, "
                                      "specialised programs)")
        self.noise_ahead = False
        self._noise_progs = {}
        self.__dict__.pop("_noise_run_cache", None)
        self._drop_graph()                               # prepared again: the graph captured for the previous run goes
        self.key = key
        self._set_observations(ys)
        if self.comm and self.cx is None:
            from .comm import make_comm
            self.cx = make_comm(self.dist, dev)
        # which exchange runs — "peer": the fused peer exchange (comm.PeerComm), no collective launch per step
        self.form = _ShardRouter.form_of(self.kind, n, W, cdf_form=self.cdf_form,
                                         peer_capable=bool(getattr(self.cx, "fused", False) and self.comm))
        self.peer_mode, self.tiles_mode = self.form == "peer", self.form != "cdf"
        self.router = None                               # (made below, once it is known whether the step is one launch)
        self.lw = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.maxs = torch.zeros((T,), dtype=torch.float32, device=dev)           # global max per step
        self.totals = torch.zeros((T,), dtype=torch.int64, device=dev)            # global integer total per step
        self.verdict = torch.zeros((1,), dtype=torch.int64, device=dev)        # gmx_sweep_verdict: 0 fine, 1 overflow, 2 failed
        self.shift = cdf_shift(self.N)
        self.batch = self.window = n
        self._build_init(bool(want_na))
        # the state is the model's return value: a float scalar, or ONE vector of D floats per particle kept
        # struct-of-arrays ([D, n + W*C]) so every component is one routed 4-byte leaf.  Extended state, double-buffered:
        # [ n local | W*C received ]; ancestors index into it; destinations of collectives come from the communicator
        # (peer-mapped memory under GENMI_COMM=p2p)
        shared = self.cx is not None and not self.peer_mode
        mk = (lambda shape: self.cx.alloc(shape, torch.float32)) if shared else None
        width = n + W * self.capacity
        self.store = _StateStore(self.p_init, width, "ShardedBootstrapSweep", tuples=False, alloc=mk)
        self.event, self.D = self.store.event, self.store.D
        self.moved = None
        if self.rejuvenate is not None:
            # store t % 2 of `moved`, [:, :n] = the MH-moved, resampled state step t is extended from; its tail receives
            # the remote copies of it when it travels as the second routed leaf of the NEXT resampling
            self.moved = _StateStore(self.p_init, width, "ShardedBootstrapSweep", tuples=False, alloc=mk)
            self.accept = torch.zeros((n,), dtype=torch.bool, device=dev)
        self._alloc_exchange()
        # the move and the extension that follows it as ONE program (what the single-GPU sweep launches per step): with
        # the routing of the previous step as its prologue a sharded MH step is ONE launch — used when that form applies
        # (fuse_sh below), else the separate programs
        from .smc import BootstrapSweep as _BS
        hn = tuple(_BS.NOISE_ROOTS_MH.split(",")) if want_na else False      # the move's proposal + accept draws
        self._build_steps(bool(want_na), bool(want_na), chain=bool(self.chain_mh_req and be.uses_streams and self.specialize),
                          chain_hoist=hn)
        if want_na and self.rejuvenate is not None:
            if self.p_mhvm_step is not None and self.p_mhvm_step.noise:
                self._noise_setup((self.p_init, self.p_mhvm_init, self.p_mhvm_step), n, T, dev)
            else:
                self._mh_na_failed = True
                self.noise_ahead_req = False if self.noise_ahead_req is None else self.noise_ahead_req
                return self.prepare(key, ys)
        elif want_na and self.p_step.noise:
            self._noise_setup((self.p_init, self.p_step, self.p_step), n, T, dev)
        elif want_na and self.p_init.noise:
            self.noise_ahead_req = False          # the steady-state program draws nothing ahead: the plain programs
            return self.prepare(key, ys)
        # ONE launch per sharded step: the program that gathers routes the previous step itself
        # (gmx_run_args.sh: its workgroup's tile of gmx_shard_step_peer, ancestors as tagged words) — the fused peer
        # exchange, systematic resampling, a scalar / short vector state without an MH move, a table that fits one
        # workgroup's registers, indices that fit an ancestor word
        tiles_ = (n + CDF_TILE - 1) // CDF_TILE
        # (with an MH move the program that GATHERS is the move's — it routes step t - 1 first, two leaves per state
        #  component: x_{t-1} and what it was extended from — and the extension that follows reads the moved state locally:
        #  two launches per step instead of three; round 6)
        want_fuse_sh = bool(self.peer_mode and be.uses_streams and self.specialize and self.kind == SYSTEMATIC
                            and W <= 8 and W * tiles_ <= 1024 and self.peer_leaves <= _lib.PEER_MAX_LEAVES
                            and n + W * self.capacity <= (1 << _lib.ANC_TAG_SHIFT) and self.fuse_sh_req is not False)
        chained = self.rejuvenate is not None and self.p_mhvm_step is not None
        self._routers = (self.p_step,) if self.rejuvenate is None else \
            ((self.p_mhvm_init, self.p_mhvm_step) if chained else (self.p_mh_init, self.p_mh_step))
        if want_fuse_sh and not any(p_.comp.is_specialized() for p_ in self._routers):
            for p_ in self._routers:
                p_.comp.set_fuse_shard_step()
        if self.specialize and be.uses_streams:
            self.p_init.comp.specialize()
            self.p_step.comp.specialize()
            if self.rejuvenate is not None:
                self.p_mh_init.comp.specialize()
                self.p_mh_step.comp.specialize()
                if chained:
                    self.p_mhvm_init.comp.specialize()
                    self.p_mhvm_step.comp.specialize()
        self.partials = torch.zeros((2, (n + 255) // 256), dtype=torch.float32, device=dev)
        writers = (self.p_init,) + (self._routers if chained else (self.p_step,))      # who leaves a step's tile statistics
        self.fuse_sh = bool(want_fuse_sh and all(p_.comp.fuses_shard_step() for p_ in self._routers)
                            and all(p_.comp.writes_tile_stats() for p_ in writers)
                            and all(p_.comp.resident_particles() >= n for p_ in self._routers))
        self.chain_mh = bool(chained and self.fuse_sh)
        if self.rejuvenate is not None and self.noise_ahead and not self.chain_mh:
            # the one-launch chained form did not come about (no fused peer exchange, a program that does not fit): the
            # separate programs draw in place
            self._mh_na_failed = True
            if self.noise_ahead_req:
                raise NotImplementedError("ShardedBootstrapSweep(noise_ahead=True, rejuvenate=...): the chained move + "
                                          "extension program does not run as the one-launch sharded step here")
            return self.prepare(key, ys)
        if self.fuse_sh_req and not self.fuse_sh:
            raise NotImplementedError("ShardedBootstrapSweep(fuse_step=True): needs the fused peer exchange, systematic "
                                      "resampling, specialised programs that leave tile statistics, world <= 8")
        # (the one-launch step reads step t - 1's log-weights / statistics while it writes step t's: two sets)
        self.lw_pp = [self.lw, torch.zeros_like(self.lw)] if self.fuse_sh else [self.lw, self.lw]
        if self.fuse_sh:
            self.sh_status = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.router = _ShardRouter(self.form, self.kind, n, self.rank, W, self.shift, cx=self.cx, comm=self.comm,
                                   fused=self.fused_req, sets=2 if self.fuse_sh else 1)
        self.router.set_capacity(self.capacity, self.peer_leaves)
        self.plan = self.router.plan
        self._set_step_keys(key)
        if self.kind == MULTINOMIAL_SORTED:
            self.router.set_sorted_keys(np.stack([self.step_keys[t][1].host() for t in range(T)]))
        if self.comm and self.world > 1 and hasattr(self.dist, "barrier"):
            # ranks leave prepare() together (hiprtc compiles are seconds apart between ranks): the bounded waits of
            # the peer-mapped exchanges only ever see the microseconds of skew a running sweep has
            self.dist.barrier()
        return self

    def _alloc_exchange(self):
        dev, n, W, C = _lib.get().device, self.n, self.world, self.capacity
        # routed leaves per step: every component of the state and, with an MH move, of what it was extended from
        self.peer_leaves = self.D * (2 if self.rejuvenate is not None else 1)
        if self.peer_mode and self.peer_leaves > _lib.PEER_MAX_LEAVES:
            raise NotImplementedError("ShardedBootstrapSweep over the fused peer exchange: at most "
                                      f"{_lib.PEER_MAX_LEAVES} routed leaves (GMX_PEER_MAX_LEAVES)")
        if self.router is not None:                      # (the overflow re-run: the landing block and the stores for the
            self.router.set_capacity(C, self.peer_leaves)         #  new capacity)
            for store in (self.store, self.moved):
                if store is not None:
                    store.allocate(n + W * C)
        self.send = torch.zeros((self.peer_leaves, W * C), dtype=torch.float32, device=dev)      # one row per routed leaf
        self.idx = self.index = torch.zeros((n,), dtype=torch.int32, device=dev)
        self._bound = [None] * self.T

    def _leaves(self, t):
        """what step t's resampling routes, in issue order: every component of x_t, then (an MH move, t >= 1) every
        component of the state it was extended from — _ShardRouter's (rows, send, recv)"""
        rows = self.store.leaves(t % 2)
        if self.rejuvenate is not None and t >= 1:
            rows += self.moved.leaves(t % 2)
        return [(r, self.send[i], r[self.n:]) for i, r in enumerate(rows)]

    def _shard_in(self, t):
        """the prologue of step t's gathering launch in the one-launch form: it ROUTES step t - 1 first — that step's
        log-weights, statistics, leaves and resampling key"""
        pw = (t - 1) % 2
        prev = self._leaves(t - 1)
        kh_ = self.step_keys[t - 1][1].host()
        return dict(lw=self.lw_pp[pw], stats_own=self.router.stats_own[pw], plan=self.plan, total_out=self.totals[t - 1:t],
                    max_out=self.maxs[t - 1:t], status=self.sh_status, shift=self.shift,
                    tag=1 + (t - 1) % _lib.ANC_TAG_MAX, key=(int(kh_[0]), int(kh_[1])), peer=self.router.peer(t - 1, prev),
                    state=[rows for rows, _s, _r in prev], tail=[recv for _r, _s, recv in prev])

    def _bind_step(self, t):
        """Everything step t launches, bound once (all buffers are persistent): the site programs' launch arguments
        and the router's for the exchange that follows."""
        be, R = _lib.get(), self.router
        n, g = self.n, self.rank
        mh, prog, leaves, key, bufs = self._programs(t)
        w = t % 2 if self.fuse_sh else 0                 # (one launch per step: two sets of log-weights / statistics)
        lw = self.lw_pp[w]
        bufs[prog.wo[1]] = lw.reshape(1, n)
        writes_stats = self.tiles_mode and prog.comp.writes_tile_stats()
        rows = int(be.c.gmx_program_grid(prog.comp.handle, n))        # block maxima the site program writes
        route = R.bind(t, self.step_keys[t][1], lw, self.maxs[t:t + 1], self.totals[t:t + 1], self._leaves(t), self.idx, w=w,
                       program_stats=writes_stats, pmax=self.partials[0, :rows], pmax_rows=rows,
                       deferred=self.fuse_sh and t + 1 < self.T)
        shard_in = self._shard_in(t) if self.fuse_sh and t >= 1 else None
        # keys of the GLOBAL particle index: split(key, N)[g*n + i]
        if mh is not None:
            mprog, mleaves, mkey, mbufs = mh
            mh = (mprog.comp, mprog.comp.bind(mleaves, (n,), lazy_split(mkey, self.N), out_buffers=mbufs,
                                              index_offset=g * n, shard_in=shard_in), mleaves)
            shard_in = None                       # (the move routed: the extension reads its output locally)
        if writes_stats:        # the workgroup maxima land in the statistics block (red_out plane 0), the sums beside them
            vm = prog.comp.bind(leaves, (n,), lazy_split(key, self.N), red_out=R.tile_max[w], out_buffers=bufs,
                                index_offset=g * n, tile_stats=(R.tile_agg[w], self.shift), peer=route["peer"],
                                shard_in=shard_in)
        else:
            vm = prog.comp.bind(leaves, (n,), lazy_split(key, self.N), red_out=self.partials, out_buffers=bufs,
                                index_offset=g * n)
        return {"mh": mh, "prog": prog.comp, "vm": vm, "route": route, "keep": leaves}

    def _step(self, t):
        b = self._bound[t]
        if b is None:
            b = self._bound[t] = self._bind_step(t)
        if b["mh"] is not None:
            b["mh"][0].launch(b["mh"][1])                               # MH move on the resampled particles
        b["prog"].launch(b["vm"])                                      # x_t, lw_t, block maxima
        self.router.launch(b["route"])

    def kernel_timers(self):
        """The site-program launch of a mid-sweep step (no collectives): bench.py's roofline kernel."""
        t = max(1, self.T // 2)

        def vm():
            _mh, prog, leaves, key, bufs = self._programs(t)
            bufs[prog.wo[1]] = self.lw.reshape(1, self.n)
            prog.comp.run(leaves, (self.n,), lazy_split(key, self.N), red_out=self.partials, out_buffers=bufs,
                          index_offset=self.rank * self.n)
        return {"k_vm": vm}

    def enqueue(self):
        self._finished = False
        self.plan.zero_()
        if self.peer_mode:       # this sweep's tags: T more than the last one's (inside a captured graph too)
            be = _lib.get()
            be.check(be.c.gmx_peer_bump(be.ptr(self.peer_tag), self.T, be.stream()), "gmx_peer_bump")
        if self.noise_ahead:
            self._enqueue_noise_ahead()
        else:
            for t in range(self.T):
                self._step(t)
        self._enqueue_verdict()

    def _status_words(self):
        """device words whose non-zero value fails the sweep: the communicator's error word, the peer exchange's, the
        one-launch step's (an ancestor word that never arrived)"""
        words = []
        if self.comm and hasattr(self.cx, "failed_word"):
            words.append(self.cx.failed_word())
        if self.comm and self.peer_mode:
            words.append(self.peer_status[0:1])
        if self.fuse_sh:
            words.append(self.sh_status[0:1])
        return words

    def _enqueue_verdict(self):
        """the last node of a sweep: overflow flag and status words folded into ONE device word (gmx_sweep_verdict), so
        that finish() costs one read by the host (it was four reads and five small launches: 250 us of a 1.6-ms sweep)"""
        from ctypes import c_void_p
        be = _lib.get()
        words = self._status_words()
        arr = (c_void_p * max(1, len(words)))(*[c_void_p(w.data_ptr()) for w in words])
        be.check(be.c.gmx_sweep_verdict(be.ptr(self.plan[2:3]), arr, len(words), be.ptr(self.verdict), be.stream()),
                 "gmx_sweep_verdict")

    def capture(self):
        """OPT-IN across GPUs (`bench.py --rccl-graph`; the default at world size 1): capture the whole sweep — kernels AND the
        RCCL collectives, which comm.RcclComm issues on this same stream — into one hipGraph so
        the host leaves the loop.  Exercised at world size 1 only (no multi-GPU box in the build
        loop); the default multi-GPU path enqueues eagerly."""
        if self.comm and not self.cx.graph_safe:
            raise RuntimeError("capture() needs the direct RCCL communicator (torch.distributed's watchdog "
                               "queries events recorded inside the capture)")
        return super().capture()

    def launch(self):
        self._finished = False
        super().launch()

    def finish(self):
        """Read the overflow flag (one sync per sweep; COLLECTIVE — every rank calls it, which
        launch-then-state()/log_ml() on all ranks does); re-run with full capacity if it is set anywhere."""
        if self._finished:
            return self
        # a wait that timed out (a peer that never arrived) fails the sweep on EVERY rank instead of handing back stale
        # particles: the status words travel with the overflow flag — folded into `verdict` by the sweep's last node
        if self.comm:
            self.cx.all_reduce_max(self.verdict)
        flag = int(self.verdict.item())
        if flag >= 2:
            raise RuntimeError("ShardedBootstrapSweep: a peer's data did not arrive in time on some rank (the "
                               "peer-mapped exchange gave up waiting): the sweep's results are not valid")
        if flag != 0:
            self.reruns += 1
            self.capacity = self.n
            # the captured sweep holds the old exchange buffers and the communicator's kernels: release it
            # (after the stream has drained) before the buffers go away — a dropped-but-live graph is what
            # made ncclCommDestroy hang at teardown; the re-run and later launches are eager
            self._drop_graph()
            self._alloc_exchange()
            self.enqueue()
            assert int(self.plan[2].item()) == 0
        self._finished = True
        return self

    def close(self):
        """Release the captured graph, then the direct RCCL communicator — in that order: a captured sweep
        holds the communicator's kernels and ncclCommDestroy waits on it forever otherwise (measured: a hang at
        teardown).  COLLECTIVE when a communicator exists."""
        be = _lib.get()
        self._drop_graph()
        if self.cx is not None and hasattr(self.cx, "destroy") and getattr(self, "_own_cx", True):
            if be.uses_streams:
                torch.cuda.synchronize()
            self.cx.destroy()
        self.cx = None

    def log_ml(self) -> float:
        self.finish()
        acc = 0.0
        for m, tot in zip(self.maxs.cpu().tolist(), self.totals.cpu().numpy().view(np.uint64).tolist()):
            acc += evidence_terms(m, tot, self.shift, self.N)
            if acc == -math.inf:
                break
        return acc

    def state(self):
        """this rank's resampled particles after the last step (global slots [g*n, (g+1)*n))"""
        self.finish()
        return self.store.take((self.T - 1) % 2, self.idx)


class CountingComm:
    """Wraps a communicator and counts its collectives (tests; `sharded_importance_resample(..., stats=...)`)."""

    def __init__(self, inner):
        self.inner, self.counts = inner, {"all_reduce_max": 0, "all_gather": 0, "all_to_all": 0}
        self.rank, self.world, self.name = inner.rank, inner.world, inner.name

    def all_reduce_max(self, t):
        self.counts["all_reduce_max"] += 1
        return self.inner.all_reduce_max(t)

    def all_gather(self, out, inp):
        self.counts["all_gather"] += 1
        return self.inner.all_gather(out, inp)

    def all_to_all(self, out, inp):
        self.counts["all_to_all"] += 1
        return self.inner.all_to_all(out, inp)

    def alloc(self, shape, dtype=torch.float32):
        return self.inner.alloc(shape, dtype)


def sharded_importance_resample(target, k_per_rank: int, key: Key, dist, kind="systematic", capacity=None, comm=None,
                                stats: dict | None = None, cdf_form=False):
    """BASELINE config 4 across ranks: `ImportanceK(target, k_particles = world * k_per_rank).run_smc(key)`
    with rank g holding particles [g*k, (g+1)*k) (same key tree: keys split(sub, K)[g*k + i], so the
    ensemble is the single-process one), then ONE global resampling with ONE plan for the whole trace (_ShardRouter):

      1. tile statistics of the local log-weights (gmx_tile_stats)         -> all-gather (12 B per 1024 particles)
      2. gmx_shard_totals: global max + every rank's integer total; gmx_shard_step_tiles routes ONE 4-byte leaf:
         each particle's LOCAL INDEX — so `send_idx[d*C + k]` names the local particle that fills slot k of the block
         this rank ships to rank d, and `next_idx` says where each of this rank's slots finds its ancestor;
      3. every 4-byte row of every trace leaf (10 latents for 8-schools) is packed by `send_idx` into one
         [world, rows, C] buffer                                              -> ONE equal-split all-to-all
      4. one gather by `next_idx` over [local | received] rebuilds every leaf.

    Two data-path collectives per resampling whatever the number of leaves (the first form did one all-to-all and one
    routing launch PER ROW, plus a max all-reduce and a totals all-gather), and one 8-byte all-reduce for the
    capacity-overflow flag.  (More than 64 ranks or multinomial_sorted: the CDF-array form computes the
    same plan — all-reduce of the max, gmx_weight_cdf, all-gather of the totals, gmx_shard_step.)
    `stats`, if given, receives {"collectives": {...}, "rows": R, "capacity": C, "form": ...}.
    Returns (ParticleCollection of this rank's k resampled particles, this rank's pre-resampling log-weights).
    COLLECTIVE: every rank calls it."""
    _check_shard_alignment(int(k_per_rank), dist.get_world_size())
    from .smc import _KINDS, LogMLOffset, ParticleCollection, trace_map
    from ..engine import materialize
    be = _lib.get()
    dev = be.device
    g, W = dist.get_rank(), dist.get_world_size()
    n, K = int(k_per_rank), int(k_per_rank) * dist.get_world_size()
    kind = _KINDS[kind] if isinstance(kind, str) else int(kind)
    if kind not in (SYSTEMATIC, STRATIFIED, MULTINOMIAL_SORTED):
        raise NotImplementedError("sharded_importance_resample: the router takes the ordered schemes (systematic, "
                                  "stratified, multinomial_sorted)")
    if comm is None and W > 1:
        from .comm import make_comm
        comm = make_comm(dist, dev)
    if comm is not None:
        comm = CountingComm(comm)
    key, sub = split(key)                                            # smc.py:299
    trs, lw = target.importance(lazy_split(sub, n, offset=g * n), ChoiceMap.empty())
    lw = lw.float().contiguous()
    shift = cdf_shift(K)                                             # (resampling key: the algorithm's leftover `key`)
    mx = torch.empty((1,), dtype=torch.float32, device=dev)
    gtotal = torch.zeros((1,), dtype=torch.int64, device=dev)
    router = _ShardRouter(_ShardRouter.form_of(kind, n, W, cdf_form=cdf_form, sweep=False), kind, n, g, W, shift,
                          cx=comm, comm=W > 1, fused=False)
    if router.form == "cdf":
        # global max (deterministic LSE kernel's max output); the router: local CDF against it, totals
        dummy = torch.empty((1,), dtype=torch.float32, device=dev)
        rows_ws = torch.empty(((be.c.gmx_logsumexp_workspace(1, n) + 3) // 4,), dtype=torch.int32, device=dev)
        be.check(be.c.gmx_logsumexp(be.ptr(lw), 1, n, be.ptr(dummy), be.ptr(mx), be.ptr(rows_ws), be.stream()), "gmx_logsumexp")
        if W > 1:
            comm.all_reduce_max(mx)
        if kind == MULTINOMIAL_SORTED:        # every rank draws the same table of the K global slots from the key
            router.set_sorted_keys(key.host().reshape(1, 2))

    lazy_out = W == 1
    # ---- every per-particle leaf of the trace as 4-byte rows [R, n] ----
    # (ONE rank: nothing is shipped — every slot's ancestor is local — so no leaf is packed at all: the new trace's leaves
    #  are lazy gathers through next_idx, materialised when read, as smc.resample's are)
    specs, rows = [], []

    def collect(v):
        v = materialize(v)
        if tuple(v.shape[:1]) != (n,):
            specs.append(None)
            return v
        orig = v.dtype
        if v.element_size() == 8:                                     # int64 / float64: two 4-byte rows per value
            flat = v.reshape(n, -1).contiguous().view(torch.int32)
        elif v.element_size() == 4:
            flat = v.reshape(n, -1)
        elif orig in (torch.bool, torch.uint8, torch.int8, torch.int16):
            flat = v.to(torch.int32).reshape(n, -1)                   # small integers travel as i32 and come back as they were
        else:
            raise TypeError(f"sharded_importance_resample: cannot route a leaf of dtype {orig}")
        specs.append((orig, tuple(v.shape), flat.dtype, len(rows), flat.shape[1]))
        for c in range(flat.shape[1]):
            rows.append(flat[:, c].contiguous().view(torch.float32))
        return v
    if not lazy_out:
        trace_map(trs, collect)
    R = len(rows)
    table = torch.stack(rows) if R else torch.zeros((0, n), dtype=torch.float32, device=dev)      # [R, n]

    # (ONE rank ships nothing: no send blocks to size, no overflow to ask the device about — and no host sync)
    C = 1 if W == 1 else max(1, min(int(capacity) if capacity else max(4096, n // 32), n))
    local_index = torch.arange(n, dtype=torch.int32, device=dev)                      # the ONE routed leaf
    again = False
    while True:
        next_idx = torch.zeros((n,), dtype=torch.int32, device=dev)
        send_idx = torch.zeros((W * C,), dtype=torch.int32, device=dev)              # unused capacity: particle 0 (valid)
        router.set_capacity(C)
        if again:
            router.plan.zero_()
        router.launch(router.bind(0, key, lw, mx, gtotal, [(local_index, send_idx, None)], next_idx), route_only=again)
        if W == 1:
            break
        flag = router.plan[2:3].clone()
        comm.all_reduce_max(flag)
        if int(flag.item()) == 0:
            break
        C, again = n, True                                           # always sufficient
    # ---- pack by destination, ONE all-to-all, one gather ----
    if W > 1 and R:
        packed = table[:, send_idx.long()].reshape(R, W, C).permute(1, 0, 2).contiguous()          # [W, R, C]
        recv = comm.alloc(tuple(packed.shape), packed.dtype)                                       # a collective's destination
        comm.all_to_all(recv.view(-1), packed.view(-1))
        # the local ancestors by ONE gather of the table; the few slots whose ancestor arrived from another rank are then
        # filled from the received blocks (no [R, n + W * C] copy of the whole table in between)
        far = next_idx >= n
        moved = table[:, torch.where(far, torch.zeros_like(next_idx), next_idx).long()]              # [R, n]
        rp = far.nonzero().squeeze(1)
        if rp.numel():
            moved[:, rp] = recv.permute(1, 0, 2).reshape(R, W * C)[:, (next_idx[rp] - n).long()]
    else:
        moved = table[:, next_idx.long()] if R else table                                             # [R, n]
    it = iter(specs)

    def rebuild(v):
        sp = next(it)
        if sp is None:
            return v
        orig, shape, fdt, r0, cols = sp
        out = moved[r0:r0 + cols].t().contiguous().view(fdt)
        if torch.empty((), dtype=orig).element_size() == 8:
            out = out.contiguous().view(orig)
        elif out.dtype != orig:
            out = (out != 0) if orig == torch.bool else out.to(orig)
        return out.reshape(shape)
    if lazy_out:
        from ..engine import Gathered

        def lazy(v):
            v = materialize(v)
            return Gathered(v, next_idx) if isinstance(v, torch.Tensor) and tuple(v.shape[:1]) == (n,) else v
        new = trace_map(trs, lazy)
    else:
        new = trace_map(trs, lambda v: rebuild(materialize(v)))
    if stats is not None:
        stats.update(collectives=dict(comm.counts) if comm is not None else {}, rows=R, capacity=C,
                     form="tile statistics" if router.form == "tiles" else "cdf array")
    off = LogMLOffset().plus(mx, gtotal, shift, K)
    out = ParticleCollection(new, None, True, off, n_zero=n)
    return out, lw
