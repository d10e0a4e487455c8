"""Sequential Monte Carlo combinators.

Part 1 restates src/genjax/_src/inference/smc.py: ParticleCollection :76-109,
SMCAlgorithm :117-225, Importance :233-279, ImportanceK :282-351,
ChangeTarget :359-465 — same key plumbing, same weight algebra — with the
`jax.vmap` over particles replaced by one fused launch per GFI call.

Part 2 is BUILD-DEFINED (the reference has no resampling strategies, no
extend step, no MH accept: SURVEY.md §0, App. B): scalable resampling
(systematic / stratified / multinomial over an exact integer CDF), a bootstrap
`extend`, an MH `rejuvenate`, and `BootstrapSweep`, the graph-captured
particle-filter sweep bench.py times.  PARITY UNPINNED against the reference
for Part 2; pinned against oracle/ and closed-form Kalman answers.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict, namedtuple
from ctypes import c_uint32

import numpy as np
import torch

from .. import _lib, engine
from ..core.choice_map import ChoiceMap
from ..core.generative import Diff
from ..engine import Gathered
from ..random import Key, fold_in, lazy_split, split
from ..static import DistributionTrace, StaticTrace, VmapTrace
from .sp import Algorithm, Target


# the float algebra between launches, as traced one-launch programs (engine.elementwise)
def _sub(a, b): return a - b
def _add(a, b): return a + b
def _sub_const(a, c): return a - c
def _reweight(new_w, old_score, w): return new_w - old_score + w      # smc.py:383


# ---------------------------------------------------------------------------
# helpers over batched traces
# ---------------------------------------------------------------------------
def trace_map(tr, fn):
    """Apply fn to every device leaf of a (batched) trace."""
    def leaf(v):
        if isinstance(v, (torch.Tensor, Gathered)):
            return fn(v)
        if isinstance(v, tuple):
            return tuple(leaf(x) for x in v)
        if isinstance(v, list):
            return [leaf(x) for x in v]
        if isinstance(v, dict):
            return {k: leaf(x) for k, x in v.items()}
        return v
    if isinstance(tr, DistributionTrace):
        return DistributionTrace(tr.gen_fn, leaf(tr.args), leaf(engine.materialize(tr.value)), leaf(engine.materialize(tr.score)))
    if isinstance(tr, VmapTrace):          # a plate / scan among the particle's sites: its own score and return value too
        return VmapTrace(tr.gen_fn, trace_map(tr.inner, fn), leaf(engine.materialize(tr.score)),
                         leaf(_materialize_tree(tr.retval)), leaf(tr.args))
    return StaticTrace(tr.gen_fn, leaf(tr.args), leaf(_materialize_tree(tr.retval)),
                       OrderedDict((a, trace_map(s, fn)) for a, s in tr.subtraces.items()))


def _materialize_tree(v):
    from ..static import _tree_materialize
    return _tree_materialize(v)


def stack_traces(trs, tr_one, axis: int = 0):
    """tree_map(stack_to_first_dim, trs, tr_one) (smc.py:56-68, :343-345): append ONE trace after the K-1 particles
    of a batched trace along the particle axis — axis 0 for one key, axis `len(key.shape)` under a batch of keys
    (the reference's `vmap` of run_csmc: leaves [*keys, K-1, ...] and [*keys, ...])."""
    def cat(a, b):
        a = engine.materialize(a)
        b = engine.materialize(b)
        if not isinstance(a, torch.Tensor):
            return a                                   # static argument (same in both traces)
        # (a retained trace built from HOST tensors joins device-resident particles: same device, same element type)
        b = torch.as_tensor(b, dtype=a.dtype, device=a.device) if not isinstance(b, torch.Tensor) else b.to(device=a.device, dtype=a.dtype)
        if a.ndim <= axis:
            return a                                   # a launch-uniform leaf (the same in both traces)
        return torch.cat([a, b.reshape(tuple(a.shape[:axis]) + (1,) + tuple(a.shape[axis + 1:]))], dim=axis)

    def leaf(a, b):
        if isinstance(a, (torch.Tensor, Gathered)):
            return cat(a, b)
        if isinstance(a, (tuple, list)):
            return type(a)(leaf(x, y) for x, y in zip(a, b))
        if isinstance(a, dict):
            return {k: leaf(a[k], b[k]) for k in a}
        return a
    if isinstance(trs, DistributionTrace):
        return DistributionTrace(trs.gen_fn, leaf(trs.args, tr_one.args), leaf(trs.value, tr_one.value),
                                 leaf(trs.score, tr_one.score))
    if isinstance(trs, VmapTrace):
        return VmapTrace(trs.gen_fn, stack_traces(trs.inner, tr_one.inner, axis), leaf(engine.materialize(trs.score), tr_one.score),
                         leaf(_materialize_tree(trs.retval), tr_one.retval), leaf(trs.args, tr_one.args))
    return StaticTrace(trs.gen_fn, leaf(trs.args, tr_one.args), leaf(trs.retval, tr_one.retval),
                       OrderedDict((a, stack_traces(s, tr_one.subtraces[a], axis)) for a, s in trs.subtraces.items()))


def trace_leaves(tr) -> list:
    out = []
    trace_map(tr, lambda v: (out.append(v), v)[1])
    return out


# ---------------------------------------------------------------------------
# Part 1: the reference's combinators
# ---------------------------------------------------------------------------
class ParticleCollection:
    """A weighted collection of particles (smc.py:76-109): `particles` is ONE
    batched trace (struct-of-arrays), `log_weights` has the same batch shape.
    `log_ml_offset` (build addition) carries the evidence accumulated by
    earlier resampling steps; it is 0 for the reference's algorithms."""

    def __init__(self, particles, log_weights, is_valid=True, log_ml_offset=None, n_zero=None):
        """log_weights: a tensor, or None with n_zero = N for "all zero" (a freshly resampled collection): the zeros
        are only materialised if somebody asks for them, and `extend` then adds nothing."""
        self.particles, self._lw, self.is_valid = particles, log_weights, is_valid
        self._n_zero = n_zero
        self.log_ml_offset = log_ml_offset

    @property
    def log_weights(self):
        if self._lw is None:
            shape = tuple(self._n_zero) if isinstance(self._n_zero, (tuple, list)) else (self._n_zero,)      # (a batched collection: [R, n])
            self._lw = torch.zeros(shape, dtype=torch.float32, device=_lib.get().device)
        return self._lw

    @log_weights.setter
    def log_weights(self, v):
        self._lw = v

    def weights_are_zero(self) -> bool:
        return self._lw is None

    def get_particles(self):
        return self.particles

    def get_log_weights(self):
        return self.log_weights

    def get_particle(self, idx):
        return trace_map(self.particles, lambda v: engine.materialize(v)[idx])

    def __getitem__(self, idx):
        return self.get_particle(idx), self.log_weights[idx]

    def get_log_marginal_likelihood_estimate(self):
        """logsumexp(lw) - log N (smc.py:96-97) [+ accumulated offset]; a batched collection: the per-row estimate."""
        n = self.log_weights.shape[-1]
        est = engine.elementwise(_sub_const, engine.logsumexp_rows(self.log_weights), math.log(n))
        if self.log_ml_offset is not None:
            off = self.log_ml_offset.value()
            if isinstance(off, np.ndarray):        # one offset per row: added in float32, as the 1-D path adds its one
                off = torch.from_numpy(off.astype(np.float32)).to(est.device).reshape(est.shape)
            est = engine.elementwise(_add, est, off)
        return est

    def sample_index(self, key: Key):
        """Categorical draw proportional to the weights (smc.py:102-108): Gumbel-max
        over logits = lw - logsumexp(lw), gumbel counter = particle index."""
        lw = self.log_weights
        lse = engine.logsumexp_rows(lw)
        logits = engine.elementwise(_sub, lw, lse) if lw.ndim > 1 else engine.elementwise(_sub, lw, lse.reshape(()))
        return engine.categorical_rows(key, logits)

    def sample_particle(self, key: Key):
        idx = self.sample_index(key)
        nb = self.log_weights.ndim

        def take(v):
            v = engine.materialize(v)
            if v.ndim < nb:
                return v
            ix = idx.long().reshape(idx.shape + (1,) * (v.ndim - nb + 1))
            ix = ix.expand(idx.shape + (1,) + tuple(v.shape[nb:]))
            return torch.gather(v, nb - 1, ix).squeeze(nb - 1)
        return trace_map(self.particles, take)


class SMCAlgorithm(Algorithm):
    """smc.py:117-225"""

    def get_num_particles(self): raise NotImplementedError
    def get_final_target(self): raise NotImplementedError
    def run_smc(self, key): raise NotImplementedError

    def run_csmc(self, key, retained): raise NotImplementedError

    def log_marginal_likelihood_estimate(self, key, target=None):
        algorithm = ChangeTarget(self, target) if target else self       # smc.py:150-153
        key, sub_key = split(key)
        return algorithm.run_smc(sub_key).get_log_marginal_likelihood_estimate()

    def random_weighted(self, key, *args):
        """smc.py:162-179"""
        target = args[0]
        assert isinstance(target, Target)
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        collection = algorithm.run_smc(key)
        particle = collection.sample_particle(sub_key)
        estimate = engine.elementwise(_sub, particle.get_score(), collection.get_log_marginal_likelihood_estimate())
        chm = target.filter_to_unconstrained(particle.get_choices())
        return estimate, chm

    def estimate_logpdf(self, key, v, *args):
        """smc.py:181-198: conditional SMC with `v` retained in the last slot."""
        target = args[0]
        assert isinstance(target, Target)
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        collection = algorithm.run_csmc(key, v)
        particle = collection.sample_particle(sub_key)
        return engine.elementwise(_sub, particle.get_score(), collection.get_log_marginal_likelihood_estimate())

    def estimate_normalizing_constant(self, key, target):
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        return algorithm.run_smc(sub_key).get_log_marginal_likelihood_estimate()

    def estimate_reciprocal_normalizing_constant(self, key, target, latent_choices, w):
        """smc.py:214-225: `w` (with `latent_choices`) is already properly weighted for `target`, so the
        conditional run skips the redundant re-weighting of the retained particle."""
        return ChangeTarget(self, target).run_csmc_for_normalizing_constant(key, latent_choices, w)


class Importance(SMCAlgorithm):
    """One-particle importance sampling (smc.py:233-266): the particle is
    generated with `key` itself (child 0 of the split)."""

    def __init__(self, target: Target, q=None):
        self.target, self.q = target, q

    def get_num_particles(self): return 1
    def get_final_target(self): return self.target

    def run_smc(self, key):
        key, sub_key = split(key)
        k1 = key.reshape(tuple(key.shape) + (1,))
        if self.q is not None:                                           # smc.py:256-258
            log_weight, choice = self.q.random_weighted(sub_key, self.target)
            tr, score = self.target.importance(k1, _expand(choice))
            return ParticleCollection(tr, engine.elementwise(_sub, score, _expand_leaf(log_weight)), True)
        tr, score = self.target.importance(k1, ChoiceMap.empty())
        return ParticleCollection(tr, score, True)

    def run_csmc(self, key, retained):
        """smc.py:268-279"""
        nb = len(key.shape)                  # a batch of keys (the reference's vmap of run_csmc): particle axis nb
        key, sub_key = split(key)
        q_score = self.q.estimate_logpdf(sub_key, retained, self.target) if self.q is not None else 0.0
        k1 = key.reshape(tuple(key.shape) + (1,))
        tgt = _target_over(self.target, key.shape, 1)
        tr, score = tgt.importance(k1, _expand(retained, nb))
        return ParticleCollection(tr, engine.elementwise(_sub, score, _expand_leaf(q_score, nb)), True)


class ImportanceK(SMCAlgorithm):
    """K-particle importance sampling (smc.py:282-315):
    key, sub = split(key); keys = split(sub, K); one fused launch over K."""

    def __init__(self, target: Target, q=None, k_particles: int = 2):
        self.target, self.q, self.k_particles = target, q, int(k_particles)

    def get_num_particles(self): return self.k_particles
    def get_final_target(self): return self.target

    def run_smc(self, key):
        key, sub_key = split(key)
        sub_keys = split(sub_key, self.k_particles)
        if self.q is not None:                                           # smc.py:301-305
            log_weights, choices = self.q.random_weighted(sub_keys, self.target)
            trs, target_scores = self.target.importance(sub_keys, choices)
            return ParticleCollection(trs, engine.elementwise(_sub, target_scores, log_weights), True)
        trs, target_scores = self.target.importance(sub_keys, ChoiceMap.empty())
        return ParticleCollection(trs, target_scores, True)         # log_weights = scores - 0.0

    def run_csmc(self, key, retained):
        """smc.py:317-351: K-1 fresh particles, the retained choices in slot K-1."""
        K = self.k_particles
        nb = len(key.shape)                  # under a batch of keys everything gains the leading key axes: ONE launch
        key, sub_key = split(key)            # set over [*keys, K] with the retained particle in slot K-1 of every row
        sub_keys = split(sub_key, K - 1)
        tgt_k1 = _target_over(self.target, key.shape, K - 1)
        if self.q is not None:
            log_scores, choices = self.q.random_weighted(sub_keys, tgt_k1)
            retained_score = self.q.estimate_logpdf(key, retained, self.target)
            stacked = _stack_chm(choices, retained, nb)
            stacked_scores = torch.cat([log_scores, _expand_leaf(retained_score, nb).to(log_scores.device)], dim=nb)
            trs, target_scores = _target_over(self.target, key.shape, K).importance(split(key, K), stacked)
            return ParticleCollection(trs, engine.elementwise(_sub, target_scores, stacked_scores), True)
        ignored, ignored_scores = tgt_k1.importance(sub_keys, ChoiceMap.empty())
        retained_tr, retained_score = self.target.importance(key, retained)
        scores = torch.cat([ignored_scores, retained_score.reshape(tuple(ignored_scores.shape[:nb]) + (1,))], dim=nb)
        return ParticleCollection(stack_traces(ignored, retained_tr, nb), scores, True)


class ChangeTarget(SMCAlgorithm):
    """Re-weight every particle for a new target (smc.py:359-396); the incoming
    key is used both for prev.run_smc(key) and for split(key, K) (:374, :386)."""

    def __init__(self, prev: SMCAlgorithm, target: Target):
        self.prev, self.target = prev, target

    def get_num_particles(self): return self.prev.get_num_particles()
    def get_final_target(self): return self.target

    def run_smc(self, key):
        collection = self.prev.run_smc(key)
        particles = collection.get_particles()
        latents = self.prev.get_final_target().filter_to_unconstrained(particles.get_choices())
        sub_keys = split(key, self.get_num_particles())
        tgt = _target_over(self.target, key.shape, self.get_num_particles())
        new_particles, new_weight = tgt.importance(sub_keys, latents)
        this_weight = engine.elementwise(_reweight, new_weight, particles.get_score(), collection.get_log_weights())   # smc.py:383
        return ParticleCollection(new_particles, this_weight, True, collection.log_ml_offset)

    def run_csmc(self, key, retained):
        """smc.py:398-425: prev.run_csmc(key, retained), then the same re-weighting."""
        collection = self.prev.run_csmc(key, retained)
        particles = collection.get_particles()
        latents = self.prev.get_final_target().filter_to_unconstrained(particles.get_choices())
        sub_keys = split(key, self.get_num_particles())
        tgt = _target_over(self.target, key.shape, self.get_num_particles())
        new_particles, new_score = tgt.importance(sub_keys, latents)
        this_weight = engine.elementwise(_reweight, new_score, particles.get_score(), collection.get_log_weights())
        return ParticleCollection(new_particles, this_weight, True)

    def run_csmc_for_normalizing_constant(self, key, latent_choices, w):
        return _csmc_normalizing_constant(self, key, latent_choices, w)


def _csmc_normalizing_constant(self, key, latent_choices, w):
    """ChangeTarget.run_csmc_for_normalizing_constant (smc.py:432-465): conditional SMC under the previous
    target with `latent_choices` retained in slot K-1; the K-1 rejected particles are re-weighted for the new
    target (keys split(key, K-1)), the retained one takes `w - retained_score + retained_weight`;
    returns retained_score - (logsumexp(all weights) - log K)."""
    nb = len(key.shape)                  # a batch of keys: every row of [*keys, K] is one conditional run
    key, sub_key = split(key)
    collection = self.prev.run_csmc(sub_key, latent_choices)
    K = self.get_num_particles()
    particles, lw = collection.get_particles(), collection.get_log_weights()
    scores = particles.get_score()
    last_i = (slice(None),) * nb + (-1,)
    head_i = (slice(None),) * nb + (slice(None, -1),)
    retained_score, retained_weight = scores[last_i], lw[last_i]
    be = _lib.get()
    w_t = w if isinstance(w, torch.Tensor) else torch.tensor(float(w), dtype=torch.float32, device=be.device)
    one = tuple(retained_score.shape) + (1,)
    last = engine.elementwise(_reweight, w_t.to(be.device).expand(retained_score.shape).reshape(one).contiguous(),
                              retained_score.reshape(one).contiguous(), retained_weight.reshape(one).contiguous())
    if K > 1:
        head = trace_map(particles, lambda v: engine.materialize(v)[head_i].contiguous()
                         if tuple(v.shape[nb:nb + 1]) == (K,) else v)
        latents = self.prev.get_final_target().filter_to_unconstrained(head.get_choices())
        _, new_score = _target_over(self.target, key.shape, K - 1).importance(split(key, K - 1), latents)
        rejected = engine.elementwise(_reweight, new_score, scores[head_i].contiguous(), lw[head_i].contiguous())
        all_weights = torch.cat([rejected.reshape(one[:-1] + (K - 1,)), last.reshape(one)], dim=nb)
    else:
        all_weights = last.reshape(one)
    total = engine.logsumexp_rows(all_weights)
    out = engine.elementwise(_recip_z, retained_score.reshape(one).contiguous(), total.reshape(one).contiguous(), math.log(K))
    return out.reshape(tuple(retained_score.shape))


def _recip_z(retained_score, total, log_k): return retained_score - (total - log_k)


def _unbatched(key: Key, who: str):
    if tuple(key.shape) != ():
        raise NotImplementedError(f"{who} under a batch of keys")


def _expand_leaf(v, nb: int = 0):
    """jnp.expand_dims(v, nb) for a score (tensor or Python number): the one-particle axis after `nb` key axes."""
    be = _lib.get()
    t = v if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float32, device=be.device)
    return t.reshape(tuple(t.shape[:nb]) + (1,) + tuple(t.shape[nb:]))


def _expand(chm: ChoiceMap, nb: int = 0) -> ChoiceMap:
    """A one-particle batch of a choice map (its values carry `nb` leading key axes)."""
    be = _lib.get()

    def one(v):
        t = torch.as_tensor(v, device=be.device) if not isinstance(v, torch.Tensor) else v
        if t.dtype == torch.float64:
            t = t.float()
        return t.reshape(tuple(t.shape[:nb]) + (1,) + tuple(t.shape[nb:]))
    return chm.map_values(one)


def _stack_chm(choices: ChoiceMap, one: ChoiceMap, nb: int = 0) -> ChoiceMap:
    """tree_map(stack_to_first_dim, choices, retained) over choice maps with the same addresses (particle axis nb)."""
    out = ChoiceMap.empty()
    for a in choices.addresses():
        v = engine.materialize(choices[a])
        r = torch.as_tensor(one[a], dtype=v.dtype, device=v.device).reshape(tuple(v.shape[:nb]) + (1,) + tuple(v.shape[nb + 1:]))
        out = out.set(a, torch.cat([v, r], dim=nb))
    return out


def _target_over(target: Target, batch: tuple, k: int) -> Target:
    """Under a batch of keys a Target's own observations may be batched over the keys too ([*keys, ...]: a nested
    Marginal's latent choices, one set per key): for a launch over [*keys, k] particles they are repeated along the
    particle axis.  One key, or launch-uniform observations (leading shape != the key batch): left alone."""
    batch = tuple(batch)
    nb = len(batch)
    if nb == 0:
        return target

    def rep(v):
        if isinstance(v, torch.Tensor) and tuple(v.shape[:nb]) == batch:
            return v.unsqueeze(nb).expand(batch + (k,) + tuple(v.shape[nb:])).contiguous()
        return v
    return Target(target.p, tuple(rep(a) for a in target.args), target.constraint.map_values(rep))


# ---------------------------------------------------------------------------
# Part 2: build-defined scalable SMC moves
# ---------------------------------------------------------------------------
MULTINOMIAL_GUIDED_MIN = 8192      # below this the per-slot search of gmx_ancestors is as fast as building a guide table
SYSTEMATIC, STRATIFIED, MULTINOMIAL = (_lib.RESAMPLE_SYSTEMATIC, _lib.RESAMPLE_STRATIFIED,
                                       _lib.RESAMPLE_MULTINOMIAL)
# two-stage multinomial (gmx_multinomial_tiled): the same offspring law, the output ordered by the ancestor's CDF tile
MULTINOMIAL_TILED = _lib.RESAMPLE_MULTINOMIAL_TILED
# multinomial with SORTED uniforms (gmx_resample_sorted): the same offspring law, the output ordered by ancestor — an
# ordered scheme on the systematic resampler's kernel; its order-statistics table comes from the background stream
MULTINOMIAL_SORTED = _lib.RESAMPLE_MULTINOMIAL_SORTED
_KINDS = {"systematic": SYSTEMATIC, "stratified": STRATIFIED, "multinomial": MULTINOMIAL,
          "multinomial_tiled": MULTINOMIAL_TILED, "multinomial_sorted": MULTINOMIAL_SORTED}
_TILE_KINDS = (SYSTEMATIC, STRATIFIED, MULTINOMIAL_TILED, MULTINOMIAL_SORTED)      # from log-weights + tile statistics, n <= 2^21


def cdf_reference(m):
    """The log-weight an integer CDF total is relative to: total * 2^-shift = sum_i exp(lw_i - cdf_reference(max lw)).
    = ceil(max lw / ln 2) * ln 2 in float32 arithmetic (gmx_tile_exp / gmx_tile_ref in csrc/gmx_math.h: the
    exponent K of the block-floating-point CDF), evaluated on the host for the evidence terms.  A float for one maximum;
    a float64 array for an array of them (one per row of gmx_resample_rows)."""
    lim = np.float32(1 << 29)
    inv_ln2 = np.frombuffer(np.uint32(0x3FB8AA3B).tobytes(), np.float32)[0]
    ln2 = np.frombuffer(np.uint32(0x3F317218).tobytes(), np.float32)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(m, dtype=np.float32) * inv_ln2
        k = np.ceil(np.clip(np.where(t > -lim, t, -lim), -lim, lim))      # (NaN: the lower clamp, as the kernels')
    ref = (k.astype(np.float32) * ln2).astype(np.float64)
    return ref if np.ndim(m) > 0 else float(ref)


def evidence_terms(maxs, totals, shift, n):
    """The evidence a resampling step contributes, ref(M) + log(total) - shift ln 2 - log n in float64, -inf where the
    total is 0 (no particle carried any mass): an array for arrays of maxima and totals (the totals as the int64 words the
    kernels leave: read as uint64), a float for one maximum and one Python-integer total.

    The callers sum the terms, each in its own order, and the last bit of a sum depends on it: np.sum over the T
    contiguous terms of a sweep (BootstrapSweep.log_ml; BootstrapBank.log_ml per row), a sequential `acc +=` over the
    steps in LogMLOffset.value and ShardedBootstrapSweep.log_ml.  The sequential callers hand over one step at a time
    and get math.log of the integer; the array callers get np.log — the two differ in the last bit for about 2 totals
    in 100 000, so neither caller can take the other's."""
    ref = cdf_reference(maxs)
    if np.ndim(totals) == 0:
        tot = int(totals) & 0xFFFFFFFFFFFFFFFF
        return ref + math.log(tot) - shift * math.log(2.0) - math.log(n) if tot else -math.inf
    tot = np.asarray(totals).view(np.uint64).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(tot == 0, -np.inf, ref + np.log(tot) - shift * math.log(2.0) - math.log(n))


def cdf_shift(n_total: int) -> int:
    """Fixed-point exponent: a sum of n_total terms <= 2^shift stays below 2^62."""
    need = 0
    while (1 << need) < n_total:
        need += 1
    return 62 - need


class LogMLOffset:
    """Evidence accumulated by resampling steps, kept on the device as exact
    integers and finished in float64 on the host when asked:
      sum_t [ M_t + log(total_t * 2^-shift) - log N ]."""

    def __init__(self, terms=()):
        self.terms = list(terms)      # (max_d f32[1], total_d u64-as-i64[1], shift, n); a batched collection: [R] each

    def plus(self, max_d, total_d, shift, n):
        return LogMLOffset(self.terms + [(max_d, total_d, shift, n)])

    def value(self):
        """a float; with [R] terms (smc.resample on a batched collection) float64 [R], row r the float the same terms of
        row r alone give"""
        if any(max_d.numel() > 1 for max_d, _, _, _ in self.terms):
            ms = [max_d.reshape(-1).cpu().numpy() for max_d, _, _, _ in self.terms]
            tots = [total_d.reshape(-1).cpu().numpy().view(np.uint64) for _, total_d, _, _ in self.terms]
            out = np.zeros((max(m.size for m in ms),), dtype=np.float64)
            for r in range(out.size):
                for m, tot, (_, _, shift, n) in zip(ms, tots, self.terms):
                    out[r] += evidence_terms(m[r % m.size], int(tot[r % tot.size]), shift, n)
                    if out[r] == -math.inf:      # no particle of the row carried any mass
                        break
            return out
        acc = 0.0
        for max_d, total_d, shift, n in self.terms:
            acc += evidence_terms(max_d.reshape(-1)[0].item(), total_d.reshape(-1)[0].item(), shift, n)
            if acc == -math.inf:         # no particle carried any mass: the evidence estimate is 0
                break
        return acc


def _key_words(key: Key):
    """ONE key as the `const uint32_t key[2]` argument of the C-ABI"""
    kh = key.host()
    return (c_uint32 * 2)(int(kh[0]), int(kh[1]))


def weight_cdf(lw: torch.Tensor, n_total=None, max_partials=None):
    """gmx_weight_cdf: returns (cdf int64-bits [n], total [1], max [1], shift)."""
    be = _lib.get()
    lw = lw.reshape(-1)
    if lw.dtype != torch.float32:
        lw = lw.float()
    lw = lw.contiguous()
    n = lw.numel()
    shift = cdf_shift(n if n_total is None else n_total)
    cdf = torch.empty((n,), dtype=torch.int64, device=lw.device)
    total = torch.empty((1,), dtype=torch.int64, device=lw.device)
    mx = torch.empty((1,), dtype=torch.float32, device=lw.device)
    ws = torch.zeros(((be.c.gmx_weight_cdf_workspace(n) + 7) // 8,), dtype=torch.int64, device=lw.device)
    partials, rows = None, 0
    if max_partials is None:
        # max via the deterministic LSE kernel's max output
        rows_ws = torch.empty(((be.c.gmx_logsumexp_workspace(1, n) + 3) // 4,), dtype=torch.int32, device=lw.device)
        dummy = torch.empty((1,), dtype=torch.float32, device=lw.device)
        be.check(be.c.gmx_logsumexp(be.ptr(lw), 1, n, be.ptr(dummy), be.ptr(mx), be.ptr(rows_ws), be.stream()),
                 "gmx_logsumexp")
    else:
        partials, rows = be.ptr(max_partials), max_partials.shape[-1]
    be.check(be.c.gmx_weight_cdf(be.ptr(lw), n, shift, partials, rows, be.ptr(mx), be.ptr(cdf), be.ptr(total), be.ptr(ws),
                                 be.stream()), "gmx_weight_cdf")
    return cdf, total, mx, shift


FUSE_RESAMPLE_MAX = 1 << 20      # the resample-first launch: all its workgroups resident at once (1024 tiles)
FUSE_RESAMPLE_LOOP_MAX = 1 << 24 # ... or, LOOPED, 1024 workgroups walking up to 16 tiles each (engine.Compiled.set_fuse_resample(loop=True))
FUSED_RESAMPLE_MAX = 2048 * 1024        # RS_MAX_TILES tiles of 1024 particles (csrc/gmx_kernels.hip)


class _Resampler:
    """THE place that launches a resampler: picks the form for (kind, n, n_out) once, owns that form's workspaces
    (allocated here, never in `launch`), and issues the form's C calls.

      "tiles"   n <= FUSED_RESAMPLE_MAX, no CDF array: the kind's tile-form entry point from the (tile maxima, tile sums)
                statistics a site program or gmx_tile_stats left; systematic / stratified without statistics: gmx_resample
      "prefix"  past FUSED_RESAMPLE_MAX (BASELINE config 4: k = 1e7), still no CDF array: gmx_tile_prefix (the tile
                prefixes from one workgroup) + gmx_resample_tiles_p / gmx_resample_sorted_p; one-off calls only
      "cdf"     gmx_weight_cdf into the CDF array + gmx_ancestors, or gmx_multinomial (the guide table) for the iid
                multinomial from MULTINOMIAL_GUIDED_MIN particles on

    sweep=True: a BootstrapSweep's launcher (persistent buffers; past FUSED_RESAMPLE_MAX it takes the CDF array).
    with_stats=True: the caller brings statistics to every launch (no gmx_resample workspace)."""

    @staticmethod
    def fused_form(kind, n):
        """which of the two forms without a CDF array resample_fused takes (their entry points refuse what they cannot)"""
        return "prefix" if n > FUSED_RESAMPLE_MAX and kind != MULTINOMIAL_TILED else "tiles"

    @staticmethod
    def form_of(kind, n, n_out=None, sweep=False):
        """the form for this kind and size: "tiles" / "prefix" where that form takes them, else the CDF array — which the
        two ordered multinomials do not have: NotImplementedError"""
        form = _Resampler.fused_form(kind, n)
        if kind in _TILE_KINDS and n_out in (None, n) and \
                (0 < n <= FUSED_RESAMPLE_MAX if form == "tiles" else (not sweep and n < 2 ** 31 - 8192)):
            return form
        if kind in (MULTINOMIAL_TILED, MULTINOMIAL_SORTED):
            if sweep:
                raise NotImplementedError("resample='multinomial_tiled' / 'multinomial_sorted': n <= 2^21 per GPU (use 'multinomial')")
            raise NotImplementedError("resample(kind='multinomial_tiled'): n_out = n <= 2^21; 'multinomial_sorted': n_out = n "
                                      "(use 'multinomial')")
        return "cdf"

    @staticmethod
    def needs_stats(kind, form):
        """forms that only run from tile statistics (the others can do without: gmx_resample, the CDF array)"""
        return form == "prefix" or (form == "tiles" and kind in (MULTINOMIAL_TILED, MULTINOMIAL_SORTED))

    def __init__(self, kind, n, n_out=None, *, form=None, sweep=False, with_stats=False, cdf=None):
        """cdf: a ready CDF array ("cdf" form: ancestors_from_cdf) instead of one of the launcher's own"""
        be = _lib.get()
        dev = be.device
        self.kind, self.n, self.n_out = int(kind), int(n), int(n if n_out is None else n_out)
        self.form = form or self.form_of(self.kind, self.n, n_out, sweep)
        self.shift = cdf_shift(self.n)
        fresh = torch.zeros if sweep else torch.empty      # (a one-off call's workspaces are written before they are read)

        def words(nbytes, dtype, alloc=fresh):
            size = torch.empty((), dtype=dtype).element_size()
            return alloc(((int(nbytes) + size - 1) // size,), dtype=dtype, device=dev)
        self.cdf = self.cdf_ws = self.ws = self.table = self.prefix = None
        if self.form == "cdf":
            self.cdf = torch.zeros((self.n,), dtype=torch.int64, device=dev) if cdf is None else cdf
        if sweep or (self.form == "cdf" and cdf is None):
            # (a sweep keeps gmx_weight_cdf's workspace in every form: its spin-bound word is part of what a sweep shows)
            self.cdf_ws = words(be.c.gmx_weight_cdf_workspace(self.n), torch.int64, torch.zeros)
        self.guided = self.form == "cdf" and self.kind == MULTINOMIAL and self.n >= MULTINOMIAL_GUIDED_MIN
        if self.guided:
            self.ws = words(be.c.gmx_multinomial_workspace(self.n), torch.int32)
        elif self.form == "tiles" and self.kind == MULTINOMIAL_TILED:
            self.ws = words(be.c.gmx_multinomial_tiled_workspace(self.n), torch.int32, torch.zeros)     # the count buffers
        elif self.form == "tiles" and self.kind != MULTINOMIAL_SORTED and not with_stats:
            self.ws = words(be.c.gmx_resample_workspace(self.n), torch.int64)
        if self.kind == MULTINOMIAL_SORTED and self.form != "cdf":
            self.table = words(4 * int(be.c.gmx_sorted_uniforms_words(self.n)), torch.int32)
        if self.form == "prefix":
            self.prefix = words(8 * int(be.c.gmx_tile_prefix_words(self.n)), torch.int64)

    def launch(self, key, lw, max_out, total_out, anc, *, stats=None, uniforms=None, partials=None, rows=0, phase=-1,
               cdf_ready=False):
        """Resample `lw` under `key`: the global max, the integer total and the ancestors into max_out / total_out / anc.

        stats     (tile maxima, tile sums) of lw, where they exist
        uniforms  drawn ahead from the key alone (the noise-ahead sweep): the stratified / two-stage multinomial slot
                  uniforms, or the sorted multinomial's ready order-statistics table
        partials, rows   block maxima of lw for gmx_resample / gmx_weight_cdf (without: they take a pass of their own)
        phase     gmx_multinomial_tiled: which count buffer is zero (-1: neither, the call clears both)
        "cdf" form: anc=None stops after the CDF array; cdf_ready=True starts from it (total_out then holds its total)"""
        be = _lib.get()
        c, P, n, st = be.c, be.ptr, self.n, be.stream()
        kk, shift = _key_words(key), self.shift
        tile_max, tile_agg = (P(stats[0]), P(stats[1])) if stats is not None else (None, None)
        if self.form == "cdf":
            if not cdf_ready:
                be.check(c.gmx_weight_cdf(P(lw), n, shift, P(partials), rows, P(max_out), P(self.cdf), P(total_out),
                                          P(self.cdf_ws), st), "gmx_weight_cdf")
            if anc is None:
                pass
            elif self.guided:
                # unordered slots: through the guide table (two table reads + a search over ~3 entries per slot instead
                # of a binary search over n) — the same ancestors
                be.check(c.gmx_multinomial(kk, P(self.cdf), n, P(total_out), self.n_out, P(anc), P(self.ws), st),
                         "gmx_multinomial")
            else:
                be.check(c.gmx_ancestors(self.kind, kk, P(self.cdf), n, 0, P(total_out), self.n_out, 0, self.n_out, P(anc),
                                         st), "gmx_ancestors")
        elif self.form == "prefix":
            be.check(c.gmx_tile_prefix(tile_max, tile_agg, n, P(self.prefix), st), "gmx_tile_prefix")
            if self.kind == MULTINOMIAL_SORTED:
                be.check(c.gmx_resample_sorted_p(kk, P(lw), n, shift, tile_max, P(self.prefix), P(self.table), 0, P(max_out),
                                                 P(total_out), P(anc), st), "gmx_resample_sorted_p")
            else:
                be.check(c.gmx_resample_tiles_p(self.kind, kk, P(lw), n, shift, tile_max, P(self.prefix), P(max_out),
                                                P(total_out), P(anc), st), "gmx_resample_tiles_p")
        elif self.kind == MULTINOMIAL_TILED:
            be.check(c.gmx_multinomial_tiled(kk, P(lw), n, shift, tile_max, tile_agg, P(uniforms), P(max_out), P(total_out),
                                             P(anc), P(self.ws), phase, st), "gmx_multinomial_tiled")
        elif self.kind == MULTINOMIAL_SORTED:
            table, ready = (self.table, 0) if uniforms is None else (uniforms, 1)
            be.check(c.gmx_resample_sorted(kk, P(lw), n, shift, tile_max, tile_agg, P(table), ready, P(max_out),
                                           P(total_out), P(anc), st), "gmx_resample_sorted")
        elif uniforms is not None:
            be.check(c.gmx_resample_tiles_u(self.kind, kk, P(lw), n, shift, tile_max, tile_agg, P(uniforms), P(max_out),
                                            P(total_out), P(anc), st), "gmx_resample_tiles_u")
        elif stats is not None:        # (in a sweep: tile maxima = the workgroup maxima the site program left)
            be.check(c.gmx_resample_tiles(self.kind, kk, P(lw), n, shift, tile_max, tile_agg, P(max_out), P(total_out),
                                          P(anc), st), "gmx_resample_tiles")
        else:
            be.check(c.gmx_resample(self.kind, kk, P(lw), n, shift, P(partials), rows, P(max_out), P(total_out), P(anc),
                                    P(self.ws), st), "gmx_resample")


def _tile_stats(lw, shift, tile_max, tile_agg):
    """gmx_tile_stats: the CDF tile statistics of log-weights no site program left them for"""
    be = _lib.get()
    be.check(be.c.gmx_tile_stats(be.ptr(lw), lw.numel(), shift, be.ptr(tile_max), be.ptr(tile_agg), be.stream()),
             "gmx_tile_stats")


def resample_fused(kind, key: Key, lw: torch.Tensor):
    """gmx_resample: log-weights -> (ancestors int32 [n], total [1], max [1], shift) in two launches with no CDF
    array (tile statistics + k_offspring_tile); the same integers as weight_cdf + ancestors_from_cdf."""
    stats = getattr(lw, "_gmx_tile_stats", None)       # left by the program that computed these weights (run_gfi)
    if stats is not None and (len(stats) < 5 or stats[4] != lw._version):
        stats = None                       # the weights were changed in place since: the statistics are stale
    lw = lw.reshape(-1).float().contiguous()
    if lw.data_ptr() % 16:
        lw = lw.clone()                    # a view into the middle of a buffer: the kernels load float4
        stats = None
    n = lw.numel()
    shift = cdf_shift(n)
    if stats is not None and not (stats[2] == shift and stats[3] == n):
        stats = None
    anc = torch.empty((n,), dtype=torch.int32, device=lw.device)
    total = torch.empty((1,), dtype=torch.int64, device=lw.device)
    mx = torch.empty((1,), dtype=torch.float32, device=lw.device)
    form = _Resampler.fused_form(int(kind), n)
    if stats is None and _Resampler.needs_stats(int(kind), form):
        tiles = (n + 1023) // 1024
        stats = (torch.empty((tiles,), dtype=torch.float32, device=lw.device),
                 torch.empty((tiles,), dtype=torch.int64, device=lw.device))
        _tile_stats(lw, shift, *stats)
    # the two-stage multinomial's count buffers are zeroed HERE (the fill kernel of the launcher's allocation; phase 0:
    # "buffer 0 is zero") rather than by the call's own memset
    # (phase -1): inside `smc.capture` the memset node of a one-off workspace did not hold across replays (replay 0
    # right, every later one wrong: tools/experiments/capture_kinds_dbg.py) — a sweep's persistent workspace is fine
    rs = _Resampler(kind, n, form=form, with_stats=stats is not None)
    rs.launch(key, lw, mx, total, anc, stats=stats and stats[:2], phase=0)
    return anc, total, mx, shift


def ancestors_from_cdf(kind, key: Key, cdf, total, n_out=None) -> torch.Tensor:
    n_in = cdf.numel()
    n_out = n_in if n_out is None else int(n_out)
    anc = torch.empty((n_out,), dtype=torch.int32, device=cdf.device)
    _Resampler(kind, n_in, n_out, form="cdf", cdf=cdf).launch(key, None, None, total, anc, cdf_ready=True)
    return anc


def resample(key: Key, collection: ParticleCollection, kind="systematic", n_out=None) -> ParticleCollection:
    """Resample a 1-D particle collection.  The result's leaves are lazy
    gathers (`engine.Gathered`), so a following `extend` fuses the gather into
    its kernel; weights reset to 0 and the evidence moves into log_ml_offset."""
    lw = collection.get_log_weights()
    if lw.ndim != 1:
        return _resample_batched(key, collection, kind, n_out)
    kind = _KINDS[kind] if isinstance(kind, str) else int(kind)
    n = lw.numel()
    if _Resampler.form_of(kind, n, n_out) != "cdf":
        anc, total, mx, shift = resample_fused(kind, key, lw)        # no CDF in memory (gmx_resample[_tiles[_p]])
    else:
        cdf, total, mx, shift = weight_cdf(lw)
        anc = ancestors_from_cdf(kind, key, cdf, total, n_out)
    particles = trace_map(collection.get_particles(),
                          lambda v: Gathered(engine.materialize(v), anc) if tuple(v.shape[:1]) == (n,) else v)
    off = (collection.log_ml_offset or LogMLOffset()).plus(mx, total, shift, n)
    out = ParticleCollection(particles, None, True, off, n_zero=anc.numel())     # weights reset to 0, lazily
    out.ancestors = anc
    return out


ROW_KINDS = (SYSTEMATIC, STRATIFIED, MULTINOMIAL)      # what gmx_resample_rows takes
ROWS_N_MAX = FUSED_RESAMPLE_MAX
ROWS_ESS_N_MAX = 1024                  # gmx_resample_rows_ess: a row of one CDF tile


def _rows_buffers(be, kind, lw, out, workspace):
    """the out= / workspace= defaults of resample_rows and resample_rows_pinned: fresh (anc, total, max, status) with
    status zeroed, and a fresh workspace of gmx_resample_rows_workspace(kind) bytes"""
    R, n = lw.shape
    if out is None:
        out = (torch.empty((R, n), dtype=torch.int32, device=lw.device), torch.empty((R,), dtype=torch.int64, device=lw.device),
               torch.empty((R,), dtype=torch.float32, device=lw.device), torch.zeros((1,), dtype=torch.int64, device=lw.device))
    if workspace is None:
        workspace = torch.empty(((int(be.c.gmx_resample_rows_workspace(int(kind), R, n)) + 7) // 8,), dtype=torch.int64,
                                device=lw.device)
    return out, workspace


def resample_rows(kind, keys: Key, lw: torch.Tensor, index_stride: int = 0, *, out=None, workspace=None):
    """gmx_resample_rows: R independent rows in one call.  lw [R, n] float32 (contiguous), keys of shape (R,) ->
    (ancestors int32 [R, n] — row-local, or into the flat [R * n] store with index_stride = n —, total [R], max [R],
    shift, status [1]: the number of rows without mass).  out = (anc, total, max, status) and workspace: persistent
    buffers of a sweep instead of fresh ones (status is then NOT zeroed here)."""
    be = _lib.get()
    R, n = lw.shape
    kd = keys if isinstance(keys, torch.Tensor) else keys.data()
    (anc, total, mx, status), workspace = _rows_buffers(be, kind, lw, out, workspace)
    be.check(be.c.gmx_resample_rows(int(kind), be.ptr(kd), be.ptr(lw), R, n, n, int(index_stride), be.ptr(mx), be.ptr(total),
                                    be.ptr(anc), be.ptr(status), be.ptr(workspace), be.stream()), "gmx_resample_rows")
    return anc, total, mx, cdf_shift(n), status


def resample_rows_pinned(keys: Key, lw: torch.Tensor, pin_lw: torch.Tensor, pin_x=None, x=None, index_stride: int = 0,
                         x_row_stride=None, *, out=None, workspace=None):
    """gmx_resample_rows_pinned: the iid multinomial of resample_rows with slot n - 1 of every row pinned (conditional SMC).
    lw [R, n] float32 (contiguous; column n - 1 is OVERWRITTEN with pin_lw [R]), pin_x [D, R] -> column r * x_row_stride +
    n - 1 of every row of the struct-of-arrays store x [D, x_ld] (x_row_stride: n by default; pin_x = x = None: no
    state).  Returns what resample_rows returns; ancestors[r, n - 1] = n - 1 + r * index_stride, the other slots are the
    unconditional draw on the pinned weights, bit for bit."""
    be = _lib.get()
    R, n = lw.shape
    kd = keys if isinstance(keys, torch.Tensor) else keys.data()
    if (pin_x is None) != (x is None):
        raise ValueError("resample_rows_pinned: pin_x and x come together (the retained states and the store they go into)")
    D, x_ld = (0, 0) if x is None else (int(v) for v in x.shape)
    if x is not None and tuple(pin_x.shape) != (D, R):
        raise ValueError(f"resample_rows_pinned: pin_x is [D, R] = {(D, R)} for a store of {D} rows; got {tuple(pin_x.shape)}")
    if tuple(pin_lw.shape) != (R,):
        raise ValueError(f"resample_rows_pinned: pin_lw is [R] = {(R,)}; got {tuple(pin_lw.shape)}")
    (anc, total, mx, status), workspace = _rows_buffers(be, MULTINOMIAL, lw, out, workspace)
    be.check(be.c.gmx_resample_rows_pinned(be.ptr(kd), be.ptr(lw), R, n, n, int(index_stride), be.ptr(pin_lw), be.ptr(pin_x),
                                           be.ptr(x), D, x_ld, n if x_row_stride is None else int(x_row_stride), be.ptr(mx),
                                           be.ptr(total), be.ptr(anc), be.ptr(status), be.ptr(workspace), be.stream()),
             "gmx_resample_rows_pinned")
    return anc, total, mx, cdf_shift(n), status


def _row_kind(kind, who):
    kind = _KINDS[kind] if isinstance(kind, str) else int(kind)
    if kind in (MULTINOMIAL_TILED, MULTINOMIAL_SORTED):
        raise NotImplementedError(f"{who}: 'multinomial_tiled' / 'multinomial_sorted' have no row form "
                                  "(use 'systematic', 'stratified' or 'multinomial')")
    if kind not in ROW_KINDS:
        raise ValueError(f"{who}: unknown resampling kind {kind}")
    return kind


def _resample_batched(keys: Key, collection: ParticleCollection, kind, n_out) -> ParticleCollection:
    """smc.resample on a collection of R independent particle systems (log_weights [R, n], keys of shape (R,)): row r
    is resampled under keys[r] as the 1-D path resamples it alone — ONE gmx_resample_rows call with index_stride = n and
    ONE gmx_gather of every (R, n) leaf over its flat [R * n] view (materialised).  `ancestors` are row-local [R, n]."""
    lw = collection.get_log_weights()
    if lw.ndim != 2:
        raise NotImplementedError(f"resample: log_weights of shape {tuple(lw.shape)} (one batch axis over the particles)")
    R, n = (int(v) for v in lw.shape)
    if tuple(keys.shape) != (R,):
        raise ValueError(f"resample: log_weights of shape {(R, n)} need keys of shape {(R,)}, one per row; got keys of "
                         f"shape {tuple(keys.shape)}")
    kind = _row_kind(kind, "resample on a batched collection")
    if n_out not in (None, n):
        raise NotImplementedError(f"resample on a batched collection: n_out != n (n_out = {n_out}, n = {n})")
    if n > ROWS_N_MAX or R * n >= 2 ** 31:
        raise NotImplementedError(f"resample on a batched collection: n <= 2^21 and R * n < 2^31 (R = {R}, n = {n})")
    lw = lw.float().contiguous()
    flat, total, mx, shift, _ = resample_rows(kind, keys, lw, index_stride=n)
    found = []

    def pick(v):
        if tuple(v.shape[:2]) == (R, n):
            v = engine.materialize(v)
            found.append(v.reshape((R * n,) + tuple(v.shape[2:])))
        return v
    trace_map(collection.get_particles(), pick)
    moved = iter(engine.gather_leaves(found, flat)) if found else iter(())
    particles = trace_map(collection.get_particles(), lambda v: next(moved) if tuple(v.shape[:2]) == (R, n) else v)
    off = (collection.log_ml_offset or LogMLOffset()).plus(mx, total, shift, n)
    out = ParticleCollection(particles, None, True, off, n_zero=(R, n))          # weights reset to 0, lazily
    out.ancestors = flat - (torch.arange(R, dtype=torch.int32, device=flat.device) * n).reshape(R, 1)
    return out


def extend(key: Key, collection: ParticleCollection, step, step_args, observations: ChoiceMap) -> ParticleCollection:
    """Bootstrap extension by one step: every particle i runs
    `step.importance(split(key, N)[i], observations, step_args_i)` and
    lw_i += weight_i (same algebra as ChangeTarget._reweight, smc.py:378-384,
    restricted to the new step's sites).  `step_args` is a tuple, or a callable
    mapping the previous particles' trace to the tuple."""
    zero = collection.weights_are_zero()
    n = collection._n_zero if zero else collection.get_log_weights().shape[-1]
    if isinstance(n, (tuple, list)):       # a batched collection: (R, n) — `key` then holds R keys, split(key, n) is (R, n)
        n = n[-1]
    args = step_args(collection.get_particles()) if callable(step_args) else tuple(step_args)
    keys = split(key, n)
    from ..static import StaticGenerativeFunction, run_gfi
    if isinstance(step, StaticGenerativeFunction):
        # the step's program also leaves the resampler's tile statistics of its weight when it can
        tr, w = run_gfi(step, "generate", keys, args, constraint=observations, weight_stats=zero)
    else:
        tr, w = step.importance(keys, observations, args)
    if zero:                           # lw + w with lw = 0 exactly (0.0f + w == w for every w but -0.0, which a
        return ParticleCollection(tr, w, True, collection.log_ml_offset)          # sum of log-densities is not)
    return ParticleCollection(tr, engine.elementwise(_add, collection.get_log_weights(), w), True, collection.log_ml_offset)


def rejuvenate(key: Key, collection: ParticleCollection, request, argdiffs=None) -> ParticleCollection:
    """One MH sweep over all particles as ONE fused launch (static.run_mh):
    particle i uses key_i = split(key, N)[i], (k_edit, k_acc) = split(key_i);
    propose with `request.edit(k_edit, ...)`, accept iff log U(k_acc) < weight,
    keep the old trace otherwise (tests/inference/test_requests.py:131-137 idiom).
    Weights are unchanged (an MH kernel leaves the target invariant)."""
    from ..static import run_mh
    tr = collection.get_particles()
    n = collection._n_zero if collection.weights_are_zero() else collection.get_log_weights().shape[0]
    if argdiffs is None:
        argdiffs = Diff.no_change(tr.get_args() or ())
    new_tr, accept, _ = run_mh(tr.get_gen_fn(), lazy_split(key, n), tr, request, argdiffs)
    res = ParticleCollection(new_tr, collection._lw, True, collection.log_ml_offset, n_zero=collection._n_zero)
    res.accept = accept
    return res


class CapturedLoop:
    NOISE_ARENA_MB = 16384     # every draw of a captured loop lives in one arena for the graph's lifetime: its bound

    """A Python inference loop over this module's functional API (resample -> rejuvenate -> extend ...) captured ONCE
    into a hipGraph and replayed without the interpreter in the loop: every C-ABI launch goes to torch's current stream,
    so one capture records them all; tensors made during the capture come from the graph's private pool and stay
    valid (and are overwritten in place) across replays.  `result` is whatever the loop returned at capture time —
    its tensors hold the latest replay's values."""

    def __init__(self, loop_fn, *args, warmup: int = 1, noise_ahead=None):
        be = _lib.get()
        if not be.uses_streams:
            raise _lib.GenmiError("capture needs the HIP backend")
        if noise_ahead is None:
            noise_ahead = os.environ.get("GENMI_NOISE_AHEAD", "1") != "0"
        from contextlib import nullcontext
        from ..static import NoiseAheadContext
        # noise ahead: the draws of the loop's extend / rejuvenate launches by background programs on a
        # second stream; in the captured graph they depend on nothing but each other and run ahead of the chain
        self.noise = NoiseAheadContext(torch.cuda.Stream(device=be.device)) if noise_ahead else None
        scope = self.noise if self.noise is not None else nullcontext()
        side = torch.cuda.Stream(device=be.device)
        side.wait_stream(torch.cuda.current_stream(be.device))
        with torch.cuda.stream(side):           # programs are traced / specialised outside the capture
            for _ in range(max(1, warmup)):
                with scope:
                    loop_fn(*args)
            if self.noise is not None and self.noise.settle():
                with scope:                      # once more, with the launches that keep their draws as they will run
                    loop_fn(*args)
            if self.noise is not None:
                side.wait_stream(self.noise.stream)
                # every draw of the loop lives in one arena for the graph's lifetime: bounded (NOISE_ARENA_MB)
                if 4 * self.noise.demand > int(self.NOISE_ARENA_MB) << 20:
                    self.noise = None
                    loop_fn(*args)               # the plain programs must exist before the capture too
        torch.cuda.current_stream(be.device).wait_stream(side)
        torch.cuda.synchronize(be.device)
        if self.noise is not None:
            self.noise.reserve(be.device)
        self.graph = torch.cuda.CUDAGraph()
        # the graph's kernel nodes point into the site programs' code: hold every program launched during the capture
        # for as long as the graph lives (the program caches are bounded LRUs; genjax_amd.clear_caches() is public)
        with engine.holding_captured_programs() as self.programs, torch.cuda.graph(self.graph):
            if self.noise is not None:
                cur = torch.cuda.current_stream(be.device)
                self.noise.stream.wait_stream(cur)          # the background stream joins the capture ...
                self.noise.issue_ahead(be.device)           # ... every recorded noise launch goes out first ...
                with self.noise:
                    self.result = loop_fn(*args)
                cur.wait_stream(self.noise.stream)          # ... and the stream is joined back before the capture ends
            else:
                self.result = loop_fn(*args)

    def replay(self):
        self.graph.replay()
        return self.result


def capture(loop_fn, *args, warmup: int = 1, noise_ahead=None) -> CapturedLoop:
    """`smc.capture(loop_fn, *args)`: see CapturedLoop.  Host-side reads of device values inside `loop_fn`
    (`.item()`, `float(tensor)`, LogMLOffset.value()) are not capturable — return tensors and read them after
    `replay()`.  noise_ahead (default: on; GENMI_NOISE_AHEAD=0): launches over >= 2^18 particles take their
    launch-keyed normal / uniform draws from background programs on a second stream (same values)."""
    return CapturedLoop(loop_fn, *args, warmup=warmup, noise_ahead=noise_ahead)


class _StateStore:
    """THE place that knows a sweep's state layout.  The state is the init program's return value — a float scalar,
    ONE vector of D floats, or (tuples=True) a tuple / list of D float scalars — kept struct-of-arrays in two [D, width]
    stores (step t writes store t % 2 and reads the other through the ancestors), every row one output of the site
    program and one gathered input of the next step.  `who` names the sweep in the refusals; alloc(shape): the
    allocator of the stores (default: zeros on the device)."""

    def __init__(self, prog, width, who, tuples=True, alloc=None):
        ro, outs = prog.ro, prog.comp.outputs
        self.tuple_state = None
        if tuples and ro[0] in ("tuple", "list") and ro[1] and all(
                o[0] == "out" and outs[o[1]][0] == "f32" and outs[o[1]][1] == () for o in ro[1]):
            self.tuple_state = type(()) if ro[0] == "tuple" else type([])
            event, D = (), len(ro[1])
        else:
            if ro[0] != "out":
                raise NotImplementedError(f"{who}: the step model must return one array (scalar or vector state)"
                                          + (" or a tuple of float scalars" if tuples else ""))
            dt, event, _slots = outs[ro[1]]
            if dt != "f32" or len(event) > 1:
                raise NotImplementedError(f"{who}: the state must be a float scalar or a float vector")
            D = int(event[0]) if event else 1
        self.event, self.D = tuple(event), D
        self._alloc = alloc or (lambda shape: torch.zeros(shape, dtype=torch.float32, device=_lib.get().device))
        self.allocate(width)

    def allocate(self, width):
        """the pair of [D, width] stores (again: another width)"""
        self.rows = [self._alloc((self.D, int(width))) for _ in range(2)]
        self._views = {}

    def view(self, which, n=None):
        """store `which` as the model sees it — [width], [width, D] or a tuple of [width] rows; n: its first n columns"""
        v = self._views.get((which, n))
        if v is None:
            s = self.rows[which] if n is None else self.rows[which][:, :n]
            if self.tuple_state is not None:
                v = self.tuple_state(s[d] for d in range(self.D))
            else:
                v = s[0] if not self.event else s.t()
            self._views[(which, n)] = v
        return v

    def gathered(self, which, index):
        """view(which)[index] as a model argument (lazy: the gather is fused into the program that reads it)"""
        v = self.view(which)
        if self.tuple_state is not None:
            return self.tuple_state(Gathered(row, index) for row in v)
        return Gathered(v, index)

    def bind(self, bufs, prog, which, n=None, moved=False):
        """the rows of store `which` (n: their first n columns) as the output buffers of prog's return value (moved=True:
        of the MH-moved state a chained program returns besides)"""
        s = self.rows[which] if n is None else self.rows[which][:, :n]
        o = prog.mo if moved else prog.ro
        if self.tuple_state is not None:
            for d, od in enumerate(o[1]):
                bufs[od[1]] = s[d:d + 1]
        else:
            bufs[o[1]] = s

    def leaves(self, which):
        """the D rows of store `which`, each a leaf the sharded exchange routes"""
        return list(self.rows[which])

    def per_filter(self, which, R, n):
        """store `which` over R * n particles as R filters see it: [R, n], [R, n, D] or a tuple of [R, n]"""
        v = self.view(which)
        if self.tuple_state is not None:
            return self.tuple_state(row.reshape(R, n) for row in v)
        return v.reshape((R, n) + self.event)

    def take(self, which, index):
        """view(which)[index], materialised: [len(index)] or [len(index), D] (ONE gmx_gather over the rows)"""
        got = engine.gather_leaves(self.leaves(which), index)
        return got[0] if not self.event else torch.stack(got, dim=1)


class _Sweep:
    """What BootstrapSweep, BootstrapBank and sharded.ShardedBootstrapSweep do alike: the per-step key schedule, the
    site programs and the table of what step t launches (`_programs`), capturing enqueue() into a graph, replaying and
    dropping it, and the noise-ahead machinery: background programs that draw the chain programs' hoisted
    normal / uniform values on a second stream, a group of steps ahead.

    What differs between the sweeps is handed over as values, set by the host class's prepare():
      batch         particles per launch (n; the bank: R * n)
      store, moved  the _StateStore of the state and (rejuvenate=) of the MH-moved state step t is extended from
      index         the ancestors the previous state is gathered through
      window        None, or the n columns of a wider store the programs write (the sharded [n | received] rows)
      tail          trailing model arguments (the bank's per-particle parameters)
      chained       the MH move and the extension run as ONE program
      step_keys[t]  (proposal, resampling, MH move) keys of step t; how a launch key is split over the particles is the
                    host class's own
    The host class also provides n, T, specialize, `_chain_step(t, skip_vm)` (everything step t launches on the chain)
    and `enqueue()`; `_noise_total` / `_noise_offset`: the keys of this shard are children offset .. offset + n - 1 of
    split(k, total) (a single GPU: total = n, offset = 0)."""

    NOISE_LDS_PAD = 56000      # bytes of unused LDS per noise workgroup: two of them per CU (160 KB)
    NOISE_GROUP = 10           # steps per group of noise launches (the noise runs one group ahead of the chain)
    NOISE_RING = 3             # groups of noise buffers (the background stream runs at most NOISE_RING - 1 groups ahead)
    _noise_offset = 0
    _noise_total = None
    graph = None
    window = moved = rejuvenate = None
    tail = ()
    chained = noise_ahead = False

    def _set_observations(self, ys):
        self.ys = ys.to(_lib.get().device).float().contiguous()
        self._obs_maps = {}

    def _obs(self, t):
        """step t's observation as the constraint of its programs (made once per prepared run, not per launch)"""
        obs = self._obs_maps.get(t)
        if obs is None:
            obs = self._obs_maps[t] = ChoiceMap.empty().set(self.obs_addr, self.ys[t])
        return obs

    def _build_init(self, hoist=False):
        from ..static import MinimalGenerate
        self.p_init = MinimalGenerate(self.init, self.tail, self._obs(0), (self.batch,), hoist_noise=hoist)

    def _build_steps(self, hoist=False, step_hoist=False, chain=False, chain_hoist=False):
        """The step programs, once p_init and the stores exist: p_step — without a move it gathers the previous state
        (noise hoisted: `hoist`), with one it reads the moved state in place (`step_hoist`) —; rejuvenate=: the move alone,
        p_mh_init / p_mh_step, and (chain) the move and the extension that follows it as ONE program, p_mhvm_init /
        p_mhvm_step (static.MinimalMHGenerate: same keys, same draws, same bits; one launch boundary and one trip of the
        moved state through memory less; `chain_hoist`: which of its draws are hoisted)"""
        from ..static import MinimalGenerate, MinimalMH, MinimalMHGenerate
        obs0, ex, b = self._obs(0), tuple(self.step_extra(1)), (self.batch,)
        prev = self.store.gathered(0, self.index)
        self.p_mhvm_init = self.p_mhvm_step = None
        if self.rejuvenate is None:
            self.p_step = MinimalGenerate(self.step, (prev,) + ex + self.tail, obs0, b, hoist_noise=hoist)
            return
        self.p_step = MinimalGenerate(self.step, (self.moved.view(0, self.window),) + ex, obs0, b, hoist_noise=step_hoist)
        ch = obs0.set(self.state_addr, prev)
        was = (self.moved.gathered(0, self.index),) + ex
        self.p_mh_init = MinimalMH(self.init, (), ch, self.rejuvenate, b)
        self.p_mh_step = MinimalMH(self.step, was, ch, self.rejuvenate, b)
        if chain:
            self.p_mhvm_init = MinimalMHGenerate(self.init, (), ch, self.rejuvenate, self.step, ex, obs0, b,
                                                 hoist_noise=chain_hoist)
            self.p_mhvm_step = MinimalMHGenerate(self.step, was, ch, self.rejuvenate, self.step, ex, obs0, b,
                                                 hoist_noise=chain_hoist)

    def _chain_prog(self, t):
        """the site program of step t on the chain"""
        if t == 0:
            return self.p_init
        if self.chained:
            return self.p_mhvm_init if t == 1 else self.p_mhvm_step
        return self.p_step

    def _programs(self, t, alone=False):
        """Which programs step t launches, on which leaves, under which key, into which buffers: (mh, prog, leaves, launch
        key, bufs) — init; the plain step; the chained MH move + extension (one program); or the separate MH move, `mh`
        = its own (prog, leaves, key, bufs), then the extension.  alone=True: the extension without its move, whatever
        the form (kernel_timers).  The log-weight buffer, and how the key is split, are the caller's to set."""
        n = self.n
        k_prop, _k_res, k_mh = self.step_keys[t]
        obs = self._obs(t)
        mh, key, moves = None, k_prop, False
        if t == 0 or self.rejuvenate is None:
            prog = self.p_init if t == 0 else self.p_step
            a_ = self.tail if t == 0 else \
                (self.store.gathered((t - 1) % 2, self.index),) + tuple(self.step_extra(t)) + self.tail
            leaves = prog.leaves(a_, obs, self._noise_leaves(t, prog)) if self.noise_ahead else prog.leaves(a_, obs)
        elif self.chained and not alone:
            # the MH move on the resampled particles of step t - 1: reads x_{t-1}[index] and, for t >= 2, the moved state
            # x_{t-1} was extended from; and, in the SAME program, the extension to step t from the moved state (keys
            # split(k_prop, ..): OP_KSPLITU of two launch values); the launch key of the chained program is the MOVE's
            prog = self.p_mhvm_init if t == 1 else self.p_mhvm_step
            kw = k_prop.host()
            leaves = prog.leaves(*self._move_leaves(t), tuple(self.step_extra(t)), obs, (int(kw[0]), int(kw[1])),
                                 self._noise_leaves(t, prog) if self.noise_ahead else ())
            key, moves = k_mh, True
        else:
            if not alone:
                mprog = self.p_mh_init if t == 1 else self.p_mh_step
                mbufs = [None] * len(mprog.comp.outputs)
                self.moved.bind(mbufs, mprog, t % 2, self.window)
                mbufs[mprog.ao[1]] = self.accept.reshape(1, n)
                mh = (mprog, mprog.leaves(*self._move_leaves(t)), k_mh, mbufs)
            prog = self.p_step                       # ... then the extension reads the move's output in place
            a_ = (self.moved.view(t % 2, self.window),) + tuple(self.step_extra(t))
            leaves = prog.leaves(a_, obs, self._noise_leaves(t, prog)) if self.noise_ahead else prog.leaves(a_, obs)
        bufs = [None] * len(prog.comp.outputs)
        self.store.bind(bufs, prog, t % 2, self.window)
        if moves:
            self.moved.bind(bufs, prog, t % 2, self.window, moved=True)     # the moved state step t was extended from
            bufs[prog.ao[1]] = self.accept.reshape(1, n)
        return mh, prog, leaves, key, bufs

    def _move_leaves(self, t):
        """(arguments, choices, request) of the MH move of step t >= 1: on x_{t-1}[index] under step t - 1's observation"""
        ch = self._obs(t - 1).set(self.state_addr, self.store.gathered((t - 1) % 2, self.index))
        a_ = () if t == 1 else (self.moved.gathered((t - 1) % 2, self.index),) + tuple(self.step_extra(t - 1))
        return a_, ch, self.rejuvenate

    def launch(self):
        """replay the captured graph, or else enqueue()"""
        if self.graph is None:
            self.enqueue()
        else:
            be = _lib.get()
            be.check(be.c.gmx_graph_launch(self.graph, be.stream()), "gmx_graph_launch")

    def _set_step_keys(self, key):
        """step key = fold_in(run key, t); (k_prop, k_res, k_mh) = split(step key, 3) — on the host"""
        self.step_keys = []
        for t in range(self.T):
            ks = split(fold_in(key, t), 3)
            self.step_keys.append((ks[0], ks[1], ks[2]))

    def _drop_graph(self):
        """release the captured graph (it holds the launch arguments and buffers of the run it was captured for), once
        the stream has drained"""
        if self.graph is None:
            return
        be = _lib.get()
        if be.uses_streams:
            torch.cuda.synchronize()
        be.c.gmx_graph_destroy(self.graph)
        self.graph = None

    def capture(self):
        """Capture enqueue() into a hipGraph (launch-bound: ~5 nodes per step)."""
        be = _lib.get()
        from ctypes import c_void_p
        s = torch.cuda.Stream(device=be.device)
        s.wait_stream(torch.cuda.current_stream(be.device))
        with torch.cuda.stream(s):
            self.enqueue()          # warm-up outside capture (program upload, lazy init)
            s.synchronize()
            be.check(be.c.gmx_capture_begin(be.stream()), "gmx_capture_begin")
            try:
                self.enqueue()
            finally:
                h = c_void_p()
                rc = be.c.gmx_capture_end(be.stream(), h)
            be.check(rc, "gmx_capture_end")
        torch.cuda.current_stream(be.device).wait_stream(s)
        self.graph = h
        return self

    def _noise_split(self, k):
        total = self._noise_total or self.n
        return lazy_split(k, total, offset=self._noise_offset) if (self._noise_offset or total != self.n) else lazy_split(k, self.n)

    def _noise_setup(self, chain_progs, n, T, dev):
        from ..static import NoiseProgram
        be = _lib.get()
        self.noise_ahead = True
        # one background program per (chain program, root key): the draws that hang off the launch key (the
        # step's own sites; with rejuvenate=, the move's proposal and accept draws: key k_mh) and those that hang
        # off the chained extension's key (KSPLITU: k_prop)
        for P in chain_progs:
            if id(P) in self._noise_progs:
                continue
            by_root = {}
            for k_, d in enumerate(P.noise):
                by_root.setdefault(d[0], []).append(k_)
            self._noise_progs[id(P)] = [(root, NoiseProgram([P.noise[k_] for k_ in idx], (n,)), idx)
                                        for root, idx in by_root.items()]
        self.noise_group = max(1, min(int(os.environ.get("GENMI_NOISE_GROUP", self.NOISE_GROUP)), T))
        # the ring of noise buffers: NOISE_RING groups, so the background stream may run NOISE_RING - 1 groups ahead
        # (measured on MI355X, config 2: 14.50 -> 14.32 us/step with 3, 14.27 with 4; the sorted multinomial, whose
        # background stream also builds tables, is better off with 2: 21.2 vs 21.9 — profiles/r03cd_ring_*.json)
        ring = 2 if getattr(self, "kind", None) == MULTINOMIAL_SORTED else self.NOISE_RING
        self.noise_ring = max(2, int(ring))
        # groups of steps [start, end): the noise of group g + 1 is issued before the chain of group g.  The chain
        # can only start once the FIRST group's noise is there, so the groups grow 1, 2, 4, ... up to noise_group
        self.noise_groups, self.noise_slot = [], []
        t0, size = 0, 1
        while t0 < T:
            t1 = min(T, t0 + min(size, self.noise_group))
            for t in range(t0, t1):
                self.noise_slot.append((len(self.noise_groups) % self.noise_ring, t - t0))
            self.noise_groups.append((t0, t1))
            t0, size = t1, size * 2
        S = max(len(P.noise) for P in chain_progs)
        # two groups of noise buffers: the background stream fills one while the chain reads the other.
        # [half, draw, row of the group, n]: a draw's rows are contiguous, so ONE launch can fill several steps
        self.zbuf = torch.zeros((self.noise_ring, S, self.noise_group, n), dtype=torch.float32, device=dev)
        self._noise_stream = torch.cuda.Stream(device=dev) if be.uses_streams else None
        pad = int(self.NOISE_LDS_PAD)
        for plist in self._noise_progs.values():
            for _, q, _ in plist:
                if self.specialize:
                    q.comp.set_background(pad)
                    q.comp.specialize()

    def _noise_views(self, t, count):
        """the [1, n] buffers of step t's draws: half (t // group) % 2 of the ring, row t % group"""
        half, row = self.noise_slot[t]
        return [self.zbuf[half, k, row:row + 1] for k in range(count)]

    def _noise_leaves(self, t, prog):
        return [v.reshape(self.n) for v in self._noise_views(t, len(prog.noise))]

    def _noise_runs(self, g):
        """The background launches of group g: the steps of a group that share a chain program get their draws from ONE
        launch per key root — a 2-D grid, one row of keys per step (GMX_KEY_ROWSPLIT; gmx_program_run) — instead of
        one launch per step: fewer nodes in the graph (the HIP runtime walks a two-stream graph node by node on the
        host) and no launch boundary between the steps' noise."""
        cache = self.__dict__.setdefault("_noise_run_cache", {})
        if g in cache:
            return cache[g]
        n = self.n
        t0, t1 = self.noise_groups[g]
        runs, ta = [], t0
        while ta < t1:
            tb = ta + 1
            while tb < t1 and self._chain_prog(tb) is self._chain_prog(ta):
                tb += 1
            runs.append((ta, tb))
            ta = tb
        out = []
        dev = self.zbuf.device
        for ta, tb in runs:
            P = self._chain_prog(ta)
            half, row_a = self.noise_slot[ta]
            rows = tb - ta
            mh = self.chained and ta >= 1
            for root, q, idx in self._noise_progs[id(P)]:
                ks = [self.step_keys[t][2] if (mh and root == "LDKEY") else self.step_keys[t][0] for t in range(ta, tb)]
                if rows == 1 or rows * n >= 2 ** 31 - 4096:
                    for r, k in enumerate(ks):
                        out.append((q, (n,), self._noise_split(k), [self.zbuf[half, k_, row_a + r:row_a + r + 1] for k_ in idx]))
                    continue
                kd = torch.from_numpy(np.stack([k.host() for k in ks]).astype(np.uint32).view(np.int32)).to(dev)
                # row r's keys: children offset .. offset + n - 1 of split(ks[r], total) (GMX_KEY_ROWSPLIT + index_offset)
                key = Key(lazy=("rowsplit", Key(dev=kd), n), split_last=True, offset=self._noise_offset)
                out.append((q, (rows * n,), key, [self.zbuf[half, k_, row_a:row_a + rows].reshape(1, rows * n) for k_ in idx]))
        cache[g] = out
        return out

    def _launch_noise_group(self, g):
        self._launch_group_extras(g)
        for q, batch, key, outs in self._noise_runs(g):
            q.run(batch, key, outs)

    def _launch_group_extras(self, g):
        """other key-only work of group g's steps that belongs on the background stream (BootstrapSweep: the stratified
        resampler's slot uniforms)"""

    def _launch_noise(self, t):
        """the draws step t's chain program reads, by the background programs: root LDKEY from the program's launch key
        (k_prop; the chained MH + extension program: k_mh), root KSPLITU from the extension's key k_prop"""
        P = self._chain_prog(t)
        views = self._noise_views(t, len(P.noise))
        mh = self.chained and t >= 1
        for root, q, idx in self._noise_progs[id(P)]:
            k = self.step_keys[t][2] if (mh and root == "LDKEY") else self.step_keys[t][0]
            q.run((self.n,), self._noise_split(k), [views[k_] for k_ in idx])

    def _enqueue_noise_ahead(self, skip_vm=False, skip_noise=False):
        """The sweep on TWO streams: the chain [site program' -> resampler] per step on the current one, the noise
        programs on the background stream, one group of steps ahead (group g + 1's noise is issued before group g's
        chain; with a ring of R groups of buffers, group g + R - 1's before group g's chain: it may overwrite slot (g - 1) % R
        once the chain of group g - 1 has read it; the groups
        grow 1, 2, 4, ... steps up to noise_group, so the chain starts after ONE noise launch).  Capturable:
        the background stream joins the capture through the first event wait and is joined back at the end.
        Without streams (the CPU mirror of the C-ABI) the same launches run in issue order."""
        be = _lib.get()
        spans = self.noise_groups
        groups = len(spans)
        two = be.uses_streams and self._noise_stream is not None
        if two:
            A, Bs = torch.cuda.current_stream(be.device), self._noise_stream
            Bs.wait_stream(A)
        done, ready = [None] * groups, [None] * groups

        def noise_group(g):
            if skip_noise:
                return
            if two:
                with torch.cuda.stream(Bs):
                    if g >= ring:
                        Bs.wait_event(done[g - ring])
                    self._launch_noise_group(g)
                    ready[g] = torch.cuda.Event()
                    ready[g].record(Bs)
            else:
                self._launch_noise_group(g)

        ring = getattr(self, "noise_ring", 2)
        for g in range(min(ring - 1, groups)):
            noise_group(g)
        for g in range(groups):
            if g + ring - 1 < groups:
                noise_group(g + ring - 1)
            if two and not skip_noise:
                A.wait_event(ready[g])
            for t in range(*spans[g]):
                self._chain_step(t, skip_vm)
            if two and not skip_noise:
                done[g] = torch.cuda.Event()
                done[g].record(A)
        if two:
            A.wait_stream(Bs)


BACKWARD_ROWS_MAX = 16                 # rows of backward-simulation logits per density launch (and per gmx_pick_rows call)
BACKWARD_CHUNK_BYTES = 256 << 20       # ... and at most this much of them in memory
_BACKWARD_CACHE = engine.new_cache()


def _assess_program(model, args, leaves, form, emit, refuse, out, specialize=False, launch=True):
    """THE builder of the programs that score a model's `assess` under a choice map made of leaves, one output (or a tuple
    of them: `emit` returns a tuple and `out` is the tuple of their buffers), over the n = out.shape[-1] particles of ONE
    launch.  The leaves are those of `args` (the model's arguments), then `leaves`, one each; `emit(assess, syms, tr)` fills the choice map(s) from the symbols `syms` of the latter and returns what is stored
    as `out`, `assess(con)` being (the call's record, its score under `con` as a float expression).  A site of the model
    that `con` does not hold goes to `refuse(addresses)`, which raises.  Cached on the model, the leaves' kinds,
    `form` (what tells the callers' programs apart) and `specialize` (specialised once, when built); launch=False builds
    the program only.  Returns a launcher for callers whose leaves and outputs are persistent buffers: its first call is
    this launch, every later one re-launches ONE binding of those buffers (Compiled.bind / launch), with none of the
    per-call flattening and cache look-up."""
    from .. import tracer as Tr
    from ..engine import Compiled, Flat, leaf_spec
    from ..static import MissingAddress, _gfkey, _traced, call_gen_fn
    outs = out if isinstance(out, tuple) else (out,)
    batch = (int(outs[0].shape[-1]),)
    flat = Flat()
    atree = flat.add(tuple(args))
    j0 = len(flat.leaves)
    for v in leaves:
        flat.add(v)
    specs = tuple(leaf_spec(v, batch) for v in flat.leaves)
    ck = (_gfkey(model), atree, specs, form, bool(specialize))
    ent = _BACKWARD_CACHE.get(ck)
    if ent is None:
        with _traced(specs, 1, store_sites=False) as p:
            sargs = p.values(atree)

            def assess(con):
                try:
                    rec, _, _, s = call_gen_fn(p.ctx, "assess", model, None, sargs, con, None, None, None, ())
                except MissingAddress as e:
                    refuse([a for a in e.args if a != ()])
                return rec, Tr.as_float(s)
            res = emit(assess, p.syms[j0:], p.tr)
            o = tuple(p.tr.emit_output(v) for v in (res if isinstance(res, tuple) else (res,)))
        comp = Compiled(p.tr)
        if specialize:
            comp.specialize()
        ent = _BACKWARD_CACHE[ck] = (comp, o)
    comp, o = ent
    bufs = [None] * len(comp.outputs)
    for oi, buf in zip(o, outs):
        bufs[oi[1]] = buf
    if launch:
        comp.run(flat.leaves, batch, None, out_buffers=bufs)
    bound = []
    # (a strided leaf — a vector state's [n, D] view of a [D, n] slab — is copied when it is bound: launched afresh)
    fixed = all(v.is_contiguous() for v in flat.leaves if isinstance(v, torch.Tensor))

    def again():
        if bound:
            return comp.launch(bound[0])
        comp.run(flat.leaves, batch, None, out_buffers=bufs)           # (a specialised program's cross-check is in run())
        if fixed:
            bound.append(comp.bind(flat.leaves, batch, None, out_buffers=bufs))
    return again


def _transition_refusal(who, sites, obs_addr):
    def refuse(addr):
        raise NotImplementedError(
            f"{who}: the step model samples {addr[0] if len(addr) == 1 else tuple(addr)!r}, "
            f"which is neither one of the state's sites {tuple(sites)!r} nor the observation {obs_addr!r}: the "
            "transition density would have to integrate it out") from None
    return refuse


def _transition_choices(sites, obs_addr, y, x_next):
    con = ChoiceMap.empty().set(obs_addr, y)
    for a, x in zip(sites, x_next):
        con = con.set(a, x)
    return con


def _backward_logits(step, sites, obs_addr, x_prev, extra, x_next, y, lw, out):
    """out[k, i] = lw[i] + step.assess({sites[d]: x_next[d][k], obs_addr: y}, (x_prev[i], *extra))[0] in float32, for the
    R = out.shape[0] rows in ONE launch: the model's `assess` traced R times, row k's constrained state read from the
    launch-uniform short vectors x_next[d] (as inference/gibbs.py traces K categories), the R sums stored as the rows
    of `out` ([R, n], rows contiguous).  The program is cached on the model, the leaves' kinds and R."""
    from ..engine import Broadcast, Sym
    R, D = int(out.shape[0]), len(x_next)

    def emit(assess, syms, tr):            # syms: y, the D short vectors, lw
        rows = np.empty((R,), dtype=object)
        for k in range(R):
            con = _transition_choices(sites, obs_addr, syms[0], [Sym(x.value[k], None) for x in syms[1:1 + D]])
            rows[k] = syms[1 + D].value + assess(con)[1]
            tr.prestore(rows[k])            # (stored now: the row's register dies here)
        return rows
    _assess_program(step, (x_prev,) + tuple(extra), [y] + [Broadcast(v) for v in x_next] + [lw], (tuple(sites), obs_addr, R),
                    emit, _transition_refusal("SweepHistory.backward_sample", sites, obs_addr), out)


def _ancestor_logits(step, sites, obs_addr, x_prev, extra, x_next, y, lw, out, specialize=False, launch=True,
                     who="ConditionalBank(ancestor_sampling=True)"):
    """out[i] = lw[i] + step.assess({sites[d]: x_next[d][i], obs_addr: y}, (x_prev[i], *extra))[0] in float32 over the
    n = lw.shape[0] particles in ONE launch: the per-particle variant of _backward_logits (ancestor sampling:
    ConditionalBank) — the constrained state is a per-particle leaf x_next[d] ([n] each: every chain's next retained state
    on each of its particles), `extra` may hold per-particle leaves (the bank's parameters), `out` is [1, n].  The
    program is cached on the model, the leaves' kinds and `specialize` (specialised once, when built); launch=False
    builds it only.  who: the caller a refusal names (ConditionalBank.draw(backward=True) runs the same program over the
    recorded steps)."""
    D = len(x_next)

    def emit(assess, syms, tr):            # syms: y, the D per-particle states, lw
        return syms[1 + D].value + assess(_transition_choices(sites, obs_addr, syms[0], syms[1:1 + D]))[1]
    _assess_program(step, (x_prev,) + tuple(extra), [y] + list(x_next) + [lw], (tuple(sites), obs_addr, "per-particle"),
                    emit, _transition_refusal(who, sites, obs_addr), out, specialize, launch)


class SweepHistory:
    """What BootstrapSweep(history=True) recorded: every step's particles, log-weights and ancestors.

      x            [T, n] (scalar state), [T, n, D] (vector state) or a tuple of [T, n] (tuple state)
      log_weights  [T, n]
      ancestors    [T, n] int32: row t is the resampling AFTER step t (row T-1 = state()[2])

    The reference's SMC carries whole Scan traces through every resampling; here a step is recorded once and a
    trajectory is ONE backward walk through the ancestor rows (gmx_lineage: one launch, one lane per trajectory)."""

    def __init__(self, xs, lws, ancs, event=(), tuple_state=None, *, step=None, ys=None, step_extra=None, obs_addr=None,
                 state_addr=None):
        """step / ys / step_extra / obs_addr / state_addr: the sweep's model, for backward_sample() (BootstrapSweep.history()
        hands them over; every other method works without)"""
        self._xs, self.log_weights, self.ancestors = xs, lws, ancs
        self._event, self._tuple = tuple(event), tuple_state
        self.T, self.D, self.n = (int(v) for v in xs.shape)
        self._step, self._ys, self._step_extra = step, ys, step_extra
        self._obs_addr, self._state_addr = obs_addr, state_addr

    def _state_view(self, a, lead):
        """[T, D, k] -> the state's shape with the step axis at `lead` = 0 ([T, k, ...]) or 1 ([k, T, ...])"""
        if self._tuple is not None:
            return self._tuple((a[:, d] if lead == 0 else a[:, d].t()) for d in range(self.D))
        if not self._event:
            return a[:, 0] if lead == 0 else a[:, 0].t()
        return a.transpose(1, 2) if lead == 0 else a.permute(2, 0, 1)

    @property
    def x(self):
        return self._state_view(self._xs, 0)

    def _walk(self, start, want_paths, want_traj):
        be = _lib.get()
        dev = self._xs.device
        if start is None:
            start = self.ancestors[self.T - 1]
        start = torch.as_tensor(start, device=dev).to(torch.int32).contiguous().reshape(-1)
        m = int(start.numel())
        paths = torch.empty((self.T, m), dtype=torch.int32, device=dev) if want_paths else None
        traj = torch.empty((self.T, self.D, m), dtype=torch.float32, device=dev) if want_traj else None
        if m == 0:
            return paths, traj
        status = torch.zeros((1,), dtype=torch.int64, device=dev)
        be.check(be.c.gmx_lineage(be.ptr(self.ancestors), be.ptr(self._xs), self.T, self.D, self.n, be.ptr(start), m,
                                  be.ptr(paths), be.ptr(traj), be.ptr(status), be.stream()), "gmx_lineage")
        bad = int(status.item())
        if bad:
            raise IndexError(f"SweepHistory: {bad} index(es) outside [0, {self.n}) on the walk (start, or a recorded "
                             "ancestor): they were clamped, nothing outside the history was read")
        return paths, traj

    def lineage(self, start=None):
        """int32 [T, m]: row t = the step-t particle on the lineage of each of `start`'s step-(T-1) particles (default:
        ancestors[T-1], the sweep's own last resampling — n equally weighted draws from the final weights)"""
        return self._walk(start, True, False)[0]

    def trajectories(self, start=None):
        """the states along those lineages: [m, T] / [m, T, D] / a tuple of [m, T] (views of the kernel's [T, D, m])"""
        return self._state_view(self._walk(start, False, True)[1], 1)

    def backward_sample(self, key: Key, m: int, state_sites=None, return_paths=False):
        """m trajectories by forward filtering, backward simulation (Godsill, Doucet & West 2004) over the recorded steps:
        the last state is drawn from the final weights, and going back every particle of step t is re-weighted by the
        transition density into the state already chosen at step t + 1 — where the lineages of `trajectories()` coalesce
        to a handful of early ancestors, these draws do not.

          k_t = fold_in(key, t)                                                    (key: ONE key)
          paths[T-1, :] = ancestors_from_cdf(MULTINOMIAL, k_{T-1}, *weight_cdf(lw_{T-1})[:2], n_out=m)
          t = T-2 .. 0, row keys split(k_t, m):
            logits[k, i] = lw_t[i] + step.assess({site_d: x~_{t+1}[k][d], obs_addr: y_{t+1}}, (x_t[i], *step_extra(t+1)))[0]
            paths[t, k]  = gmx_pick_rows: the exact-integer multinomial draw of row k under its key
            x~_t[k]      = x_t[paths[t, k]]

        (float32 sums; the observation's term is constant along a row and kept so that the bits are defined).  The
        densities of up to BACKWARD_ROWS_MAX rows are ONE launch of one cached site program (the model's own `assess`
        traced once per row with that row's chosen state as launch-uniform values); nothing passes through the host
        between steps.  Every draw has the resolution of the multinomial resampler's 23-bit uniform, as everywhere else
        in the project: a particle whose share of a row's mass is below 2^-23 may never be drawn.

        state_sites: the address of each state component, in order (default (state_addr,) for a scalar state; required
        for D > 1).  The model may have no latent site besides them and the observation.
        Returns the trajectories in trajectories()'s layout ([m, T] / [m, T, D] / a tuple of [m, T]); with
        return_paths=True, (paths int32 [T, m], trajectories).  A row without any mass (every candidate's density -inf)
        raises FloatingPointError naming the step."""
        if self._step is None or self._ys is None or self._obs_addr is None:
            raise RuntimeError("SweepHistory.backward_sample: this SweepHistory was built without the model (step=, ys=, "
                               "step_extra=, obs_addr=, state_addr=): take it from BootstrapSweep.history()")
        if tuple(key.shape) != ():
            raise ValueError("SweepHistory.backward_sample takes ONE key")
        if state_sites is None:
            if self.D > 1:
                raise NotImplementedError("SweepHistory.backward_sample: a state of more than one component needs "
                                          "state_sites= (the address of each component, in order)")
            state_sites = (self._state_addr,)
        sites = tuple(state_sites)
        if len(sites) != self.D:
            raise ValueError(f"SweepHistory.backward_sample: state_sites names {len(sites)} addresses for a state of "
                             f"{self.D} components")
        be = _lib.get()
        dev = self._xs.device
        T_, D, n, m = self.T, self.D, self.n, int(m)
        paths = torch.empty((T_, m), dtype=torch.int32, device=dev)
        traj = torch.empty((T_, D, m), dtype=torch.float32, device=dev)
        if m > 0:
            lw_last = self.log_weights[T_ - 1]
            if lw_last.data_ptr() % 16:        # row T-1 of a [T, n] slab with n % 4 != 0: gmx_weight_cdf loads float4
                lw_last = lw_last.clone()
            cdf, total, _, _ = weight_cdf(lw_last)
            paths[T_ - 1] = ancestors_from_cdf(MULTINOMIAL, fold_in(key, T_ - 1), cdf, total, n_out=m)
            traj[T_ - 1] = self._xs[T_ - 1].index_select(1, paths[T_ - 1].long())
            status = torch.zeros((T_,), dtype=torch.int64, device=dev)      # word t: the rows of step t without any mass
            extra = self._step_extra or (lambda t: ())
            R = max(1, min(BACKWARD_ROWS_MAX, m, BACKWARD_CHUNK_BYTES // (4 * n), 40 // D))
            logits = torch.empty((R, n), dtype=torch.float32, device=dev)
            ws = torch.empty(((be.c.gmx_pick_rows_workspace(R, n) + 7) // 8,), dtype=torch.int64, device=dev)
            for t in range(T_ - 2, -1, -1):
                keys = split(fold_in(key, t), m).data()
                x_t = self._state_view(self._xs[t:t + 1], 0)
                x_t = type(x_t)(v[0] for v in x_t) if self._tuple is not None else x_t[0]
                for r0 in range(0, m, R):
                    rc = min(R, m - r0)
                    _backward_logits(self._step, sites, self._obs_addr, x_t, tuple(extra(t + 1)),
                                     [traj[t + 1, d, r0:r0 + rc] for d in range(D)], self._ys[t + 1], self.log_weights[t],
                                     logits[:rc])
                    be.check(be.c.gmx_pick_rows(be.ptr(keys[r0:]), be.ptr(logits), rc, n, n, be.ptr(paths[t, r0:]),
                                                be.ptr(status[t:]), be.ptr(ws), be.stream()), "gmx_pick_rows")
                traj[t] = self._xs[t].index_select(1, paths[t].long())
            if int(total.item()) == 0:
                raise FloatingPointError(f"SweepHistory.backward_sample: step {T_ - 1}: the final weights carry no mass")
            bad = torch.nonzero(status).reshape(-1).tolist()
            if bad:
                raise FloatingPointError(f"SweepHistory.backward_sample: step {bad[-1]}: {int(status[bad[-1]].item())} of the {m} "
                                         "trajectories found no step-t particle with a positive transition density into "
                                         "their next state (a row of -inf logits)")
        out = self._state_view(traj, 1)
        return (paths, out) if return_paths else out

    def filter_mean(self):
        """E[x_t | y_1..t] per step: sum_i softmax(lw_t)_i x_t[i], float64 [T] (scalar state) or [T, D]"""
        # the softmax written out (torch.softmax on float64 was measured at float32-level error on the device: weights
        # off by 4e-9, against the 1e-16 of exp / sum / divide in float64)
        lw = self.log_weights.double()
        e = torch.exp(lw - lw.max(dim=1, keepdim=True).values)
        w = e / e.sum(dim=1, keepdim=True)
        mean = (w[:, None, :] * self._xs.double()).sum(dim=2)
        return mean[:, 0] if (self._tuple is None and not self._event) else mean


class BootstrapSweep(_Sweep):
    """A whole bootstrap particle filter (T steps, resampling every step) as a
    fixed sequence of launches on one stream, capturable into a hipGraph — two launches per step:

      per step t:  [site program]  x_t[i] ~ step(x_{t-1}[anc[i]]), lw[i] = log p(y_t | x_t[i]); specialised with 4
                                   particles per thread a workgroup is one 1024-particle tile of the integer CDF
                                   and also leaves the tile statistics (max, fixed-point weight sum)
                   [offspring]     k_offspring_tile: global exponent + tile prefixes from the statistics, the
                                   tile's CDF rebuilt in registers, exact systematic / stratified ancestors
      (programs that cannot write the statistics: + gmx_tile_stats; multinomial or n > 2^21: gmx_weight_cdf +
       gmx_ancestors)

    Key schedule (build-defined): step key = fold_in(run_key, t);
    (k_prop, k_res, k_mh) = split(step key, 3); particle i uses split(k_prop, N)[i].
    The evidence is accumulated from the integer CDF totals in float64 on the host.

    NOISE AHEAD (`noise_ahead`, default: on when it applies; GENMI_NOISE_AHEAD=0 switches it off).  A step is bound by
    vector-instruction issue, and two thirds of its instructions are the Threefry blocks and the `erf_inv` of the
    step's normal draws — which depend on keys and particle indices only, not on anything the chain
    [site program -> resampler -> site program ...] produces.  So the step's `normal` sites take their standard-normal
    draws from memory (static.MinimalGenerate(hoist_noise=True)) and a BACKGROUND program (static.NoiseProgram:
    priority 0, a capped number of workgroups per CU) draws them on a second stream, a group of steps ahead of the
    chain, filling the issue slots the chain's launch boundaries and memory round trips leave idle.  Same keys, same
    operations in the same order: every particle, weight and ancestor is the one the one-stream form computes.
    Measured on MI355X (config 2): 17.9 -> 15.8 us/step.

    `resample`: "systematic" (default), "stratified", and three multinomial forms with the same offspring law —
    "multinomial" (iid slot order: a random particle per slot), "multinomial_tiled" (ordered by the ancestor's CDF tile)
    and "multinomial_sorted" (the uniforms drawn sorted: ordered by ancestor, on the systematic resampler's kernel; the
    fastest of the three: DESIGN.md §4).  The background stream also draws what the resampler needs from its key alone:
    the stratified slot uniforms, the sorted multinomial's order-statistics table.
    """

    NOISE_LDS_PAD = 56000      # bytes of unused LDS per noise workgroup: two of them per CU (160 KB)
    NOISE_GROUP = 10           # steps per group of noise launches (the noise runs one group ahead of the chain)
    NOISE_ROOTS_MH = "LDKEY"   # with rejuvenate=: which keys' draws the background programs take (see prepare)
    SORTED_LDS_PAD = 16000     # residency cap of the sorted multinomial's table kernels (they wait on memory)

    def __init__(self, init, step, n_particles: int, T: int, obs_addr="y", resample="systematic",
                 step_extra=None, specialize=True, rejuvenate=None, state_addr="x", noise_ahead=None, chain_mh=True,
                 noise_roots=None, fuse_resample=None, history=False):
        """chain_mh=False keeps the MH move and the extension as two launches (the form a chained program too large
        for the tile statistics falls back to); noise_roots: which keys' draws of the chained program the background
        stream takes ("LDKEY" = the move's proposal + accept draws, the default; "KSPLITU" = the extension's; "all").
        rejuvenate: an edit request (e.g. StaticRequest({"x": Rejuvenate(...)})) applied as one fused
        MH move per particle after every resampling, before the next extension (BASELINE config 3; the
        graph-captured form of smc.resample -> smc.rejuvenate -> smc.extend, same keys, same results).
        Supported for models whose trace is {state_addr: the return value, obs_addr: the observation}.
        history=True keeps EVERY step's particles, log-weights and ancestors (one gmx_history_record launch per step on
        the chain's stream, inside a captured graph too) — `history()` gives the per-step filtering distribution and the
        ancestral lineage of the survivors (SweepHistory).  Off: nothing is allocated, nothing is launched."""
        self.init, self.step, self.n, self.T = init, step, int(n_particles), int(T)
        self.keep_history = bool(history)
        if self.keep_history and rejuvenate is not None:
            raise NotImplementedError("BootstrapSweep(history=True, rejuvenate=...): the trajectory's state would be the "
                                      "moved state, which is not recorded yet (drop rejuvenate= or history=)")
        self.obs_addr, self.state_addr, self.rejuvenate = obs_addr, state_addr, rejuvenate
        self.kind = _KINDS[resample] if isinstance(resample, str) else int(resample)
        self.step_extra = step_extra or (lambda t: ())
        self.specialize = specialize
        self.noise_ahead_req = noise_ahead
        self.chain_mh = bool(chain_mh)
        self.noise_roots = noise_roots or self.NOISE_ROOTS_MH
        # ONE launch per step (None: when it applies): the program that gathers the resampled state first resamples the
        # previous step itself — its workgroup's tile of k_offspring_tile, ancestors as tagged words its neighbours poll
        # (include/genmi.h: gmx_run_args.rs) — so only the grid-wide dependency (the tile statistics) still needs a
        # launch boundary.  Systematic resampling, n <= 2^20, specialised programs.
        self.fuse_req = fuse_resample

    def prepare(self, key: Key, ys: torch.Tensor):
        be = _lib.get()
        # a sweep object may be prepared again (another key, other observations): nothing bound for the previous run
        # survives — the background launches' key rows in particular (found by the unbiasedness test on the GPU: a
        # second prepare() replayed the first run's noise launches)
        self.__dict__.pop("_noise_run_cache", None)
        self._drop_graph()                   # a graph captured for the previous run holds its launch arguments
        # noise ahead: asked for explicitly, or by default on a device with streams on the fast path (specialised
        # programs; with rejuvenate=, the MH move chained into the extension)
        fuse_mh_ok = self.chain_mh
        want_na = self.noise_ahead_req
        if want_na is None:
            want_na = (os.environ.get("GENMI_NOISE_AHEAD", "1") != "0" and be.uses_streams and self.specialize
                       and (self.rejuvenate is None or fuse_mh_ok))
        if want_na and self.rejuvenate is not None and not fuse_mh_ok:
            raise NotImplementedError("BootstrapSweep(noise_ahead=True, rejuvenate=...) needs the chained MH + extension "
                                      "program (chain_mh=False)")
        self.noise_ahead = False
        self._noise_progs = {}
        n, T = self.n, self.T
        dev = be.device
        self.key = key
        self._set_observations(ys)
        assert self.ys.numel() >= T
        self.lw = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.anc = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.maxs = torch.zeros((T,), dtype=torch.float32, device=dev)
        self.totals = torch.zeros((T,), dtype=torch.int64, device=dev)
        self.shift = cdf_shift(n)
        # fused: the resampler works from tile statistics, no CDF array (the launcher itself is built below, once it is
        # known whether the site programs leave the statistics)
        self.fused = _Resampler.form_of(self.kind, n, sweep=True) == "tiles"
        self.fuse = False
        self.batch, self.index = n, self.anc
        self._build_init(bool(want_na))
        # the state is the model's return value, stored struct-of-arrays as [D, n] and seen by models (and by state())
        # as the [n] / [n, D] / tuple-of-rows view
        self.store = _StateStore(self.p_init, n, "BootstrapSweep")
        self.tuple_state, self.event, D = self.store.tuple_state, self.store.event, self.store.D
        hn = False
        if self.rejuvenate is not None:
            if self.tuple_state is not None:
                raise NotImplementedError("BootstrapSweep(rejuvenate=...): a tuple state is not supported (return one "
                                          "array, or use smc.resample / rejuvenate / extend under smc.capture)")
            # store t % 2 of `moved`: the MH-moved, resampled state the extension of step t starts from
            self.moved = _StateStore(self.p_init, n, "BootstrapSweep")
            self.accept = torch.zeros((n,), dtype=torch.bool, device=dev)
            # which draws of the chained program go to the background stream: the two streams should carry about the
            # same vector work (noise_roots: "all", "LDKEY" = the move's proposal + accept draws, "KSPLITU" = the
            # extension's draw)
            roots = self.noise_roots
            hn = False if not want_na else (True if roots == "all" else tuple(roots.split(",")))
        # (with rejuvenate=, the extension alone, p_step, draws in place whatever the chained program does)
        self._build_steps(bool(want_na), False, chain=self.chain_mh, chain_hoist=hn)
        # the chain's programs by step: t = 0, t = 1, t >= 2
        chain_progs = (self.p_init, self.p_step, self.p_step) if self.rejuvenate is None else \
            (self.p_init, self.p_mhvm_init, self.p_mhvm_step)
        if want_na and chain_progs[2] is not None and chain_progs[2].noise:
            self._noise_setup(chain_progs, n, T, dev)
        elif want_na and any(P is not None and P.noise for P in chain_progs):
            # the steady-state program draws nothing ahead although another one would: the plain programs throughout
            self.noise_ahead_req = False
            return self.prepare(key, ys)
        want_fuse = self.fuse_req
        if want_fuse is None:
            want_fuse = be.uses_streams
        # past 2^21 particles the standalone tile-form resamplers do not apply (RS_MAX_TILES) — the LAST step of a sweep is
        # resampled through the CDF array there — but the looped resample-first launch does (up to 2^24): the steps in
        # between stay ONE launch each
        self.big = bool(self.kind == SYSTEMATIC and not self.fused and n <= FUSE_RESAMPLE_LOOP_MAX)
        want_fuse = bool(want_fuse and self.specialize and self.kind == SYSTEMATIC and (self.fused or self.big)
                         and n <= FUSE_RESAMPLE_LOOP_MAX)
        if self.rejuvenate is None:
            gatherers = (self.p_step,)
        elif self.p_mhvm_init is not None:
            gatherers = (self.p_mhvm_init, self.p_mhvm_step)
        else:
            gatherers = ()
        if want_fuse:
            for p_ in gatherers:
                if not p_.comp.is_specialized():
                    # (past 2^20 particles the workgroups of ONE launch are not all resident: each walks several tiles)
                    # (the looped form at 1e6 particles, by workgroup count, was measured and is slower than one tile per
                    #  workgroup: profiles/r06d_loop_grid.txt — 14.2 us/step plain, 14.9 looped at 1024, 17.4 at 512)
                    p_.comp.set_fuse_resample(loop=n > FUSE_RESAMPLE_MAX)
        if self.specialize:
            self.p_init.comp.specialize()
            self.p_step.comp.specialize()
            if self.rejuvenate is not None:
                self.p_mh_init.comp.specialize()
                self.p_mh_step.comp.specialize()
            if self.p_mhvm_init is not None:
                self.p_mhvm_init.comp.specialize()
                self.p_mhvm_step.comp.specialize()
        # block partials: sized for the interpreter's one row per 256 particles; a specialised kernel
        # writes fewer rows (gmx_program_grid), asked per launch in _rows()
        self.partials = torch.zeros((2, (n + 255) // 256), dtype=torch.float32, device=dev)
        # two launches per step: when the site programs can leave the CDF tile statistics themselves (specialised,
        # 4 particles per thread: a workgroup is one 1024-particle tile) the resampler needs no pass of its own
        # over the log-weights (gmx_resample_tiles); programs that cannot (interpreted) get a gmx_tile_stats launch
        self.tile_agg = torch.zeros(((n + 1023) // 1024,), dtype=torch.int64, device=dev)
        self.tile_stats = bool((self.fused or (self.big and want_fuse)) and self.p_init.comp.writes_tile_stats()
                               and self.p_step.comp.writes_tile_stats())
        if self.p_mhvm_init is not None and self.tile_stats and not (self.p_mhvm_init.comp.writes_tile_stats()
                                                                     and self.p_mhvm_step.comp.writes_tile_stats()):
            self.p_mhvm_init = self.p_mhvm_step = None      # the chained programs are too large for the tile form
        self.fuse_mh = self.p_mhvm_init is not None
        self.resampler = _Resampler(self.kind, n, sweep=True, with_stats=self.tile_stats)
        self.ws = self.resampler.cdf_ws
        if self.noise_ahead and self.rejuvenate is not None and not self.fuse_mh:
            # the noise-ahead form needs the chained program: start over with the plain ones
            if self.noise_ahead_req:
                raise NotImplementedError("BootstrapSweep(noise_ahead=True, rejuvenate=...): the chained MH + extension "
                                          "program does not fit the tile form")
            self.noise_ahead_req = False
            return self.prepare(key, ys)
        # ONE launch per step where the gathering programs can resample first: two sets of log-weights / statistics (a
        # launch reads step t-1's while it writes step t's)
        # ... and where the device holds every workgroup of such a launch at once (they wait for each other): asked of
        # the runtime per code object (engine.Compiled.resident_particles), two launches per step otherwise
        self.fuse = bool(want_fuse and self.tile_stats and gatherers and (self.rejuvenate is None or self.fuse_mh)
                         and all(p_.comp.fuses_resample() and p_.comp.resident_particles() >= n for p_ in gatherers))
        if self.fuse_req and not self.fuse:
            raise NotImplementedError("BootstrapSweep(fuse_resample=True): needs specialised 4-particles-per-thread programs "
                                      "that gather, systematic resampling and n <= 2^20")
        if self.fuse:
            self.lw_pp = [self.lw, torch.zeros_like(self.lw)]
            self.partials_pp = [self.partials, torch.zeros_like(self.partials)]
            self.tile_agg_pp = [self.tile_agg, torch.zeros_like(self.tile_agg)]
            self.rs_status = torch.zeros((1,), dtype=torch.int64, device=dev)
        else:
            self.lw_pp, self.partials_pp, self.tile_agg_pp = [self.lw] * 2, [self.partials] * 2, [self.tile_agg] * 2
        self._set_step_keys(key)
        self._slot_uniforms_setup()
        self.hist_xs = self.hist_lws = self.hist_ancs = self.hist_status = None
        if self.keep_history:
            # row t of each slab: step t's particles [D, n] / log-weights / ancestors (the resampling AFTER step t)
            self.hist_xs = torch.zeros((T, D, n), dtype=torch.float32, device=dev)
            self.hist_lws = torch.zeros((T, n), dtype=torch.float32, device=dev)
            self.hist_ancs = torch.zeros((T, n), dtype=torch.int32, device=dev)
            self.hist_status = torch.zeros((1,), dtype=torch.int64, device=dev)
        return self

    def _record(self, t, tagged=False):
        """Step t into the history slabs (gmx_history_record), enqueued at the one point where its state x_store[t % 2],
        its log-weights and its ancestors are all in place: right after step t's resampler — which, in the one-launch
        form, is the prologue of step t + 1's launch (tagged=True: `anc` then holds that launch's tagged words, tag
        1 + t % 255 as in _resample_in(t + 1); the record stores the indices and counts any word with another tag) —
        and before the launch of step t + 2 overwrites the first two."""
        be = _lib.get()
        w = t % 2 if self.fuse else 0
        tag = 1 + t % _lib.ANC_TAG_MAX if tagged else 0
        be.check(be.c.gmx_history_record(be.ptr(self.store.rows[t % 2]), self.store.D, be.ptr(self.lw_pp[w]),
                                         be.ptr(self.anc), self.n, tag, be.ptr(self.hist_xs[t]), be.ptr(self.hist_lws[t]),
                                         be.ptr(self.hist_ancs[t]), be.ptr(self.hist_status), be.stream()),
                 "gmx_history_record")

    chained = property(lambda self: self.fuse_mh)

    def _launch_step(self, t, skip_vm=False, alone=False):
        """step t's programs (_programs) with what is the single-GPU sweep's own: the log-weights and block maxima of set
        t % 2 (the one-launch form alternates two), the tile statistics, and — a one-launch step that gathers — the
        resampling of step t - 1 as its prologue.  skip_vm: the separate MH move only; alone: the extension only."""
        n = self.n
        mh, prog, leaves, key, bufs = self._programs(t, alone)
        if mh is not None:
            mprog, mleaves, mkey, mbufs = mh
            mprog.comp.run(mleaves, (n,), lazy_split(mkey, n), out_buffers=mbufs)
        if skip_vm:
            return
        w = t % 2 if self.fuse else 0
        bufs[prog.wo[1]] = self.lw_pp[w].reshape(1, n)
        gathers = t >= 1 and (self.rejuvenate is None or not alone)
        prog.comp.run(leaves, (n,), lazy_split(key, n), red_out=self.partials_pp[w], out_buffers=bufs,
                      tile_stats=(self.tile_agg_pp[w], self.shift) if self.tile_stats else None,
                      resample_in=self._resample_in(t) if (self.fuse and gathers) else None)

    def _resample_in(self, t):
        """gmx_run_args.rs of the launch of step t (>= 1) that gathers: resample step t-1's weights first"""
        kh = self.step_keys[t - 1][1].host()
        w = (t - 1) % 2
        return dict(lw=self.lw_pp[w], tile_max=self.partials_pp[w], tile_agg=self.tile_agg_pp[w], shift=self.shift,
                    key=(int(kh[0]), int(kh[1])), tag=1 + (t - 1) % _lib.ANC_TAG_MAX, max_out=self.maxs[t - 1:t],
                    total_out=self.totals[t - 1:t], status=self.rs_status)

    def _rows(self, t) -> int:
        """partial rows the site program of step t wrote"""
        return int(_lib.get().c.gmx_program_grid(self._chain_prog(t).comp.handle, self.n))

    def _slot_uniforms_setup(self):
        """Stratified resampling draws one uniform per SLOT, keyed by the step's resampling key and the slot number —
        nothing the chain produces.  In the noise-ahead form they are drawn on the background stream with the steps'
        normals (gmx_slot_uniforms, one 2-D launch per group of steps) and the resampler reads them
        (gmx_resample_tiles_u): the same ancestors, one Threefry block per slot-edge evaluation less on the chain
        (the one-stream form draws them inside the resampler)."""
        self._u_ring = None
        if not (self.noise_ahead and self.kind in (STRATIFIED, MULTINOMIAL_TILED, MULTINOMIAL_SORTED) and self.fused
                and self.tile_stats):
            return
        dev = self.zbuf.device
        # (the sorted multinomial's row is its whole order-statistics table: gmx_sorted_uniforms_words(n) words)
        row_words = int(_lib.get().c.gmx_sorted_uniforms_words(self.n)) if self.kind == MULTINOMIAL_SORTED else self.n
        self._u_ring = torch.zeros((self.noise_ring, self.noise_group, row_words), dtype=torch.int32, device=dev)
        self._u_keys = []
        for t0, t1 in self.noise_groups:
            # stratified: the resampling key itself; the two-stage multinomial: its first child (stage 1's key)
            rk = (lambda t: split(self.step_keys[t][1], 2)[0]) if self.kind == MULTINOMIAL_TILED else (lambda t: self.step_keys[t][1])
            ks = np.stack([rk(t).host() for t in range(t0, t1)]).astype(np.uint32)
            self._u_keys.append(torch.from_numpy(ks.view(np.int32)).to(dev))
        self._u_pad = int(self.NOISE_LDS_PAD)
        if self.kind == MULTINOMIAL_SORTED:       # its two kernels wait on memory, not on the vector ALUs: more of them per CU
            self._u_pad = self.SORTED_LDS_PAD

    def _launch_group_extras(self, g):
        if self._u_ring is None:
            return
        be = _lib.get()
        t0, t1 = self.noise_groups[g]
        half, row = self.noise_slot[t0]
        if self.kind == MULTINOMIAL_SORTED:
            be.check(be.c.gmx_sorted_uniforms(be.ptr(self._u_keys[g]), t1 - t0, self.n,
                                              be.ptr(self._u_ring[half, row:row + (t1 - t0)]), self._u_pad, be.stream()),
                     "gmx_sorted_uniforms")
            return
        be.check(be.c.gmx_slot_uniforms(be.ptr(self._u_keys[g]), t1 - t0, self.n, be.ptr(self._u_ring[half, row:row + (t1 - t0)]),
                                        self._u_pad, be.stream()), "gmx_slot_uniforms")

    def _resample(self, t, cdf_only=False, cdf_ready=False):
        """step t's resampler: the launcher's call on the persistent buffers (ancestors into `anc`, the evidence terms
        into maxs[t] / totals[t]); cdf_only / cdf_ready: one half of the CDF-array form (kernel_timers)"""
        rs = self.resampler
        w = t % 2 if self.fuse else 0          # (a one-launch sweep alternates two sets of log-weights / partials)
        lw, partials, tile_agg = self.lw_pp[w], self.partials_pp[w], self.tile_agg_pp[w]
        stats = None
        if self.tile_stats:        # tile maxima = the workgroup maxima the site program left in partials[0]
            stats = (partials, tile_agg)
        elif rs.needs_stats(rs.kind, rs.form):
            stats = (partials, tile_agg)
            _tile_stats(lw, self.shift, *stats)
        uniforms = None
        if self._u_ring is not None:           # drawn ahead on the background stream
            half, row = self.noise_slot[t]
            uniforms = self._u_ring[half, row]
        rows = 0
        if (rs.form == "cdf" and not cdf_ready) or (rs.form == "tiles" and stats is None):
            rows = self._rows(t)               # gmx_weight_cdf / gmx_resample reduce the site program's block maxima
        rs.launch(self.step_keys[t][1], lw, self.maxs[t:t + 1], self.totals[t:t + 1], None if cdf_only else self.anc,
                  stats=stats, uniforms=uniforms, partials=partials, rows=rows,
                  phase=-1 if t == 0 else (t & 1),       # count buffers alternate: one memset per sweep
                  cdf_ready=cdf_ready)

    def _chain_step(self, t, skip_vm=False):
        """everything step t launches on the chain: [the MH move], site program', then the resampler"""
        separate_mh = t >= 1 and self.rejuvenate is not None and not self.fuse_mh
        if separate_mh or not skip_vm:            # (the move as a launch of its own — one-stream form only — is not
            self._launch_step(t, skip_vm)         #  part of skip_vm)
        if not skip_vm:
            if self.keep_history and self.fuse and t >= 1:
                self._record(t - 1, tagged=True)      # (this launch's prologue resampled step t - 1)
        if self.fuse and t < self.T - 1:
            return                         # step t's weights are resampled by step t + 1's launch itself
        self._resample(t)
        if self.keep_history:
            self._record(t)

    def enqueue(self, skip_vm=False):
        """Issue every launch of the sweep on the current stream (no syncs, no allocations).
        skip_vm=True leaves the site-program launches out (the resampling kernels then run on the
        previous sweep's log-weights): bench.py times that variant to get the site program's cost
        IN the sweep as a difference."""
        if self.noise_ahead:
            return self._enqueue_noise_ahead(skip_vm)
        for t in range(self.T):
            self._chain_step(t, skip_vm)

    def kernel_timers(self):
        """Representative single launches (a mid-sweep step) for per-kernel timing in bench.py."""
        t = max(1, self.T // 2)
        out = {"k_vm": lambda: self._launch_step(t, alone=True)}
        if self.noise_ahead:
            out["k_noise"] = lambda: self._launch_noise(t)
        if self.fuse:
            pass                           # (the resampler is the prologue of k_vm's launch)
        elif self.fused and self.tile_stats:
            out["k_offspring_tile"] = lambda: self._resample(t)
        elif self.fused:
            out["resample(k_tile_stats+k_offspring_tile)"] = lambda: self._resample(t)
        else:
            out["k_weight_cdf"] = lambda: self._resample(t, cdf_only=True)
            out["k_ancestors"] = lambda: self._resample(t, cdf_ready=True)
        return out

    def _check_valid(self):
        """the fused resampling prologue's sticky timeout word: a workgroup that gave up waiting clamps stale words into
        indices, so nothing of such a sweep may be read.  The word is STICKY for the object's lifetime (nothing in the
        captured sweep clears it: one timed-out poll condemns every later replay until `reset_status()`), which is the
        safe side: a launch that was not resident once will not be the next time either"""
        if self.fuse and int(self.rs_status.item()) != 0:
            raise RuntimeError("BootstrapSweep: a workgroup's wait for its ancestors timed out (the launch was not "
                               "resident at once?): the sweep's results are not valid")

    def reset_status(self):
        """clear the sticky timeout word (after the cause — e.g. another process holding compute units — is gone)"""
        if getattr(self, "rs_status", None) is not None:
            self.rs_status.zero_()
        if getattr(self, "hist_status", None) is not None:
            self.hist_status.zero_()

    def history(self) -> "SweepHistory":
        """Every step of the last launch (BootstrapSweep(history=True); synchronises): views of the history slabs — the
        next launch() overwrites them."""
        if not self.keep_history:
            raise RuntimeError("BootstrapSweep.history(): the sweep was built without history=True")
        self._check_valid()
        if int(self.hist_status.item()) != 0:
            raise RuntimeError("BootstrapSweep.history(): a recorded ancestor word carried another step's tag (a stale "
                               "word of the fused resampling prologue): the history is not valid")
        return SweepHistory(self.hist_xs, self.hist_lws, self.hist_ancs, self.event, self.tuple_state, step=self.step,
                            ys=self.ys, step_extra=self.step_extra, obs_addr=self.obs_addr, state_addr=self.state_addr)

    def log_ml(self) -> float:
        """sum_t [ ref(M_t) + log(total_t * 2^-shift) - log N ] in float64 (synchronises)."""
        self._check_valid()
        terms = evidence_terms(self.maxs.cpu().numpy(), self.totals.cpu().numpy(), self.shift, self.n)
        if np.any(np.isneginf(terms)):   # a step where no particle carried any mass
            return -math.inf
        return float(np.sum(terms))

    def state(self):
        """(x_T particles before the last resampling, log-weights, last ancestors)."""
        self._check_valid()
        return self.store.view((self.T - 1) % 2), self.lw_pp[(self.T - 1) % 2 if self.fuse else 0], self.anc


class BootstrapBank(_Sweep):
    """R independent bootstrap particle filters of n particles each as ONE chain of launches (the reference's
    `jax.vmap(smc_run)(keys)`: replicate keys for the variance of the evidence estimate, a grid or a chain over model
    parameters): per step ONE site program over the R * n particles and ONE gmx_resample_rows call (every row under its
    own key, n <= 1024: a single launch), no host read of a device value in between — the whole sweep is capturable.

    Key schedule: row r follows BootstrapSweep's under keys[r] — step key = fold_in(keys[r], t); (k_prop, k_res, _) =
    split(step key, 3); particle i of the row draws under split(k_prop, n)[i] (derived in the program from the row's key:
    GMX_KEY_ROWSPLIT, no key launch); the row is resampled under k_res.  The T x R proposal / resampling keys are
    derived on the host and uploaded once by prepare().

    Contract: row r of state() and log_ml()[r] equal, bit for bit, what BootstrapSweep(init, step, n, T, ...).prepare(
    keys[r], ys) gives launched on its own.

    The programs are built as the sweep builds them (static.MinimalGenerate), over the flat R * n particle axis; the
    next step gathers through GLOBAL ancestors (gmx_resample_rows with index_stride = n) over the flat state store.
    `params`: a tuple of float32 [R] tensors, one value per filter; the models are called as init(*params_r) and
    step(x_prev, *step_extra(t), *params_r).  Each is expanded ONCE, in prepare(), to a persistent [R * n] per-particle
    leaf (4 bytes per particle and parameter read by every step; nothing is launched for it inside the sweep) — the
    engine's launch-uniform leaves have no per-row form.  ys: [T], shared by the filters.

    ess_threshold=tau (None: every row is resampled at every step, the sweep above launch for launch): ADAPTIVE
    resampling, decided per filter and per step inside the row resampler's one launch (gmx_resample_rows_ess, n <= 1024).
    Row r is resampled after step t only when the effective sample size of its accumulated weights is below tau * n — an
    exact integer predicate on the fixed-point weights, ess_q8 = min(ceil(tau * n * 256), 256 n + 1) computed on the host:
    tau = 0 never resamples, tau > 1 (or inf) always does, and is then bit for bit the sweep without the argument.  A row
    that is not resampled keeps its particles (identity ancestors) and carries its log-weights into the next step, where
    the new observation weights are added to them; state() returns these ACCUMULATED log-weights and resampled() the
    [T, R] table of decisions.  log_ml()[r] sums the evidence terms of the steps after which row r was resampled, and of
    step T - 1 always.  This is the unbiased estimate: between two resamplings a particle's weight is the unnormalised
    PRODUCT of its incremental weights, so its mean over the row at the next resampling (or at the end) estimates the
    ratio of normalisers across the whole stretch at once, and the product of those means over the stretches — each
    started from an equally weighted population — is the usual product-form estimate of Z (Del Moral, Doucet & Jasra
    2012, section 2); a skipped step's own term is already inside the next counted one."""

    def __init__(self, init, step, n_particles: int, n_filters: int, T: int, obs_addr="y", resample="systematic",
                 step_extra=None, params=None, specialize=True, state_addr="x", rejuvenate=None, history=False,
                 noise_ahead=None, fuse_resample=None, comm=None, ess_threshold=None):
        for name, given in (("rejuvenate=", rejuvenate is not None), ("history=", bool(history)),
                            ("noise_ahead= (the background noise stream)", bool(noise_ahead)),
                            ("fuse_resample= (the one-launch fused step)", bool(fuse_resample)),
                            ("comm= (sharding over several GPUs)", comm is not None)):
            if given:
                raise NotImplementedError(f"BootstrapBank: {name} is not supported (use BootstrapSweep per filter)")
        self.init, self.step = init, step
        self.n, self.R, self.T = int(n_particles), int(n_filters), int(T)
        if self.n < 1 or self.R < 1 or self.T < 1:
            raise ValueError("BootstrapBank: n_particles, n_filters and T must be positive")
        self.kind = _row_kind(resample, "BootstrapBank(resample=)")
        if self.n > ROWS_N_MAX:
            raise NotImplementedError(f"BootstrapBank: n_particles = {self.n} > 2^21 (gmx_resample_rows)")
        if self.R * self.n >= 2 ** 31:
            raise NotImplementedError(f"BootstrapBank: R * n >= 2^31 (R = {self.R}, n = {self.n}): the ancestors index the "
                                      "flat [R * n] store in int32")
        self.obs_addr, self.state_addr = obs_addr, state_addr
        self.step_extra = step_extra or (lambda t: ())
        self.params = tuple(params) if params is not None else ()
        self.specialize = specialize
        self.ess_threshold, self.ess_q8 = None, None
        if ess_threshold is not None:
            tau = float(ess_threshold)
            if math.isnan(tau) or tau < 0.0:
                raise ValueError(f"BootstrapBank(ess_threshold={ess_threshold!r}): a fraction of n, >= 0 (above 1, or inf: always)")
            if self.n > ROWS_ESS_N_MAX:
                raise NotImplementedError(f"BootstrapBank(ess_threshold=): n_particles = {self.n} > {ROWS_ESS_N_MAX} "
                                          "(gmx_resample_rows_ess decides on the weights of a row of one tile)")
            always = 256 * self.n + 1
            self.ess_threshold = tau
            self.ess_q8 = always if tau > 1.0 else min(int(math.ceil(tau * self.n * 256)), always)

    def _key_tables(self, keys: Key, third=False):
        """the key schedule of every row, on the host: [T, R, 2] proposal keys and [T, R, 2] resampling keys (int32 words);
        third=True: also the [T, R, 2] table of the step key's third child (ConditionalBank's ancestor draws)"""
        from ..random import _derive_host
        R, T = self.R, self.T
        kh = np.asarray(keys.host(), dtype=np.uint32).reshape(R, 2)
        prop, res, last = (np.empty((T, R, 2), np.uint32) for _ in range(3))
        for t in range(T):
            ks = _derive_host(_derive_host(kh, np.uint64(t))[:, None, :], np.arange(3, dtype=np.uint64))
            prop[t], res[t], last[t] = ks[:, 0], ks[:, 1], ks[:, 2]
        if third:
            return prop.view(np.int32), res.view(np.int32), last.view(np.int32)
        return prop.view(np.int32), res.view(np.int32)

    def prepare(self, keys: Key, ys: torch.Tensor):
        be = _lib.get()
        self._drop_graph()
        R, n, T = self.R, self.n, self.T
        N = R * n
        dev = be.device
        if tuple(keys.shape) != (R,):
            raise ValueError(f"BootstrapBank.prepare: {R} filters need keys of shape {(R,)}, got {tuple(keys.shape)}")
        ys = torch.as_tensor(ys)
        if ys.ndim != 1:
            raise NotImplementedError(f"BootstrapBank.prepare: per-filter observations (ys of [R, T]; got "
                                      f"{tuple(ys.shape)}) are not supported: ys is [T], shared by the filters")
        self.keys = keys
        self._set_observations(ys)
        assert self.ys.numel() >= T
        prop, res = self._key_tables(keys)
        self.keys_prop = torch.from_numpy(prop).to(dev)
        self.keys_res = torch.from_numpy(res).to(dev)
        self.lw = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.anc = torch.zeros((R, n), dtype=torch.int32, device=dev)          # indices into the flat [R * n] store
        self.maxs = torch.zeros((T, R), dtype=torch.float32, device=dev)
        self.totals = torch.zeros((T, R), dtype=torch.int64, device=dev)
        self.status = torch.zeros((1,), dtype=torch.int64, device=dev)         # rows without mass, over the last sweep
        self.shift = cdf_shift(n)
        self.ws = torch.zeros(((int(be.c.gmx_resample_rows_workspace(self.kind, R, n)) + 7) // 8,), dtype=torch.int64, device=dev)
        if self.ess_q8 is not None:
            self.carry = torch.zeros((N,), dtype=torch.float32, device=dev)    # log-weights since the row's last resampling
            self.flags = torch.zeros((T, R), dtype=torch.int32, device=dev)    # was row r resampled after step t
        self.params_full = []
        for p in self.params:
            p = torch.as_tensor(p)
            if tuple(p.shape) != (R,):
                raise ValueError(f"BootstrapBank: params are [R] = {(R,)} tensors, one value per filter; got {tuple(p.shape)}")
            self.params_full.append(p.to(dev).float().reshape(R, 1).expand(R, n).contiguous().reshape(N))
        # particle i of row r draws under split(k_prop[r], n)[i]: derived in the program from the row's key
        self.step_keys = [(Key(lazy=("rowsplit", Key(dev=self.keys_prop[t]), n)), self.keys_res[t], None) for t in range(T)]
        self.batch, self.index, self.tail = N, self.anc.reshape(-1), tuple(self.params_full)
        self._build_init()
        self.store = _StateStore(self.p_init, N, "BootstrapBank")
        self.tuple_state, self.event = self.store.tuple_state, self.store.event
        self._build_steps()
        if self.specialize:
            self.p_init.comp.specialize()
            self.p_step.comp.specialize()
        self.partials = torch.zeros((2, (N + 255) // 256), dtype=torch.float32, device=dev)
        return self

    def _resample(self, t):
        if self.ess_q8 is not None:
            return self._resample_adaptive(t)
        resample_rows(self.kind, self.step_keys[t][1], self.lw.reshape(self.R, self.n), index_stride=self.n,
                      out=(self.anc, self.totals[t], self.maxs[t], self.status), workspace=self.ws)

    def _resample_adaptive(self, t):
        """lw += carry; every row whose integer ESS is below the threshold resampled, the others carried (one launch)"""
        be = _lib.get()
        R, n = self.R, self.n
        be.check(be.c.gmx_resample_rows_ess(self.kind, be.ptr(self.step_keys[t][1]), be.ptr(self.lw), be.ptr(self.carry), R, n,
                                            n, n, self.ess_q8, be.ptr(self.maxs[t]), be.ptr(self.totals[t]),
                                            be.ptr(self.flags[t]), be.ptr(self.anc), be.ptr(self.status), be.ptr(self.ws),
                                            be.stream()), "gmx_resample_rows_ess")

    def enqueue(self):
        """every launch of the sweep on the current stream: per step the site program and gmx_resample_rows (with
        ess_threshold=: gmx_resample_rows_ess) — no syncs, no allocations, no host read of a device value"""
        N = self.R * self.n
        self.status.zero_()
        if self.ess_q8 is not None:
            self.carry.zero_()
        for t in range(self.T):
            _mh, prog, leaves, key, bufs = self._programs(t)
            bufs[prog.wo[1]] = self.lw.reshape(1, N)
            prog.comp.run(leaves, (N,), key, red_out=self.partials, out_buffers=bufs)
            self._resample(t)

    def log_ml(self) -> np.ndarray:
        """float64 [R]: row r is BootstrapSweep.log_ml() of that filter — sum_t [ ref(M_t) + log(total_t 2^-shift) - log n ]
        from the [T, R] evidence terms, finished in float64 on the host (synchronises).  With ess_threshold=: the terms of
        the steps after which row r was resampled, and of step T - 1 always (the class docstring says why), in the same
        order; with every row resampled at every step that is the same float."""
        terms = evidence_terms(self.maxs.cpu().numpy(), self.totals.cpu().numpy(), self.shift, self.n)      # [T, R]
        counted = np.ones((self.T, self.R), dtype=bool)
        if self.ess_q8 is not None:
            counted = self.resampled().numpy().copy()
            counted[self.T - 1] = True
        out = np.empty((self.R,), dtype=np.float64)
        for r in range(self.R):
            tr = np.ascontiguousarray(terms[:, r][counted[:, r]])
            # (-inf: a step where no particle of the row carried any mass)
            out[r] = -math.inf if np.any(np.isneginf(tr)) else float(np.sum(tr))
        return out

    def resampled(self) -> torch.Tensor:
        """bool [T, R], on the host: was row r resampled after step t in the last sweep (ess_threshold= only; synchronises)"""
        if self.ess_q8 is None:
            raise ValueError("BootstrapBank.resampled: without ess_threshold= every row is resampled at every step")
        return self.flags.cpu() != 0

    def state(self):
        """(x_T before the last resampling: [R, n], [R, n, D] or a tuple of [R, n]; log-weights [R, n] — with
        ess_threshold=, accumulated since the row's last resampling; the last ancestors, int32 [R, n], row-local)"""
        R, n = self.R, self.n
        x = self.store.per_filter((self.T - 1) % 2, R, n)
        local = self.anc - (torch.arange(R, dtype=torch.int32, device=self.anc.device) * n).reshape(R, 1)
        return x, self.lw.reshape(R, n), local


class ConditionalBank(BootstrapBank):
    """R independent CONDITIONAL bootstrap particle filters of n particles each (conditional SMC, the kernel of particle
    Gibbs: Andrieu, Doucet & Holenstein 2010) as one chain of launches: BootstrapBank's programs, stores and key schedule,
    with slot n - 1 of every chain pinned to a retained trajectory — at every step t it holds the retained state
    ref_x[t, :, r] and its observation weight ref_lw[t, r], and it always descends from slot n - 1; the other n - 1 slots
    are resampled as usual (gmx_resample_rows_pinned: n <= 1024, one launch per step).  Every step is recorded
    (gmx_history_record over the flat R * n particles), so a new trajectory per chain is one exact-integer draw from the
    final weights (gmx_pick_rows) and one walk through the recorded ancestors (gmx_lineage).

    Resampling is the iid multinomial, fixed: its slots are independent, so "draw the other slots as always, force the last
    one" IS the conditional resampling distribution.  Forcing a slot of a systematic, stratified or ordered scheme is not
    a valid conditional draw; those kinds are refused by name.

    With nothing retained a sweep is, row for row and bit for bit, BootstrapBank(resample="multinomial") under the same
    keys (plain gmx_resample_rows), recorded.

      cb.prepare(keys, ys, retained=None)   keys (R,), ys [T]; every buffer is allocated here
      cb.launch()                           one sweep (the captured graph when there is one)
      traj = cb.draw(key)                   ONE key: one trajectory per chain from the last sweep
      traj = cb.draw(key, backward=True)    ... by backward simulation over the recorded steps (below)
      cb.retain()                           the last draw becomes the retained path (device copies, in place)
      cb.rekey(keys)                        a new (R,) key batch into the existing key tables, in place
      cb.set_retained(x_ref)                a caller's own path(s), in draw()'s layout; weights from the model
      cb.run(key, ys, iters, retained=None, backward=False)   the particle-Gibbs driver: [iters, R, T, ...]

    The recorded weight of a particle IS its observation weight under the same ys and params, so a retained path that came
    from a sweep needs no model evaluation.  log_ml() with a retained path is the CONDITIONAL sweep's normaliser estimate
    (the retained particle is in every step's sum), not the unbiased estimate of an unconditional filter.

    capture() fixes the form (conditional or not): going from "nothing retained" to "retained" drops the graph; rekey()
    and retain() on a captured conditional sweep only change buffer contents, which the graph reads when replayed.

    ancestor_sampling=True (particle Gibbs with ancestor sampling: Lindsten, Jordan & Schön 2014): at every step t < T - 1
    the pinned slot does not record itself as its ancestor but ONE draw among the chain's n step-t particles, particle i
    with probability proportional to exp(lw_t[i]) times the transition density from x_t[i] into the NEXT retained state
    ref_x[t + 1] — where the lineages coalesce, the new trajectory then leaves the retained one instead of repeating it.
    Only which ancestor the pinned slot records changes: particles, weights and every other ancestor are bit for bit those
    of ancestor_sampling=False under the same keys.  Row r's draw at step t is under the THIRD child of its step key.
    A conditional step t < T - 1 is then: the site program; gmx_rows_pin (the pins, and ref_x[t + 1] broadcast over each
    chain's particles); one per-particle program, the model's own `assess`,

        as_lw[i] = lw[i] + step.assess({state_sites[d]: next_x[d][i], obs_addr: y_{t+1}}, (x_t[i], *step_extra(t+1), *params[i]))[0]

    in float32 (the observation's term is constant along a chain and kept so that the bits are defined, as in
    SweepHistory.backward_sample); gmx_resample_rows_as (n <= 1024: one launch); gmx_history_record.  Step T - 1, and every
    step while nothing is retained, are the launches of ancestor_sampling=False.  It needs state_sites= when the state has
    more than one component, and a step model that samples nothing besides the state and the observation.  A chain whose
    ancestor logits carry no mass at some step keeps the plain pin there and is counted: draw() raises FloatingPointError.

    draw(key, backward=True) (particle Gibbs with backward simulation: Whiteley 2010; Lindsten & Schön 2013): the new
    trajectory is drawn by backward simulation over the recorded particle system instead of walking the recorded
    ancestors.  It is a choice made at draw time — any bank, ancestor_sampling or not, captured or not; the sweep keeps its
    launches — and it applies to the unconditional first sweep too (one FFBS draw per chain).  For ONE key and R chains:

        t = T-1:       row keys split(key, R)                 (draw()'s own: the last state equals draw(key)'s)
                       logits = hist_lws[T-1]
        t = T-2 .. 0:  row keys split(fold_in(key, t), R)
                       logits[i] = hist_lws[t][i] + step.assess({state_sites[d]: next[d][i], obs_addr: y_{t+1}},
                                                                (hist_x_t[i], *step_extra(t+1), *params[i]))[0]      (float32)
        every t:       gmx_pick_rows_take(keys_t, logits, R, n, n, hist_lws[t], n, hist_xs[t], D, R*n, n, index_stride = n,
                                          paths[t], lw_path[t], traj[t], next (null at t = 0), R*n, status[t], ...)

    `next` is the per-particle leaf the call of step t + 1 broadcast: chain r's chosen state on each of its particles.  The
    logits program is the ancestor-sampling one (same cache, same `specialize`); the observation's term is constant along
    a row and kept so that the bits are defined, as in SweepHistory.backward_sample.  The pins are in the record, so the
    retained particle is a candidate at every step.  Two launches per step for n <= 1024, nothing through the host between
    steps, one synchronisation at the end; the buffers (next [D, R * n], logits [R * n], status [T], the [T, R, 2] key
    table, the workspace) are allocated at the first backward draw and kept.  The recorded slabs, the ancestors, the
    sweep's status and a captured graph are not touched.  retain() takes a backward draw as it takes any other.  It needs
    state_sites= when the state has more than one component, and a step model that samples nothing besides the state and
    the observation.  A chain whose logits carry no mass at a step t < T - 1 raises FloatingPointError naming the latest
    such step and the count.

    Not here: rejuvenate=, noise ahead, the fused one-launch step, sharding, per-chain observations, ess_threshold=, more
    than one backward trajectory per chain.
    Memory: the history slabs take T * (D + 2) * R * n * 4 bytes; ancestor sampling adds (D + 1) * R * n * 4, a backward
    draw (D + 1) * R * n * 4."""

    def __init__(self, init, step, n_particles: int, n_chains: int, T: int, obs_addr="y", step_extra=None, params=None,
                 specialize=True, state_addr="x", state_sites=None, resample="multinomial", ancestor_sampling=False,
                 ess_threshold=None):
        if ess_threshold is not None:
            raise NotImplementedError("ConditionalBank: ess_threshold= is not supported (the pinned slot and the recorded "
                                      "history assume a resampling after every step; BootstrapBank takes it)")
        kind = _KINDS.get(resample, None) if isinstance(resample, str) else int(resample)
        if kind != MULTINOMIAL:
            name = resample if isinstance(resample, str) else next((k for k, v in _KINDS.items() if v == kind), resample)
            raise NotImplementedError(f"ConditionalBank(resample={name!r}): forcing a slot is only a valid conditional draw "
                                      "under iid multinomial resampling (resample=\"multinomial\", the only kind)")
        super().__init__(init, step, n_particles, n_chains, T, obs_addr=obs_addr, resample="multinomial",
                         step_extra=step_extra, params=params, specialize=specialize, state_addr=state_addr)
        self.state_sites = None if state_sites is None else tuple(state_sites)
        self.ancestor_sampling = bool(ancestor_sampling)
        self.conditional = False

    def prepare(self, keys: Key, ys: torch.Tensor, retained=None):
        super().prepare(keys, ys)
        be = _lib.get()
        dev = be.device
        R, n, T, D = self.R, self.n, self.T, self.store.D
        N = R * n
        self.D = D
        self.conditional = False
        self._last = None
        # the retained path in gmx_lineage's own `traj` layout (m = R), and its observation weights
        self.ref_x = torch.zeros((T, D, R), dtype=torch.float32, device=dev)
        self.ref_lw = torch.zeros((T, R), dtype=torch.float32, device=dev)
        # row t of each slab: step t's particles [D, N] / log-weights / FLAT ancestors (the resampling after step t)
        self.hist_xs = torch.zeros((T, D, N), dtype=torch.float32, device=dev)
        self.hist_lws = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.hist_ancs = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.hist_status = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.pick_ws = torch.zeros(((int(be.c.gmx_pick_rows_workspace(R, n)) + 7) // 8,), dtype=torch.int64, device=dev)
        self._views = SweepHistory(self.hist_xs, self.hist_lws, self.hist_ancs, self.event, self.tuple_state)
        if self.ancestor_sampling:
            self._prepare_ancestors(keys)
        if retained is not None:
            self.set_retained(retained)
        return self

    def _prepare_ancestors(self, keys):
        """what ancestor sampling adds to prepare(): the third key table, the ancestor logits, the broadcast next state, two
        status words, the wider workspace — and the logits program, built (and specialised) here"""
        be = _lib.get()
        dev = be.device
        R, n, T, D = self.R, self.n, self.T, self.D
        N = R * n
        sites = self.state_sites
        if sites is None:
            if D > 1:
                raise NotImplementedError("ConditionalBank(ancestor_sampling=True): a state of more than one component needs "
                                          "state_sites= (the address of each component, in order)")
            sites = (self.state_addr,)
        if len(sites) != D:
            raise ValueError(f"ConditionalBank(ancestor_sampling=True): state_sites names {len(sites)} addresses for a state "
                             f"of {D} components")
        self._as_sites = sites
        self.keys_as = torch.from_numpy(self._key_tables(keys, third=True)[2]).to(dev)
        self.as_lw = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.next_x = torch.zeros((D, N), dtype=torch.float32, device=dev)
        self.status = torch.zeros((2,), dtype=torch.int64, device=dev)       # rows without mass; rows without ancestor mass
        self.ws = torch.zeros(((max(int(be.c.gmx_resample_rows_as_workspace(R, n)),
                                    int(be.c.gmx_resample_rows_workspace(self.kind, R, n))) + 7) // 8,), dtype=torch.int64,
                              device=dev)
        if T > 1:
            self._ancestor_logits(0, launch=False)

    def _ancestor_logits(self, t, launch=True):
        """as_lw = lw + the transition (and observation) density of step t + 1 from every step-t particle into its chain's
        next retained state (next_x: gmx_rows_pin's broadcast)"""
        _ancestor_logits(self.step, self._as_sites, self.obs_addr, self.store.view(t % 2),
                         tuple(self.step_extra(t + 1)) + self.tail, list(self.next_x), self.ys[t + 1], self.lw,
                         self.as_lw.reshape(1, self.R * self.n), specialize=self.specialize, launch=launch)

    def _set_conditional(self, flag):
        if bool(flag) != self.conditional:
            self._drop_graph()             # a captured graph holds the launches of the other form
            self.conditional = bool(flag)

    def _resample(self, t):
        if not self.conditional:
            return super()._resample(t)
        if self.ancestor_sampling and t < self.T - 1:
            return self._resample_ancestors(t)
        resample_rows_pinned(self.step_keys[t][1], self.lw.reshape(self.R, self.n), self.ref_lw[t], self.ref_x[t],
                             self.store.rows[t % 2], index_stride=self.n, x_row_stride=self.n,
                             out=(self.anc, self.totals[t], self.maxs[t], self.status), workspace=self.ws)

    def _resample_ancestors(self, t):
        """a conditional step t < T - 1 under ancestor sampling: the pins and the next retained state over every particle
        (gmx_rows_pin), the ancestor logits (one program), the multinomial with slot n - 1 drawn from them
        (gmx_resample_rows_as)"""
        be = _lib.get()
        R, n, D = self.R, self.n, self.D
        N = R * n
        x = self.store.rows[t % 2]
        be.check(be.c.gmx_rows_pin(be.ptr(self.lw), R, n, n, be.ptr(self.ref_lw[t]), be.ptr(self.ref_x[t]), be.ptr(x), D,
                                   int(x.shape[1]), n, be.ptr(self.ref_x[t + 1]), be.ptr(self.next_x), N, be.stream()),
                 "gmx_rows_pin")
        self._ancestor_logits(t)
        be.check(be.c.gmx_resample_rows_as(be.ptr(self.step_keys[t][1]), be.ptr(self.lw), R, n, n, n, be.ptr(self.keys_as[t]),
                                           be.ptr(self.as_lw), n, be.ptr(self.maxs[t]), be.ptr(self.totals[t]),
                                           be.ptr(self.anc), be.ptr(self.status), be.ptr(self.ws), be.stream()),
                 "gmx_resample_rows_as")

    def enqueue(self):
        """every launch of the sweep on the current stream, per step: the site program over the R * n particles,
        gmx_resample_rows_pinned (nothing retained: gmx_resample_rows; ancestor_sampling=True and t < T - 1: gmx_rows_pin,
        the ancestor-logits program and gmx_resample_rows_as), gmx_history_record — in this order, so that the
        record holds the pins and the next step's gather extends every child of slot n - 1 from the retained state.  No
        syncs, no allocations, no host read of a device value."""
        be = _lib.get()
        N = self.R * self.n
        self.status.zero_()
        for t in range(self.T):
            _mh, prog, leaves, key, bufs = self._programs(t)
            bufs[prog.wo[1]] = self.lw.reshape(1, N)
            prog.comp.run(leaves, (N,), key, red_out=self.partials, out_buffers=bufs)
            self._resample(t)
            be.check(be.c.gmx_history_record(be.ptr(self.store.rows[t % 2]), self.D, be.ptr(self.lw), be.ptr(self.anc), N, 0,
                                             be.ptr(self.hist_xs[t]), be.ptr(self.hist_lws[t]), be.ptr(self.hist_ancs[t]),
                                             be.ptr(self.hist_status), be.stream()), "gmx_history_record")

    def rekey(self, keys: Key):
        """a new (R,) key batch: the proposal / resampling key tables — and the ancestor-draw table of
        ancestor_sampling=True — are rewritten IN PLACE (BootstrapBank.prepare's derivation), so a captured graph replays
        under the new keys"""
        if tuple(keys.shape) != (self.R,):
            raise ValueError(f"ConditionalBank.rekey: {self.R} chains need keys of shape {(self.R,)}, got {tuple(keys.shape)}")
        prop, res, last = self._key_tables(keys, third=True)
        self.keys_prop.copy_(torch.from_numpy(prop))
        self.keys_res.copy_(torch.from_numpy(res))
        if self.ancestor_sampling:
            self.keys_as.copy_(torch.from_numpy(last))
        self.keys = keys
        return self

    def draw(self, key: Key, backward=False):
        """One trajectory per chain from the last sweep (synchronises): k[r] = gmx_pick_rows of chain r's final log-weights
        under split(key, R)[r]; one gmx_lineage walk from the flat indices k + r * n through the recorded ancestors.
        Returns SweepHistory.trajectories()' layout — [R, T], [R, T, D] or a tuple of [R, T] — and keeps the trajectories
        and the recorded weights along them for retain().  backward=True: the same last state, then backward simulation
        over the recorded steps instead of the walk (the class docstring has the definition)."""
        if tuple(key.shape) != ():
            raise ValueError("ConditionalBank.draw takes ONE key")
        be = _lib.get()
        if self.ancestor_sampling and int(self.status[1].item()):
            raise FloatingPointError(f"ConditionalBank.draw: {int(self.status[1].item())} ancestor draw(s) of the last sweep "
                                     "found no particle with a positive transition density into the next retained state (a "
                                     "row of -inf logits): those steps kept the plain pin")
        if backward:
            return self._draw_backward(key)
        dev = self.hist_xs.device
        R, n, T, D = self.R, self.n, self.T, self.D
        k = torch.empty((R,), dtype=torch.int32, device=dev)
        status = torch.zeros((2,), dtype=torch.int64, device=dev)       # rows without mass; indices outside the history
        lw_last = self.hist_lws[T - 1]
        keys = split(key, R).data()                                      # (held until the call has returned)
        be.check(be.c.gmx_pick_rows(be.ptr(keys), be.ptr(lw_last), R, n, n, be.ptr(k), be.ptr(status[0:]),
                                    be.ptr(self.pick_ws), be.stream()), "gmx_pick_rows")
        start = (k + torch.arange(R, dtype=torch.int32, device=dev) * n).contiguous()
        paths = torch.empty((T, R), dtype=torch.int32, device=dev)
        traj = torch.empty((T, D, R), dtype=torch.float32, device=dev)
        be.check(be.c.gmx_lineage(be.ptr(self.hist_ancs), be.ptr(self.hist_xs), T, D, R * n, be.ptr(start), R, be.ptr(paths),
                                  be.ptr(traj), be.ptr(status[1:]), be.stream()), "gmx_lineage")
        lw_path = self.hist_lws.gather(1, paths.long())
        empty, bad = (int(v) for v in status.tolist())
        if empty:
            raise FloatingPointError(f"ConditionalBank.draw: the final weights of {empty} of the {R} chains carry no mass")
        if bad or int(self.hist_status.item()):
            raise IndexError(f"ConditionalBank.draw: {bad} index(es) outside [0, {R * n}) on the walk through the recorded "
                             "ancestors: they were clamped, nothing outside the history was read")
        self._last = (traj, lw_path, paths, k)
        return self._views._state_view(traj, 1)

    def _backward_buffers(self):
        """what the first backward draw allocates and every later one reuses: the state sites, the broadcast next state
        [D, R * n], the logits [R * n], the status words [T], the [T, R, 2] key table and gmx_pick_rows_take's workspace"""
        bw = getattr(self, "_bw", None)
        if bw is not None and bw["of"] is self.hist_xs:
            return bw
        be = _lib.get()
        dev = self.hist_xs.device
        R, n, T, D = self.R, self.n, self.T, self.D
        who = "ConditionalBank.draw(backward=True)"
        sites = self.state_sites
        if sites is None:
            if D > 1:
                raise NotImplementedError(f"{who}: a state of more than one component needs state_sites= (the address of "
                                          "each component, in order)")
            sites = (self.state_addr,)
        if len(sites) != D:
            raise ValueError(f"{who}: state_sites names {len(sites)} addresses for a state of {D} components")
        bw = dict(of=self.hist_xs, sites=sites,
                  next=torch.zeros((D, R * n), dtype=torch.float32, device=dev),
                  logits=torch.zeros((R * n,), dtype=torch.float32, device=dev),
                  status=torch.zeros((T,), dtype=torch.int64, device=dev),
                  keys=torch.zeros((T, R, 2), dtype=torch.int32, device=dev),
                  ws=torch.zeros(((int(be.c.gmx_pick_rows_take_workspace(R, n)) + 7) // 8,), dtype=torch.int64, device=dev))
        self._bw = bw
        return bw

    def _backward_keys(self, key: Key):
        """the row keys of a backward draw, on the host, int32 words [T, R, 2]: split(key, R) at t = T - 1 (draw()'s own),
        split(fold_in(key, t), R) below it"""
        from ..random import _derive_host
        R, T = self.R, self.T
        kh = np.asarray(key.host(), dtype=np.uint32).reshape(1, 2)
        children = np.arange(R, dtype=np.uint64)
        table = np.empty((T, R, 2), np.uint32)
        if T > 1:
            folds = _derive_host(kh, np.arange(T - 1, dtype=np.uint64)).reshape(T - 1, 1, 2)
            table[:T - 1] = _derive_host(folds, children).reshape(T - 1, R, 2)
        table[T - 1] = _derive_host(kh, children).reshape(R, 2)
        return table.view(np.int32)

    def _draw_backward(self, key: Key):
        """draw(key, backward=True): per step the logits program (t < T - 1) and gmx_pick_rows_take, which hands the chosen
        state to the next program — nothing passes through the host in between; one synchronisation at the end"""
        be = _lib.get()
        dev = self.hist_xs.device
        R, n, T, D = self.R, self.n, self.T, self.D
        N = R * n
        bw = self._backward_buffers()
        bw["keys"].copy_(torch.from_numpy(self._backward_keys(key)))           # (one upload)
        status = bw["status"]
        status.zero_()
        paths = torch.empty((T, R), dtype=torch.int32, device=dev)
        lw_path = torch.empty((T, R), dtype=torch.float32, device=dev)
        traj = torch.empty((T, D, R), dtype=torch.float32, device=dev)
        nxt, logits = bw["next"], bw["logits"]
        for t in range(T - 1, -1, -1):
            lw_t = self.hist_lws[t]
            if t < T - 1:
                x_t = self._views._state_view(self.hist_xs[t:t + 1], 0)
                x_t = type(x_t)(v[0] for v in x_t) if self.tuple_state is not None else x_t[0]
                _ancestor_logits(self.step, bw["sites"], self.obs_addr, x_t, tuple(self.step_extra(t + 1)) + self.tail,
                                 list(nxt), self.ys[t + 1], lw_t, logits.reshape(1, N), specialize=self.specialize,
                                 who="ConditionalBank.draw(backward=True)")
            be.check(be.c.gmx_pick_rows_take(be.ptr(bw["keys"][t]), be.ptr(lw_t if t == T - 1 else logits), R, n, n,
                                             be.ptr(lw_t), n, be.ptr(self.hist_xs[t]), D, N, n, n, be.ptr(paths[t]),
                                             be.ptr(lw_path[t]), be.ptr(traj[t]), be.ptr(nxt) if t > 0 else None, N,
                                             be.ptr(status[t:]), be.ptr(bw["ws"]), be.stream()), "gmx_pick_rows_take")
        counts = status.tolist()
        if counts[T - 1]:
            raise FloatingPointError(f"ConditionalBank.draw: the final weights of {counts[T - 1]} of the {R} chains carry no mass")
        bad = [t for t in range(T - 1) if counts[t]]
        if bad:
            raise FloatingPointError(f"ConditionalBank.draw(backward=True): step {bad[-1]}: {counts[bad[-1]]} of the {R} chains "
                                     "found no step-t particle with a positive transition density into their next state (a "
                                     "row of -inf logits)")
        k = paths[T - 1] - torch.arange(R, dtype=torch.int32, device=dev) * n
        self._last = (traj, lw_path, paths, k)
        return self._views._state_view(traj, 1)

    def retain(self):
        """the last draw() becomes the retained path: two device copies into ref_x / ref_lw, in place"""
        if self._last is None:
            raise RuntimeError("ConditionalBank.retain: nothing drawn yet (draw(key) after a launch())")
        self._set_conditional(True)
        self.ref_x.copy_(self._last[0])
        self.ref_lw.copy_(self._last[1])
        return self

    def _paths_to_rows(self, x_ref):
        """a path per chain in draw()'s layout -> [T, D, R]"""
        R, T, D = self.R, self.T, self.D
        dev = self.ref_x.device
        if self.tuple_state is not None:
            ok = isinstance(x_ref, (tuple, list)) and len(x_ref) == D and all(tuple(torch.as_tensor(v).shape) == (R, T) for v in x_ref)
            want = f"a {self.tuple_state.__name__} of {D} arrays of shape {(R, T)}"
            rows = (lambda: torch.stack([torch.as_tensor(v).to(dev).float().t() for v in x_ref], dim=1))
        elif not self.event:
            ok = not isinstance(x_ref, (tuple, list)) and tuple(torch.as_tensor(x_ref).shape) == (R, T)
            want = f"an array of shape {(R, T)}"
            rows = (lambda: torch.as_tensor(x_ref).to(dev).float().t().reshape(T, 1, R))
        else:
            ok = not isinstance(x_ref, (tuple, list)) and tuple(torch.as_tensor(x_ref).shape) == (R, T, D)
            want = f"an array of shape {(R, T, D)}"
            rows = (lambda: torch.as_tensor(x_ref).to(dev).float().permute(1, 2, 0))
        if not ok:
            got = [tuple(torch.as_tensor(v).shape) for v in x_ref] if isinstance(x_ref, (tuple, list)) else \
                tuple(torch.as_tensor(x_ref).shape)
            raise ValueError(f"ConditionalBank.set_retained: the retained paths are {want} (R chains, T steps: draw()'s "
                             f"layout); got {got}")
        return rows().contiguous()

    def set_retained(self, x_ref):
        """A caller's own retained path per chain, in draw()'s layout.  Its weights come from the model, at set-up time (one
        launch of R particles per step, none of it in the sweep): ref_lw[t] is the OBSERVATION site's score of step t's
        model — init for t = 0, else step called with (x_ref[t-1], *step_extra(t), *params) — constrained on the state
        sites and the observation (importance, then project on obs_addr; not the importance weight, which also holds the
        transition density).  state_sites (the constructor's): the address of each state component, in order; default
        (state_addr,), required for D > 1.  The model may have no latent site besides them and the observation."""
        from ..core.choice_map import Selection
        from ..random import key as _key
        if not hasattr(self, "ref_x"):
            raise RuntimeError("ConditionalBank.set_retained: prepare(keys, ys) first")
        R, T, D = self.R, self.T, self.D
        sites = self.state_sites
        if sites is None:
            if D > 1:
                raise NotImplementedError("ConditionalBank.set_retained: a state of more than one component needs "
                                          "state_sites= (the address of each component, in order)")
            sites = (self.state_addr,)
        if len(sites) != D:
            raise ValueError(f"ConditionalBank.set_retained: state_sites names {len(sites)} addresses for a state of {D} "
                             "components")
        rows = self._paths_to_rows(x_ref)
        dev = rows.device
        params = tuple(torch.as_tensor(p).to(dev).float() for p in self.params)
        keys = split(_key(0), R)                   # (nothing is left to draw)
        sel = Selection.at[self.obs_addr]
        ref_lw = torch.empty((T, R), dtype=torch.float32, device=dev)
        for t in range(T):
            con = self._obs(t)
            for d, a in enumerate(sites):
                con = con.set(a, rows[t, d])
            if t == 0:
                model, args = self.init, params
            else:
                prev = self._views._state_view(rows[t - 1:t], 0)
                prev = type(prev)(v[0] for v in prev) if self.tuple_state is not None else prev[0]
                model, args = self.step, (prev,) + tuple(self.step_extra(t)) + params
            tr, _w = model.importance(keys, con, args)
            extra = [a for a in tr.subtraces if a not in sites and a != self.obs_addr]
            if extra:
                raise NotImplementedError(
                    f"ConditionalBank.set_retained: the {'init' if t == 0 else 'step'} model samples {extra[0]!r}, which is "
                    f"neither one of the state's sites {tuple(sites)!r} nor the observation {self.obs_addr!r}: the retained "
                    "path does not say what it was")
            ref_lw[t] = engine.materialize(model.project(keys, tr, sel)).reshape(R)
        self._set_conditional(True)
        self.ref_x.copy_(rows)
        self.ref_lw.copy_(ref_lw)
        return self

    def run(self, key: Key, ys=None, iters: int = 1, retained=None, backward=False):
        """The particle-Gibbs driver: `iters` conditional sweeps, each followed by a draw that becomes the next sweep's
        retained path.  Schedule (build-defined, as the sweeps' key schedules are): for k = 0 .. iters - 1

            (k_sweep, k_draw) = split(fold_in(key, k), 2)
            rekey(split(k_sweep, R)); launch(); draw(k_draw, backward); retain()

        With nothing retained (no `retained`, no earlier retain() / set_retained()) iteration 0 is an unconditional sweep.
        ys given: the bank is prepared for it first (prepare(split(key, R), ys, retained)); ys = None keeps a prepared bank
        — its observations, its retained path and its captured graph.  Returns the stacked draws: [iters, R, T],
        [iters, R, T, D] or a tuple of [iters, R, T]."""
        if tuple(key.shape) != ():
            raise ValueError("ConditionalBank.run takes ONE key")
        if ys is not None:
            self.prepare(split(key, self.R), ys, retained)
        elif retained is not None:
            self.set_retained(retained)
        out = []
        for k in range(int(iters)):
            ks = split(fold_in(key, k), 2)
            self.rekey(split(ks[0], self.R))
            self.launch()
            x = self.draw(ks[1], backward=backward)
            self.retain()
            out.append(x)                  # (views of this draw's own buffer)
        if self.tuple_state is not None:
            return self.tuple_state(torch.stack([o[d] for o in out]) for d in range(self.D))
        return torch.stack(out)


# ---------------------------------------------------------------------------
# particle marginal Metropolis-Hastings over a bank of filters
# ---------------------------------------------------------------------------
PMMH_MAX_PARAMS = 8                     # GMX_PMMH_MAX_P (csrc/gmx_sizes.h): the proposal kernel's LDS layout
ParticleMHResult = namedtuple("ParticleMHResult", ["theta", "log_ml", "accepted"])


def _prior_logpdf(prior, addrs, values, out, specialize=False, launch=True, who="ParticleMH"):
    """out[0, r] = prior.assess({addrs[p]: values[p][r]}, ())[0] in float32 over the R = out.shape[1] chains in ONE launch:
    the prior's `assess` traced once over a batch of R, every site constrained to a per-chain leaf values[p] ([R] each).
    Built as _ancestor_logits builds the per-particle program: cached on the model, the leaves' kinds and `specialize`
    (specialised once, when built); launch=False builds it only.  A prior whose sites are not exactly `addrs` is refused
    by name."""
    def refuse(sites):
        extra = [a for a in sites if a not in addrs]
        unused = [a for a in addrs if a not in sites]
        raise ValueError(f"{who}: the prior's sites are not exactly param_addrs = {tuple(addrs)!r}"
                         + (f"; it samples {extra!r}, which is not a parameter" if extra else "")
                         + (f"; it has no site {unused!r}" if unused else "")) from None

    def emit(assess, syms, tr):            # syms: the P per-chain parameter leaves
        con = ChoiceMap.empty()
        for a, v in zip(addrs, syms):
            con = con.set(a, v)
        rec, score = assess(con)
        if set(rec.sites) != set(addrs) or len(rec.sites) != len(addrs):
            refuse(list(rec.sites))
        return score
    return _assess_program(prior, (), list(values), (tuple(addrs), "prior"), emit, refuse, out, specialize, launch)


class ParticleMH(_Sweep):
    """Particle marginal Metropolis-Hastings (PMMH: Andrieu, Doucet & Holenstein 2010, section 2.4.2) over the P
    parameters of a state-space model: R independent random-walk chains, chain r driving filter r of a
    BootstrapBank(init, step, n, R, T, params=theta0, ...) it owns — the bank's programs, stores and launches untouched.
    The models are called as the bank calls them: init(*params_r), step(x_prev, *step_extra(t), *params_r).  `prior`: a
    `@gen` function of no arguments with one scalar site per entry of `param_addrs` (parameter p is the site
    param_addrs[p] and the p-th entry of `params_r`); `step_size`: P positive floats, the standard deviations of the
    random-walk proposal (no transforms, no adaptation).

    One iteration, enqueue(), is a fixed chain of launches with no sync, no allocation and no host read of a device value —
    so capture() makes it one graph replay:
      1. gmx_pmmh_propose   the proposals theta' (iteration 0: theta' = theta, the start is evaluated), broadcast over the
                            bank's per-particle parameter leaves, and the bank's T x R key tables;
      2. the prior program  log prior(theta'_r) for every chain, one `assess` program over a batch of R;
      3. bank.enqueue()     the sweep: per step one site program over the R * n particles and one row resampling;
      4. gmx_pmmh_accept    the evidence of every chain's sweep from the exact-integer (maxs, totals) in float64 on the
                            device, the decision log u < (float32)((ll' - ll) + (lp' - lp)), the chains' state, the record.
    The iteration count lives in two device words.  A chain starts at ll = -inf, lp = 0: iteration 0 accepts any start
    whose sweep carries mass.  A proposal outside the prior's support (lp' = -inf), or one whose sweep lost all mass
    against a finite current state, is never accepted (NaN rejects).

    Key schedule, under the ONE key of prepare(): k_it = fold_in(key, j) for iteration j (counted from prepare());
    (k_bank, k_prop, k_acc) = split(k_it, 3); chain r's sweep runs under split(k_bank, R)[r], its proposal for parameter p
    is the normal draw under split(split(k_prop, R)[r], P)[p], its uniform under split(k_acc, R)[r].

    Contract: under the keys split(k_bank_j, R) and the parameters theta'_j, the sweep of iteration j is, row for row and
    bit for bit, what BootstrapBank(..., params=theta'_j).prepare(those keys, ys) gives launched on its own; every
    decision is gmx_mh_accept's on the float32 log_alpha.

    Limits: 1 <= P <= 8 (the proposal kernel holds P draws per chain of a workgroup in LDS); whatever BootstrapBank
    refuses (rejuvenate=, history=, comm=, ...) is refused by it, by name."""

    def __init__(self, init, step, prior, n_particles: int, n_chains: int, T: int, param_addrs, step_size, obs_addr="y",
                 state_addr="x", resample="systematic", step_extra=None, ess_threshold=None, specialize=True, **bank_kw):
        self.param_addrs = tuple(param_addrs)
        self.P = len(self.param_addrs)
        if self.P < 1 or self.P > PMMH_MAX_PARAMS:
            raise NotImplementedError(f"ParticleMH: {self.P} parameters; param_addrs names between 1 and {PMMH_MAX_PARAMS} "
                                      "(gmx_pmmh_propose holds the draws of a workgroup's chains in LDS)")
        if len(set(self.param_addrs)) != self.P:
            raise ValueError(f"ParticleMH: param_addrs = {self.param_addrs!r} names a site twice")
        try:
            sizes = [float(s) for s in step_size]
        except TypeError:
            sizes = None
        if sizes is None or len(sizes) != self.P or not all(math.isfinite(s) and s > 0.0 for s in sizes):
            raise ValueError(f"ParticleMH: step_size is {self.P} positive floats, one per entry of param_addrs; got {step_size!r}")
        self.step_size = tuple(sizes)
        self.prior = prior
        self.specialize = specialize
        self.bank = BootstrapBank(init, step, n_particles, n_chains, T, obs_addr=obs_addr, resample=resample,
                                  step_extra=step_extra, specialize=specialize, state_addr=state_addr,
                                  ess_threshold=ess_threshold, **bank_kw)
        self.n, self.R, self.T = self.bank.n, self.bank.R, self.bank.T
        self.done = self.max_iters = 0

    def prepare(self, key: Key, ys: torch.Tensor, theta0, max_iters: int):
        """ONE key; theta0: P float32 [R] tensors, the chains' starts; max_iters: how many iterations run() may be asked
        for in all (the record slabs hold that many rows).  Every buffer is allocated here."""
        be = _lib.get()
        self._drop_graph()
        P, R, n, T = self.P, self.R, self.n, self.T
        dev = be.device
        if tuple(key.shape) != ():
            raise ValueError(f"ParticleMH.prepare takes ONE key (the chains' keys are split from it); got a batch of shape "
                             f"{tuple(key.shape)}")
        theta0 = tuple(theta0) if isinstance(theta0, (tuple, list)) else (theta0,)
        theta0 = tuple(torch.as_tensor(v) for v in theta0)
        if len(theta0) != P or any(tuple(v.shape) != (R,) for v in theta0):
            raise ValueError(f"ParticleMH.prepare: theta0 is {P} tensors of shape {(R,)}, one per entry of param_addrs; got "
                             f"{[tuple(v.shape) for v in theta0]}")
        max_iters = int(max_iters)
        if max_iters < 1 or max_iters >= 2 ** 32:
            raise ValueError(f"ParticleMH.prepare: max_iters = {max_iters} is outside [1, 2^32) (an iteration is fold_in's "
                             "32-bit word)")
        self.key, self._key_c = key, _key_words(key)
        self.bank.params = tuple(v.to(dev).float() for v in theta0)
        self.bank.prepare(split(split(fold_in(key, 0), 3)[0], R), ys)
        self.theta = torch.stack(self.bank.params).contiguous()                      # [P, R]
        self.theta_prop = self.theta.clone()
        self.scale = torch.tensor(self.step_size, dtype=torch.float32, device=dev)
        self.lp_prop = torch.zeros((1, R), dtype=torch.float32, device=dev)
        self.ll = torch.full((R,), -math.inf, dtype=torch.float64, device=dev)
        self.lp = torch.zeros((R,), dtype=torch.float32, device=dev)
        self.it = torch.zeros((2,), dtype=torch.int32, device=dev)                   # the iteration words (uint32)
        self.rec_theta = torch.zeros((max_iters, P, R), dtype=torch.float32, device=dev)
        self.rec_ll = torch.zeros((max_iters, R), dtype=torch.float64, device=dev)
        self.rec_acc = torch.zeros((max_iters, R), dtype=torch.uint8, device=dev)
        self.rec_base = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.status = torch.zeros((1,), dtype=torch.int64, device=dev)               # iterations outside the record
        self.leaves = torch.tensor([v.data_ptr() for v in self.bank.params_full], dtype=torch.int64, device=dev)
        self.shift_ln2, self.log_n = self.bank.shift * math.log(2.0), math.log(n)    # as evidence_terms computes them
        self.max_iters, self.done = max_iters, 0
        self._prior(launch=False)
        return self

    def _prior(self, launch=True):
        _prior_logpdf(self.prior, self.param_addrs, [self.theta_prop[p] for p in range(self.P)], self.lp_prop,
                      specialize=self.specialize, launch=launch)

    def enqueue(self):
        """one iteration on the current stream: gmx_pmmh_propose, the prior program, the bank's sweep, gmx_pmmh_accept —
        no syncs, no allocations, no host read of a device value"""
        be = _lib.get()
        b = self.bank
        be.check(be.c.gmx_pmmh_propose(self._key_c, be.ptr(self.it), be.ptr(self.theta), be.ptr(self.scale), self.P, self.R,
                                       self.n, self.T, be.ptr(b.keys_prop), be.ptr(b.keys_res), be.ptr(self.leaves),
                                       be.ptr(self.theta_prop), be.stream()), "gmx_pmmh_propose")
        self._prior()
        b.enqueue()
        be.check(be.c.gmx_pmmh_accept(self._key_c, be.ptr(self.it), be.ptr(b.maxs), be.ptr(b.totals),
                                      be.ptr(b.flags) if b.ess_q8 is not None else None, self.T, self.R, self.P, b.shift,
                                      self.shift_ln2, self.log_n, be.ptr(self.lp_prop), be.ptr(self.theta), be.ptr(self.ll),
                                      be.ptr(self.lp), be.ptr(self.theta_prop), be.ptr(self.rec_theta), be.ptr(self.rec_ll),
                                      be.ptr(self.rec_acc), be.ptr(self.rec_base), self.max_iters, be.ptr(self.status),
                                      be.stream()), "gmx_pmmh_accept")

    def capture(self):
        """Capture one iteration into a hipGraph (_Sweep.capture).  Its warm-up enqueue() runs outside the capture and
        ADVANCES the chains by one iteration, so the iteration words, the chains' state (theta, log_ml, log_prior), the
        record base and the status word are saved before and restored afterwards: capture() leaves the chains where
        they were (the record row the warm-up wrote is written again by the iteration it belongs to)."""
        saved = [(t, t.clone()) for t in (self.it, self.theta, self.ll, self.lp, self.rec_base, self.status)]
        super().capture()
        for t, was in saved:
            t.copy_(was)
        return self

    def run(self, iters: int) -> ParticleMHResult:
        """`iters` more iterations of every chain (the chains continue from where the last run() left them); one sync,
        at the end.  Returns theta [iters, P, R] float32, log_ml [iters, R] float64 (the evidence estimate the chain
        holds after each iteration) and accepted [iters, R] bool."""
        iters = int(iters)
        if iters < 0 or self.done + iters > self.max_iters:
            raise ValueError(f"ParticleMH.run: {self.done} iterations done and {iters} asked for, past max_iters = "
                             f"{self.max_iters} (prepare(..., max_iters=) sizes the record)")
        self.rec_base.fill_(self.done)                 # a device write: this run's iterations land in rows 0 .. iters - 1
        for _ in range(iters):
            self.launch()
        self.done += iters
        out = ParticleMHResult(self.rec_theta[:iters].clone(), self.rec_ll[:iters].clone(), self.rec_acc[:iters] != 0)
        missed = int(self.status.item())               # (synchronises)
        if missed:
            raise _lib.GenmiError(f"ParticleMH.run: {missed} iterations fell outside the record")
        return out

    def state(self):
        """(theta [P, R] float32, log_ml [R] float64, log_prior [R] float32) of the chains now"""
        return self.theta.clone(), self.ll.clone(), self.lp.clone()


# ---------------------------------------------------------------------------
# particle Gibbs over a bank of conditional filters
# ---------------------------------------------------------------------------
ParticleGibbsResult = namedtuple("ParticleGibbsResult", ["theta", "log_joint", "accepted", "paths"])


def _trajectory_scores(model, sites, obs_addr, args, x, y, out, specialize=False, launch=True, who="ParticleGibbs"):
    """out = (joint, obs), each [1, B]:  joint[0, c] = model.assess({sites[d]: x[d][c], obs_addr: y}, args_c)[0] and
    obs[0, c] = the observation site's score inside that call, in float32, over the B columns in ONE launch — one step of
    a trajectory scored under per-column arguments (ParticleGibbs: the drawn path on both halves of B = 2R, theta on one
    and theta' on the other).  x: the D per-column state leaves; `args` may hold per-column leaves.  Built on
    _assess_program with two outputs: cached on the model, the leaves' kinds and `specialize` (specialised once, when
    built); launch=False builds it only.  A model that samples anything besides `sites` and the observation is refused."""
    from .. import tracer as Tr
    D = len(x)

    def emit(assess, syms, tr):            # syms: y, the D per-column states
        rec, score = assess(_transition_choices(sites, obs_addr, syms[0], syms[1:1 + D]))
        site = rec.sites.get(obs_addr)
        if site is None or getattr(site, "score", None) is None:
            raise NotImplementedError(f"{who}: the model has no site {obs_addr!r} of its own to score the observation at")
        return score, Tr.as_float(site.score)
    return _assess_program(model, tuple(args), [y] + list(x), (tuple(sites), obs_addr, "trajectory"), emit,
                           _transition_refusal(who, sites, obs_addr), out, specialize, launch)


class ParticleGibbs:
    """Particle Gibbs (Andrieu, Doucet & Holenstein 2010, section 2.4.3) over the P parameters of a state-space model: R
    independent chains, the state of chain r being (theta[:, r], x_ref[:, :, r]) — its parameters and the retained path of
    chain r of a ConditionalBank(init, step, n, R, T, params=theta0, state_sites=, ancestor_sampling=) it owns, the bank's
    programs, stores and launches untouched.  An iteration alternates x | theta, y by conditional SMC with a random-walk
    Metropolis-Hastings move of theta | x, y.  The models are called as the bank calls them: init(*params_r),
    step(x_prev, *step_extra(t), *params_r).  `prior`, `param_addrs` and `step_size` are ParticleMH's: a `@gen` function of
    no arguments with one scalar site per entry of `param_addrs`, and P positive standard deviations (no transforms, no
    adaptation).  ancestor_sampling=True is PGAS, backward=True draws every new path by backward simulation (PGBS).

    Iteration j, counted from prepare(), is host-driven (the draw synchronises); j is an argument of the entry points:
      1. gmx_pg_open        the bank's key tables (keys_prop, keys_res, and keys_as with ancestor sampling) for the chain
                            keys split(k_sweep, R) — BootstrapBank._key_tables(keys, third=True), on the device — and
                            theta[p, r] broadcast over the bank's P per-particle parameter leaves: ONE launch;
      2. bank.launch(); x = bank.draw(k_draw, backward); bank.retain() — unchanged; with nothing retained, iteration 0 is
                            the unconditional sweep, as in ConditionalBank.run;
      3. gmx_pg_propose     theta_pair[p] = [theta[p] | theta'[p]], theta' a random-walk step at EVERY j: ONE launch;
      4. the prior program  lp[0:R] under theta, lp[R:2R] under theta': one `assess` program over a batch of 2R;
      5. the scores         for t = 0 .. T - 1 one program over a batch of 2R, the drawn path on both halves:
                              joint[t, c] = model_t.assess({state_sites[d]: x[t][d], obs_addr: y_t}, args_t(c))[0]   (float32)
                              obs[t, c]   = the observation site's score inside that call                             (float32)
                            model_0 = init, args_0 = theta_c; t >= 1: model_t = step, args_t = (x[t-1], *step_extra(t), *theta_c);
      6. gmx_pg_accept      per chain S = sum_t (double)joint[t, r] and S' = sum_t (double)joint[t, R + r], ascending t, in
                            float64; log_alpha = (float)((S' - S) + ((double)lp[R + r] - (double)lp[r])); taken iff
                            log u < log_alpha (gmx_mh_accept's rule; NaN rejects); then theta[:, r], log_joint[r] =
                            (taken ? S' + lp' : S + lp), the record row — and ref_lw[t, r] = obs[t, taken ? R + r : r] for
                            every t: the pinned weights are those of the parameters the next sweep runs under, whatever
                            the decision.  ONE launch.

    Key schedule, under the ONE key of prepare(): k_it = fold_in(key, j); (k_sweep, k_draw, k_prop, k_acc) =
    split(k_it, 4); chain r's sweep runs under split(k_sweep, R)[r], the draw under k_draw, the proposal for parameter p
    under split(split(k_prop, R)[r], P)[p], the uniform under split(k_acc, R)[r].

    Contract: run() is, bit for bit, the Python loop over public parts — per iteration a fresh ConditionalBank(...,
    params=theta_j).prepare(split(k_sweep, R), ys, retained=x_{j-1}), launch(), draw(k_draw, backward); the public
    init.assess / step.assess / prior.assess over a batch of R under theta_j and theta'_j, summed sequentially in float64;
    gmx_mh_accept's decision.  In particular ref_lw after the move equals what ConditionalBank.set_retained(x) computes
    under params = the accepted theta.

    capture() captures the bank's sweep (ConditionalBank.capture) in its current form: after iteration 0 (or with
    `retained=`) that is the conditional sweep every later iteration replays; the rest of an iteration is not capturable.

    Limits: 1 <= P <= 8 (gmx_pg_open holds the values of a workgroup's chains in LDS); a model that samples anything besides
    the state sites and the observation is refused; a state of more than one component needs state_sites=; whatever
    ConditionalBank refuses (resample=, ess_threshold=, n > 1024 once a path is retained, ...) is refused by it, by name.
    Not here: adaptive or correlated proposals, transforms, conjugate updates, several moves per sweep, per-chain
    observations, sharding."""

    def __init__(self, init, step, prior, n_particles: int, n_chains: int, T: int, param_addrs, step_size, obs_addr="y",
                 state_addr="x", state_sites=None, step_extra=None, ancestor_sampling=False, backward=False, specialize=True,
                 **bank_kw):
        self.param_addrs = tuple(param_addrs)
        self.P = len(self.param_addrs)
        if self.P < 1 or self.P > PMMH_MAX_PARAMS:
            raise NotImplementedError(f"ParticleGibbs: {self.P} parameters; param_addrs names between 1 and {PMMH_MAX_PARAMS} "
                                      "(gmx_pg_open holds the values of a workgroup's chains in LDS)")
        if len(set(self.param_addrs)) != self.P:
            raise ValueError(f"ParticleGibbs: param_addrs = {self.param_addrs!r} names a site twice")
        try:
            sizes = [float(s) for s in step_size]
        except TypeError:
            sizes = None
        if sizes is None or len(sizes) != self.P or not all(math.isfinite(s) and s > 0.0 for s in sizes):
            raise ValueError(f"ParticleGibbs: step_size is {self.P} positive floats, one per entry of param_addrs; got {step_size!r}")
        self.step_size = tuple(sizes)
        self.init, self.step, self.prior = init, step, prior
        self.specialize, self.backward = specialize, bool(backward)
        self.bank = ConditionalBank(init, step, n_particles, n_chains, T, obs_addr=obs_addr, step_extra=step_extra,
                                    specialize=specialize, state_addr=state_addr, state_sites=state_sites,
                                    ancestor_sampling=ancestor_sampling, **bank_kw)
        self.n, self.R, self.T = self.bank.n, self.bank.R, self.bank.T
        self.done = self.max_iters = 0

    def prepare(self, key: Key, ys: torch.Tensor, theta0, max_iters: int, retained=None):
        """ONE key; theta0: P float32 [R] tensors, the chains' starts; max_iters: how many iterations run() may be asked
        for in all (the record slabs hold that many rows); retained: a path per chain in draw()'s layout
        (ConditionalBank.set_retained under theta0), or None: iteration 0 sweeps unconditionally.  Every buffer is
        allocated here."""
        be = _lib.get()
        P, R, T = self.P, self.R, self.T
        dev = be.device
        b = self.bank
        if tuple(key.shape) != ():
            raise ValueError(f"ParticleGibbs.prepare takes ONE key (the chains' keys are split from it); got a batch of shape "
                             f"{tuple(key.shape)}")
        theta0 = tuple(theta0) if isinstance(theta0, (tuple, list)) else (theta0,)
        theta0 = tuple(torch.as_tensor(v) for v in theta0)
        if len(theta0) != P or any(tuple(v.shape) != (R,) for v in theta0):
            raise ValueError(f"ParticleGibbs.prepare: theta0 is {P} tensors of shape {(R,)}, one per entry of param_addrs; got "
                             f"{[tuple(v.shape) for v in theta0]}")
        max_iters = int(max_iters)
        if max_iters < 1 or max_iters >= 2 ** 32:
            raise ValueError(f"ParticleGibbs.prepare: max_iters = {max_iters} is outside [1, 2^32) (an iteration is fold_in's "
                             "32-bit word)")
        self.key, self._key_c = key, _key_words(key)
        self.theta = torch.stack([v.to(dev).float() for v in theta0]).contiguous()   # [P, R]
        b.params = tuple(self.theta[p] for p in range(P))                            # (views: the bank sees the chains' theta)
        b.prepare(split(split(fold_in(key, 0), 4)[0], R), ys, retained)
        D = b.D
        sites = b.state_sites
        if sites is None:
            if D > 1:
                raise NotImplementedError("ParticleGibbs: a state of more than one component needs state_sites= (the address "
                                          "of each component, in order)")
            sites = (b.state_addr,)
        if len(sites) != D:
            raise ValueError(f"ParticleGibbs: state_sites names {len(sites)} addresses for a state of {D} components")
        self._sites = tuple(sites)
        self.theta_pair = torch.zeros((P, 2 * R), dtype=torch.float32, device=dev)
        self.scale = torch.tensor(self.step_size, dtype=torch.float32, device=dev)
        self.lp = torch.zeros((1, 2 * R), dtype=torch.float32, device=dev)
        self.joint = torch.zeros((T, 2 * R), dtype=torch.float32, device=dev)
        self.obs = torch.zeros((T, 2 * R), dtype=torch.float32, device=dev)
        self.x_pair = torch.zeros((T, D, 2 * R), dtype=torch.float32, device=dev)    # the drawn path on both halves
        self.log_joint = torch.full((R,), -math.inf, dtype=torch.float64, device=dev)
        self.rec_theta = torch.zeros((max_iters, P, R), dtype=torch.float32, device=dev)
        self.rec_lj = torch.zeros((max_iters, R), dtype=torch.float64, device=dev)
        self.rec_acc = torch.zeros((max_iters, R), dtype=torch.uint8, device=dev)
        self.leaves = torch.tensor([v.data_ptr() for v in b.params_full], dtype=torch.int64, device=dev)
        self.max_iters, self.done = max_iters, 0
        self._launchers = [self._prior()] + self._scores()
        return self

    def _prior(self):
        """the launcher of lp: the prior's program over the batch of 2R, built here"""
        return _prior_logpdf(self.prior, self.param_addrs, [self.theta_pair[p] for p in range(self.P)], self.lp,
                             specialize=self.specialize, launch=False, who="ParticleGibbs")

    def _scores(self):
        """the launchers of joint[t], obs[t] for every step: T launches over the batch of 2R (two programs, init's and
        step's, built here; every leaf and output is a persistent buffer, so each launcher keeps ONE binding)"""
        b = self.bank
        theta_c = tuple(self.theta_pair[p] for p in range(self.P))
        out = []
        for t in range(self.T):
            if t == 0:
                model, args = self.init, theta_c
            else:
                prev = b._views._state_view(self.x_pair[t - 1:t], 0)
                prev = type(prev)(v[0] for v in prev) if b.tuple_state is not None else prev[0]
                model, args = self.step, (prev,) + tuple(b.step_extra(t)) + theta_c
            out.append(_trajectory_scores(model, self._sites, b.obs_addr, args, list(self.x_pair[t]), b.ys[t],
                                          (self.joint[t:t + 1], self.obs[t:t + 1]), specialize=self.specialize, launch=False))
        return out

    def _iterate(self, j):
        """iteration j: the class docstring's six steps; returns the draw"""
        be = _lib.get()
        b = self.bank
        P, R, T = self.P, self.R, self.T
        be.check(be.c.gmx_pg_open(self._key_c, j, be.ptr(self.theta), P, R, self.n, T, be.ptr(b.keys_prop), be.ptr(b.keys_res),
                                  be.ptr(b.keys_as) if b.ancestor_sampling else None, be.ptr(self.leaves), be.stream()),
                 "gmx_pg_open")
        b.launch()
        x = b.draw(split(fold_in(self.key, j), 4)[1], backward=self.backward)
        b.retain()
        traj = b._last[0]
        self.x_pair[:, :, :R].copy_(traj)
        self.x_pair[:, :, R:].copy_(traj)
        be.check(be.c.gmx_pg_propose(self._key_c, j, be.ptr(self.theta), be.ptr(self.scale), P, R, be.ptr(self.theta_pair),
                                     be.stream()), "gmx_pg_propose")
        for launch in self._launchers:
            launch()
        be.check(be.c.gmx_pg_accept(self._key_c, j, be.ptr(self.joint), be.ptr(self.obs), be.ptr(self.lp), be.ptr(self.theta_pair),
                                    T, R, P, be.ptr(self.theta), be.ptr(self.log_joint), be.ptr(b.ref_lw), be.ptr(self.rec_theta),
                                    be.ptr(self.rec_lj), be.ptr(self.rec_acc), j, self.max_iters, be.stream()), "gmx_pg_accept")
        return x

    def capture(self):
        """capture the bank's sweep in its current form (ConditionalBank.capture); the chains stay where they are"""
        self.bank.capture()
        return self

    def run(self, iters: int, paths=False) -> ParticleGibbsResult:
        """`iters` more iterations of every chain (the chains continue from where the last run() left them).  Returns
        theta [iters, P, R] float32, log_joint [iters, R] float64 (log p(theta, x, y) of the state each iteration ends
        in), accepted [iters, R] bool, and with paths=True the stacked draws as ConditionalBank.run returns them
        ([iters, R, T], [iters, R, T, D] or a tuple of [iters, R, T]), else None."""
        iters = int(iters)
        if not self.max_iters:
            raise RuntimeError("ParticleGibbs.run: prepare(key, ys, theta0, max_iters) first")
        if iters < 0 or self.done + iters > self.max_iters:
            raise ValueError(f"ParticleGibbs.run: {self.done} iterations done and {iters} asked for, past max_iters = "
                             f"{self.max_iters} (prepare(..., max_iters=) sizes the record)")
        b = self.bank
        first, out = self.done, []
        for _ in range(iters):
            x = self._iterate(self.done)
            self.done += 1
            if paths:
                out.append(x)
        stacked = None
        if paths and out:
            stacked = b.tuple_state(torch.stack([o[d] for o in out]) for d in range(b.D)) if b.tuple_state is not None \
                else torch.stack(out)
        rows = slice(first, first + iters)
        return ParticleGibbsResult(self.rec_theta[rows].clone(), self.rec_lj[rows].clone(), self.rec_acc[rows] != 0, stacked)

    def state(self):
        """(theta [P, R] float32, log_joint [R] float64, the retained paths in draw()'s layout) of the chains now"""
        b = self.bank
        x = b._views._state_view(b.ref_x.clone(), 1)
        return self.theta.clone(), self.log_joint.clone(), x
