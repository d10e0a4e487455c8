"""Shared drivers of tests/test_pmmh_cpu.py (the C-ABI's CPU mirror) and tests/test_pmmh_gpu.py (the HIP library):
gmx_pmmh_propose and gmx_pmmh_accept against their definitions in numpy (random._derive_host for the keys, the existing
gmx_random_bits / gmx_std_normal_from_bits / gmx_mh_accept entry points for the draws, float32 / float64 numpy for the
rest), gmx_log64 against numpy's log, smc.ParticleMH against the same chain composed in a Python loop from public parts,
the device against the mirror, the API's refusals, and the law: the chains' mean against the exact posterior."""
from __future__ import annotations

import ctypes
import functools
import math
import types

import numpy as np
import torch

from tests import history_checks as H

POISON = np.float32(-12345.5)
ITERS = 6
SEED = 20102                            # the run key of every chain case; no reference decision is a near-tie (asserted)
NEAR_TIE = 1e-5
# (R, n, T, P, ess_threshold): rows and tables that fill no vector; R * n no multiple of 4 or 256; R beyond one workgroup
# in both kernels; one parameter; the adaptive bank's flags (both outcomes must occur: asserted)
CASES = {"tiny": (5, 8, 3, 2, None), "edges": (3, 100, 4, 2, None), "wide": (300, 4, 2, 2, None), "one": (5, 8, 3, 1, None),
         "ess": (6, 16, 5, 2, 0.5)}
STEP_SIZE = (0.05, 0.1)
PRIOR = ((0.5, 0.99), (0.2, 1.0))       # uniform priors on the transition coefficient and on the process-noise scale


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _words(key_words):
    return (ctypes.c_uint32 * 2)(int(key_words[0]), int(key_words[1]))


# --- the key schedule and the draws, from existing pieces -------------------------------------------------------------------
def iter_keys(key_words, j):
    """(k_bank, k_prop, k_acc) of iteration j: split(fold_in(key, j), 3)"""
    from genjax_amd.random import _derive_host
    k_it = _derive_host(np.asarray(key_words, np.uint32).reshape(2), np.uint64(j))
    ks = _derive_host(k_it[None, :], np.arange(3, dtype=np.uint64))
    return ks[0], ks[1], ks[2]


def split_host(k, m):
    from genjax_amd.random import _derive_host
    return _derive_host(np.asarray(k, np.uint32).reshape(1, 2), np.arange(m, dtype=np.uint64)).reshape(m, 2)


def bits_of(be, keys):
    """counter 0's 32 bits under each key: gmx_random_bits"""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    k_d = torch.from_numpy(_i32(keys)).to(be.device)
    out = torch.zeros((keys.shape[0],), dtype=torch.int32, device=be.device)
    be.check(be.c.gmx_random_bits(be.ptr(k_d), keys.shape[0], 1, be.ptr(out), be.stream()), "gmx_random_bits")
    return out.cpu().numpy().view(np.uint32)


def std_normal_of(be, bits):
    b_d = torch.from_numpy(_i32(bits)).to(be.device)
    out = torch.zeros((bits.size,), dtype=torch.float32, device=be.device)
    be.check(be.c.gmx_std_normal_from_bits(be.ptr(b_d), bits.size, be.ptr(out), be.stream()), "gmx_std_normal_from_bits")
    return out.cpu().numpy()


def mh_accept_of(be, keys, log_alpha):
    k_d = torch.from_numpy(_i32(keys).reshape(-1, 2)).to(be.device)
    la = torch.from_numpy(np.ascontiguousarray(log_alpha, dtype=np.float32)).to(be.device)
    acc = torch.full((la.numel(),), 7, dtype=torch.uint8, device=be.device)
    be.check(be.c.gmx_mh_accept(be.ptr(k_d), be.ptr(la), la.numel(), be.ptr(acc), be.stream()), "gmx_mh_accept")
    return acc.cpu().numpy()


def unit_of(bits):
    """jax.random.uniform's mantissa trick on the host: the u of gmx_uniform_sample(k, 0, 0, 1)"""
    return ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def key_tables(chain_keys, T):
    """BootstrapBank._key_tables under the R keys `chain_keys`: ([T, R, 2], [T, R, 2]) uint32"""
    from genjax_amd.inference.smc import BootstrapBank
    from genjax_amd.random import Key
    me = types.SimpleNamespace(R=chain_keys.shape[0], T=T)
    prop, res = BootstrapBank._key_tables(me, Key(host=np.ascontiguousarray(chain_keys, dtype=np.uint32)))
    return prop.view(np.uint32), res.view(np.uint32)


def proposals(be, k_prop, j, theta, scale):
    """theta' [P, R]: the start at j = 0, else z * scale rounded, + theta rounded, z under split(split(k_prop, R)[r], P)[p]"""
    from genjax_amd.random import _derive_host
    P, R = theta.shape
    if j == 0:
        return theta.copy()
    kr = split_host(k_prop, R)
    kp = np.stack([split_host(kr[r], P) for r in range(R)]) if R <= 16 else \
        _derive_host(kr[:, None, :], np.arange(P, dtype=np.uint64))
    z = std_normal_of(be, bits_of(be, kp.reshape(-1, 2))).reshape(R, P).T
    with np.errstate(invalid="ignore", over="ignore"):
        v = (z * np.asarray(scale, np.float32)[:, None]).astype(np.float32)
        return (v + theta).astype(np.float32)


def propose_definition(be, key_words, j, theta, scale, n, T):
    P, R = theta.shape
    k_bank, k_prop, _k_acc = iter_keys(key_words, j)
    prop, res = key_tables(split_host(k_bank, R), T)
    th = proposals(be, k_prop, j, theta, scale)
    return dict(theta_prop=th, leaves=np.repeat(th, n, axis=1), keys_prop=prop, keys_res=res, it=np.array([j, j + 1], np.uint32))


# --- the entry points ---------------------------------------------------------------------------------------------------------
def run_propose(be, key_words, j, theta, scale, n, T, lead=0, pad=5):
    """the leaves are rows of ONE poisoned buffer, `lead` floats into their row: rows start at every 4-byte alignment"""
    dev = be.device
    P, R = theta.shape
    N = R * n
    it = torch.from_numpy(_i32([j, 77])).to(dev)
    th = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float32)).to(dev)
    sc = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).to(dev)
    buf = torch.full((P, lead + N + pad), float(POISON), dtype=torch.float32, device=dev)
    table = torch.tensor([buf[p].data_ptr() + 4 * lead for p in range(P)], dtype=torch.int64, device=dev)
    kp = torch.full((T, R, 2), -3, dtype=torch.int32, device=dev)
    kr = torch.full((T, R, 2), -3, dtype=torch.int32, device=dev)
    out = torch.full((P, R), float(POISON), dtype=torch.float32, device=dev)
    rc = be.c.gmx_pmmh_propose(_words(key_words), be.ptr(it), be.ptr(th), be.ptr(sc), P, R, n, T, be.ptr(kp), be.ptr(kr),
                               be.ptr(table), be.ptr(out), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    b = buf.cpu().numpy()
    assert np.all(b[:, :lead] == POISON) and np.all(b[:, lead + N:] == POISON), "the padding around a leaf was written"
    assert H.same_bits(th.cpu().numpy(), np.ascontiguousarray(theta, dtype=np.float32)), "theta was written"
    return dict(theta_prop=out.cpu().numpy(), leaves=b[:, lead:lead + N], keys_prop=kp.cpu().numpy().view(np.uint32),
                keys_res=kr.cpu().numpy().view(np.uint32), it=it.cpu().numpy().view(np.uint32))


def assert_propose_equal(got, want, what):
    assert np.array_equal(got["it"], want["it"]), (what, "it", got["it"], want["it"])
    assert np.array_equal(got["keys_prop"], want["keys_prop"]), (what, "keys_prop")
    assert np.array_equal(got["keys_res"], want["keys_res"]), (what, "keys_res")
    assert H.same_bits(got["theta_prop"], want["theta_prop"]), (what, "theta_prop", got["theta_prop"], want["theta_prop"])
    assert H.same_bits(got["leaves"], want["leaves"]), (what, "leaves", np.argwhere(got["leaves"] != want["leaves"])[:5].tolist())


def start_of(R, P, seed=0):
    rng = np.random.default_rng(1000 + seed)
    lo = np.array([PRIOR[p][0] for p in range(P)], np.float32)[:, None]
    hi = np.array([PRIOR[p][1] for p in range(P)], np.float32)[:, None]
    return (lo + (hi - lo) * rng.uniform(0.05, 0.95, size=(P, R))).astype(np.float32)


def check_propose(be, case):
    """the key tables, the proposals and the broadcast leaves, bit for bit; j = 0 leaves theta' = theta"""
    R, n, T, P, _tau = CASES[case]
    key = np.array([0x1234, 0x9ABC + R], np.uint32)
    theta, scale = start_of(R, P), np.asarray(STEP_SIZE[:P], np.float32)
    for j, lead in ((0, 0), (1, 0), (5, 1), (2 ** 32 - 2, 3)):
        got = run_propose(be, key, j, theta, scale, n, T, lead=lead)
        want = propose_definition(be, key, j, theta, scale, n, T)
        assert_propose_equal(got, want, (case, j, lead))
        if j == 0:
            assert H.same_bits(got["theta_prop"], theta)
        else:
            assert not np.any(got["theta_prop"] == theta)


def run_accept(be, key_words, it1, maxs, totals, flags, shift_ln2, log_n, lp_prop, theta, ll, lp, theta_prop, rec_base, cap,
               shift=30):
    dev = be.device
    P, R = theta.shape
    T = maxs.shape[0]

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    it = torch.from_numpy(_i32([55, it1])).to(dev)
    mx, tot = up(maxs, np.float32), torch.from_numpy(np.array(totals, dtype=np.uint64).view(np.int64)).to(dev)
    fl = None if flags is None else up(flags, np.int32)
    th, l, p_, tp, lpp = up(theta, np.float32), up(ll, np.float64), up(lp, np.float32), up(theta_prop, np.float32), up(lp_prop, np.float32)
    rt = torch.full((cap, P, R), float(POISON), dtype=torch.float32, device=dev)
    rl = torch.full((cap, R), float(POISON), dtype=torch.float64, device=dev)
    ra = torch.full((cap, R), 9, dtype=torch.uint8, device=dev)
    rb = torch.tensor([rec_base], dtype=torch.int64, device=dev)
    st = torch.zeros((1,), dtype=torch.int64, device=dev)
    rc = be.c.gmx_pmmh_accept(_words(key_words), be.ptr(it), be.ptr(mx), be.ptr(tot), be.ptr(fl), T, R, P, shift, float(shift_ln2),
                              float(log_n), be.ptr(lpp), be.ptr(th), be.ptr(l), be.ptr(p_), be.ptr(tp), be.ptr(rt), be.ptr(rl),
                              be.ptr(ra), be.ptr(rb), cap, be.ptr(st), be.stream())
    assert rc == 0, be.c.gmx_last_error()
    return dict(theta=th.cpu().numpy(), ll=l.cpu().numpy(), lp=p_.cpu().numpy(), rec_theta=rt.cpu().numpy(), rec_ll=rl.cpu().numpy(),
                rec_acc=ra.cpu().numpy(), status=int(st.item()), it=it.cpu().numpy().view(np.uint32))


# --- the evidence -------------------------------------------------------------------------------------------------------------
def evidence_reference(maxs, totals, shift, n, counted=None):
    """evidence_terms summed sequentially in float64 over the counted steps, per chain: (sum [R], bound [R]) with the bound
    16 T 2^-53 S, S the largest absolute value among the computation's terms (ref, log total, shift ln 2, log n and each
    evidence term) and running sums — one rounding per operation counted generously, plus a few ulp for gmx_log64"""
    from genjax_amd.inference.smc import cdf_reference, evidence_terms
    maxs, totals = np.asarray(maxs, np.float32), np.asarray(totals).view(np.uint64)
    T, R = maxs.shape
    terms = evidence_terms(maxs, totals.view(np.int64), shift, n)
    counted = np.ones((T, R), bool) if counted is None else np.asarray(counted, bool).copy()
    counted[T - 1] = True
    out, bound = np.zeros((R,), np.float64), np.zeros((R,), np.float64)
    with np.errstate(divide="ignore"):
        parts = np.stack([np.abs(cdf_reference(maxs)), np.abs(np.log(totals.astype(np.float64))),
                          np.full((T, R), shift * math.log(2.0)), np.full((T, R), math.log(n))])
    for r in range(R):
        acc, S, dead = 0.0, 0.0, False
        for t in range(T):
            if not counted[t, r]:
                continue
            if totals[t, r] == 0:
                dead = True
                continue
            acc = acc + terms[t, r]
            S = max(S, abs(acc), abs(terms[t, r]), float(parts[:, t, r].max()))
        out[r] = -math.inf if dead else acc
        bound[r] = 16.0 * T * 2.0 ** -53 * S
    return out, bound


def within(got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isneginf(want)
    return bool(np.array_equal(np.isneginf(got), inf) and np.all(np.abs(got[~inf] - want[~inf]) <= bound[~inf]))


def accept_case(R, T, n, with_flags, seed=3):
    """synthetic sweep statistics (never modified): chain 2 holds a zero total at a counted step; with flags, chain 4 holds
    one at a step that is not counted"""
    from genjax_amd.inference.smc import cdf_shift
    rng = np.random.default_rng(seed + 7 * R + T)
    shift = cdf_shift(n)
    maxs = (3.0 * rng.normal(size=(T, R))).astype(np.float32)
    totals = rng.integers(1, (1 << shift) * n, size=(T, R), dtype=np.uint64, endpoint=False)
    totals[0, 0], totals[T - 1, 1 % R] = 1, (np.uint64(1) << np.uint64(shift)) * np.uint64(n) - np.uint64(1)
    flags = None
    if with_flags:
        flags = rng.integers(0, 2, size=(T, R)).astype(np.int32)
        flags[:, 0] = 0
        if R > 4 and T > 1:
            flags[0, 4], totals[0, 4] = 0, 0
    if R > 2:
        totals[T - 1, 2] = 0
    return maxs, totals, flags, shift


def check_accept(be, R, T, P, n, with_flags):
    maxs, totals, flags, shift = accept_case(R, T, n, with_flags)
    key = np.array([77, 1000 + R], np.uint32)
    it1, rec_base, cap = 8, 5, 4                       # iteration j = 7 lands in row 2 of 4
    j, row = it1 - 1, it1 - 1 - rec_base
    _kb, _kp, k_acc = iter_keys(key, j)
    shift_ln2, log_n = shift * math.log(2.0), math.log(n)
    rng = np.random.default_rng(R + T)
    theta, theta_prop = start_of(R, P), start_of(R, P, seed=1)
    zeros, minf = np.zeros((R,), np.float32), np.full((R,), -np.inf)
    # A. against a chain that holds nothing (ll = -inf, lp = 0): every chain with mass accepts, and records its evidence
    a = run_accept(be, key, it1, maxs, totals, flags, shift_ln2, log_n, zeros, theta, minf, zeros, theta_prop, rec_base, cap, shift)
    want_ll, bound = evidence_reference(maxs, totals, shift, n, None if flags is None else flags != 0)
    err = np.abs(a["ll"][np.isfinite(want_ll)] - want_ll[np.isfinite(want_ll)])
    print("evidence against evidence_terms summed in float64: largest error", err.max(), "smallest bound", bound[np.isfinite(want_ll)].min())
    assert within(a["ll"], want_ll, bound), (a["ll"], want_ll, bound)
    alive = np.isfinite(want_ll)
    if R > 2:
        assert not alive[2] and (not with_flags or R <= 4 or T == 1 or alive[4])
    assert np.array_equal(a["rec_acc"][row], alive.astype(np.uint8))
    assert H.same_bits(a["theta"], np.where(alive[None, :], theta_prop, theta))
    assert a["status"] == 0 and a["it"].tolist() == [it1, it1]
    ll_new = a["ll"]
    # B. against a state: the float32 log_alpha, the uniform, the select and the record are exact
    ll_old = np.where(alive, ll_new, -5.0) + rng.normal(size=(R,))
    lp = rng.normal(size=(R,)).astype(np.float32)
    lp_prop = rng.normal(size=(R,)).astype(np.float32)
    lp_prop[0] = -np.inf
    if R > 3:
        lp_prop[1], ll_old[3] = np.nan, -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        log_alpha = ((ll_new - ll_old) + (lp_prop.astype(np.float64) - lp.astype(np.float64))).astype(np.float32)
    take = mh_accept_of(be, split_host(k_acc, R), log_alpha) != 0
    assert not take[0] and (R <= 3 or (not take[1] and take[3] == bool(alive[3] and lp_prop[3] > -np.inf)))
    assert take.any() and not take.all(), take
    b = run_accept(be, key, it1, maxs, totals, flags, shift_ln2, log_n, lp_prop, theta, ll_old, lp, theta_prop, rec_base, cap, shift)
    want = dict(theta=np.where(take[None, :], theta_prop, theta), ll=np.where(take, ll_new, ll_old), lp=np.where(take, lp_prop, lp))
    assert np.array_equal(b["rec_acc"][row], take.astype(np.uint8)), (b["rec_acc"][row], take)
    assert H.same_bits(b["theta"], want["theta"]) and H.same_bits(b["rec_theta"][row], want["theta"])
    assert np.array_equal(b["ll"].view(np.uint64), want["ll"].view(np.uint64)) and np.array_equal(b["rec_ll"][row].view(np.uint64), want["ll"].view(np.uint64))
    assert H.same_bits(np.nan_to_num(b["lp"], nan=7.0), np.nan_to_num(want["lp"], nan=7.0))
    others = [k for k in range(cap) if k != row]
    assert np.all(b["rec_theta"][others] == POISON) and np.all(b["rec_ll"][others] == POISON) and np.all(b["rec_acc"][others] == 9)
    assert b["status"] == 0 and b["it"].tolist() == [it1, it1]
    # C. a record row outside [0, cap): nothing recorded, nothing changed, counted; the iteration word still advances
    for base in (it1, it1 - 1 - cap):
        c = run_accept(be, key, it1, maxs, totals, flags, shift_ln2, log_n, lp_prop, theta, ll_old, lp, theta_prop, base, cap, shift)
        assert c["status"] == 1 and c["it"].tolist() == [it1, it1], (base, c["status"], c["it"])
        assert H.same_bits(c["theta"], theta) and np.array_equal(c["ll"].view(np.uint64), ll_old.view(np.uint64))
        assert np.all(c["rec_theta"] == POISON) and np.all(c["rec_ll"] == POISON) and np.all(c["rec_acc"] == 9)


# --- gmx_log64 ----------------------------------------------------------------------------------------------------------------
LOG64_ULP_BOUND = 4.0


@functools.lru_cache(maxsize=None)
def log64_totals():
    """1, the powers of two up to 2^61 and their neighbours, 2^62 - 1, and 4000 random values of up to 62 bits"""
    rng = np.random.default_rng(64)
    v = [1, 2, 3, (1 << 62) - 1]
    for k in range(2, 62):
        v += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    v += [int(x) >> int(s) for x, s in zip(rng.integers(1 << 61, 1 << 62, size=4000, dtype=np.uint64),
                                           rng.integers(0, 50, size=4000))]
    out = np.array(v, dtype=np.uint64)
    out.setflags(write=False)
    return out


def log64_of(be, totals):
    """gmx_log64 through gmx_pmmh_accept: T = 1, a maximum of 0 (reference 0), shift ln 2 = log n = 0, against an empty chain
    — the recorded evidence is ((0 + log64(total)) - 0) - 0"""
    R = totals.size
    z = np.zeros((R,), np.float32)
    th = np.zeros((1, R), np.float32)
    out = run_accept(be, [1, 2], 1, np.zeros((1, R), np.float32), totals.reshape(1, R), None, 0.0, 0.0, z, th,
                     np.full((R,), -np.inf), z, th, 0, 1)
    assert out["rec_acc"].all()
    return out["rec_ll"][0]


def log64_ulp_errors(be):
    totals = log64_totals()
    got, want = log64_of(be, totals), np.log(totals.astype(np.float64))
    assert got[0] == 0.0 and totals[0] == 1
    return np.abs(got - want) / np.spacing(np.where(want == 0.0, 1.0, want))


def check_log64(be):
    err = log64_ulp_errors(be)
    print("gmx_log64 against numpy's log: largest error", err.max(), "ulp over", err.size, "totals; bound", LOG64_ULP_BOUND)
    assert err.max() <= LOG64_ULP_BOUND, err.max()


# --- refusals ----------------------------------------------------------------------------------------------------------------
def refusal_calls():
    """(entry point, arguments, what the message has to name) the two entry points must refuse before any launch"""
    N, i64, i32, dbl = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    buf = (ctypes.c_int64 * 8)()
    Pt = ctypes.cast(buf, ctypes.c_void_p)
    key = (ctypes.c_uint32 * 2)(1, 2)

    def propose(key=key, it=Pt, theta=Pt, scale=Pt, P=2, R=3, n=4, T=2, kp=Pt, kr=Pt, leaves=Pt, out=Pt):
        return (key, it, theta, scale, i32(P), i64(R), i64(n), i32(T), kp, kr, leaves, out, N)

    def accept(key=key, it=Pt, maxs=Pt, totals=Pt, flags=N, T=2, R=3, P=2, shift=30, lp_prop=Pt, theta=Pt, ll=Pt, lp=Pt,
               theta_prop=Pt, rt=Pt, rl=Pt, ra=Pt, rb=Pt, cap=4, status=Pt):
        return (key, it, maxs, totals, flags, i32(T), i64(R), i32(P), ctypes.c_int(shift), dbl(1.0), dbl(1.0), lp_prop, theta, ll, lp,
                theta_prop, rt, rl, ra, rb, i64(cap), status, N)
    calls = [("gmx_pmmh_propose", propose(**{a: None if a == "key" else N}), b"null")
             for a in ("key", "it", "theta", "scale", "kp", "kr", "leaves", "out")]
    calls += [("gmx_pmmh_propose", propose(P=0), b"P = 0 is outside [1, 8]"), ("gmx_pmmh_propose", propose(P=9), b"P = 9"),
              ("gmx_pmmh_propose", propose(R=0), b"R = 0"), ("gmx_pmmh_propose", propose(n=0), b"n = 0"),
              ("gmx_pmmh_propose", propose(T=0), b"T = 0"), ("gmx_pmmh_propose", propose(R=2 ** 20, n=2 ** 11), b"R * n = 2147483648"),
              ("gmx_pmmh_propose", propose(R=2 ** 30, n=1, T=2), b"T * R = 2147483648")]
    calls += [("gmx_pmmh_accept", accept(**{a: None if a == "key" else N}), b"null")
              for a in ("key", "it", "maxs", "totals", "lp_prop", "theta", "ll", "lp", "theta_prop", "rt", "rl", "ra", "rb", "status")]
    calls += [("gmx_pmmh_accept", accept(P=9), b"P = 9"), ("gmx_pmmh_accept", accept(R=2 ** 31), b"R = 2147483648"),
              ("gmx_pmmh_accept", accept(T=-1), b"T = -1"), ("gmx_pmmh_accept", accept(shift=0), b"shift = 0"),
              ("gmx_pmmh_accept", accept(shift=63), b"shift = 63"), ("gmx_pmmh_accept", accept(cap=0), b"cap = 0"),
              ("gmx_pmmh_accept", accept(cap=2 ** 32 + 1), b"cap = 4294967297")]
    return calls, (buf, key)


def refusal_messages(lib):
    """lib: a ctypes library (the HIP library without a GPU, or the mirror): every call refused, naming what it refuses"""
    lib.gmx_last_error.restype = ctypes.c_char_p
    lib.gmx_pmmh_propose.argtypes = None
    lib.gmx_pmmh_accept.argtypes = None
    calls, _keep = refusal_calls()
    out = []
    for name, args, names in calls:
        assert getattr(lib, name)(*args) != 0, (name, names)
        msg = lib.gmx_last_error()
        assert name.encode() in msg and names in msg, (msg, names)
        out.append(msg)
    return out


# --- the models ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def models(P):
    """the LGSSM of workloads.make_lgssm with its transition coefficient (P = 1) and its process-noise scale (P = 2) as
    parameters, a uniform prior on each: (init, step, prior, param_addrs)"""
    import genjax_amd as G
    from genjax_amd import workloads
    p = workloads.LGSSM
    sy, s0, sx0 = p["sy"], p["s0"], p["sx"]
    if P == 1:
        @G.gen
        def init(a):
            x = G.normal(0.0, s0) @ "x"
            _ = G.normal(x, sy) @ "y"
            return x

        @G.gen
        def step(x_prev, a):
            x = G.normal(a * x_prev, sx0) @ "x"
            _ = G.normal(x, sy) @ "y"
            return x

        @G.gen
        def prior():
            a = G.uniform(PRIOR[0][0], PRIOR[0][1]) @ "a"
            return a
        return init, step, prior, ("a",)

    @G.gen
    def init(a, sx):
        x = G.normal(0.0, s0) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x

    @G.gen
    def step(x_prev, a, sx):
        x = G.normal(a * x_prev, sx) @ "x"
        _ = G.normal(x, sy) @ "y"
        return x

    @G.gen
    def prior():
        a = G.uniform(PRIOR[0][0], PRIOR[0][1]) @ "a"
        _ = G.uniform(PRIOR[1][0], PRIOR[1][1]) @ "sx"
        return a
    return init, step, prior, ("a", "sx")


def _data(T):
    from genjax_amd import workloads
    return torch.from_numpy(workloads.lgssm_data(T))


def make_chain(case, specialize, max_iters=ITERS):
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleMH
    R, n, T, P, tau = CASES[case]
    init, step, prior, addrs = models(P)
    pm = ParticleMH(init, step, prior, n, R, T, addrs, STEP_SIZE[:P], ess_threshold=tau, specialize=specialize)
    th0 = start_of(R, P, seed=2)
    return pm.prepare(G.key(SEED), _data(T), tuple(torch.from_numpy(th0[p].copy()) for p in range(P)), max_iters)


def _np(t):
    return t.detach().cpu().numpy()


def snapshot(pm, res):
    """everything check 3 compares: the record slabs, the final state, the key tables, the iteration words"""
    th, ll, lp = pm.state()
    return dict(theta=_np(res.theta), log_ml=_np(res.log_ml), accepted=_np(res.accepted), s_theta=_np(th), s_ll=_np(ll), s_lp=_np(lp),
                keys_prop=_np(pm.bank.keys_prop), keys_res=_np(pm.bank.keys_res), it=_np(pm.it), theta_prop=_np(pm.theta_prop),
                maxs=_np(pm.bank.maxs), totals=_np(pm.bank.totals))


def assert_same_run(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else \
            (H.same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y))
        assert same, (what, k)


@functools.lru_cache(maxsize=None)
def run_of(device_type, case, specialize):
    """ParticleMH.run(6) of a case, once per backend (never modified)"""
    pm = make_chain(case, specialize)
    return snapshot(pm, pm.run(ITERS))


# --- the chain is the composition ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def composed_chain(device_type, case, specialize):
    """The same chain as a Python loop over public parts, once per backend: per iteration a fresh
    BootstrapBank(params=theta').prepare(split(k_bank, R), ys), its maxs / totals and log_ml(), prior.assess, and
    gmx_mh_accept on the float32 log_alpha.  Asserts that no decision is a near-tie."""
    import genjax_amd as G
    from genjax_amd import _lib
    from genjax_amd.core.choice_map import ChoiceMap
    from genjax_amd.inference.smc import BootstrapBank
    from genjax_amd.random import Key
    be = _lib.get()
    R, n, T, P, tau = CASES[case]
    init, step, prior, addrs = models(P)
    key = np.asarray(G.key(SEED).host(), np.uint32)
    theta = start_of(R, P, seed=2)
    scale = np.asarray(STEP_SIZE[:P], np.float32)
    ll, lp = np.full((R,), -np.inf), np.zeros((R,), np.float32)
    out = []
    for j in range(ITERS):
        k_bank, k_prop, k_acc = iter_keys(key, j)
        th = proposals(be, k_prop, j, theta, scale)
        bank = BootstrapBank(init, step, n, R, T, params=tuple(torch.from_numpy(th[p].copy()) for p in range(P)),
                             ess_threshold=tau, specialize=specialize)
        bank.prepare(Key(host=split_host(k_bank, R)), _data(T)).launch()
        ll_new = bank.log_ml()
        con = ChoiceMap.empty()
        for p, a in enumerate(addrs):
            con = con.set(a, torch.from_numpy(th[p].copy()).to(be.device))
        lp_new = _np(prior.assess(con, (), batch_shape=(R,))[0]).astype(np.float32).reshape(R)
        with np.errstate(invalid="ignore", over="ignore"):
            log_alpha = ((ll_new - ll) + (lp_new.astype(np.float64) - lp.astype(np.float64))).astype(np.float32)
        keys = split_host(k_acc, R)
        take = mh_accept_of(be, keys, log_alpha) != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.abs(np.log(unit_of(bits_of(be, keys)).astype(np.float64)) - log_alpha.astype(np.float64))
        assert not np.any(gap < NEAR_TIE), (case, j, "a decision of the reference is a near-tie: choose another SEED", gap.min())
        flags = _np(bank.flags) != 0 if tau is not None else None
        theta = np.where(take[None, :], th, theta)
        ll, lp = np.where(take, ll_new, ll), np.where(take, lp_new, lp)
        out.append(dict(theta_prop=th, maxs=_np(bank.maxs), totals=_np(bank.totals), flags=flags, ll_new=ll_new, take=take,
                        theta=theta.copy(), ll=ll.copy(), lp_new=lp_new, shift=bank.shift))
    return out


def check_chain_is_the_composition(be, case, specialize):
    R, n, T, P, tau = CASES[case]
    want = composed_chain(be.device.type, case, specialize)
    takes = np.stack([w["take"] for w in want])
    print("composed chain", case, ": accepted", int(takes.sum()), "of", takes.size, "; proposals outside the prior",
          int(sum(np.isneginf(w["lp_new"]).sum() for w in want)))
    assert takes[0].all() and not takes[1:].all() and takes[1:].any()
    if tau is not None:
        flags = np.stack([w["flags"] for w in want])
        assert flags.any() and not flags.all(), "both outcomes of the adaptive decision must occur"
    # iteration by iteration: theta', maxs and totals bit-equal, the evidence within its bound, every decision equal
    pm = make_chain(case, specialize)
    for j, w in enumerate(want):
        res = pm.run(1)
        assert H.same_bits(_np(pm.theta_prop), w["theta_prop"]), (case, j, "theta'")
        assert H.same_bits(_np(pm.bank.maxs), w["maxs"]) and np.array_equal(_np(pm.bank.totals), w["totals"]), (case, j, "maxs / totals")
        assert np.array_equal(_np(res.accepted)[0], w["take"]), (case, j, "decisions", _np(res.accepted)[0], w["take"])
        ref, bound = evidence_reference(w["maxs"], w["totals"], w["shift"], n, w["flags"])
        assert within(np.where(w["take"], _np(res.log_ml)[0], ref), ref, bound), (case, j, "evidence")
        assert within(w["ll_new"], ref, bound), (case, j, "log_ml() of the composed bank")
        assert H.same_bits(_np(res.theta)[0], w["theta"]), (case, j, "theta")
    assert _np(pm.it).tolist() == [ITERS, ITERS] and int(pm.status.item()) == 0
    stepped = snapshot(pm, types.SimpleNamespace(theta=pm.rec_theta[:1], log_ml=pm.rec_ll[:1], accepted=pm.rec_acc[:1] != 0))
    # run(6) in one go, and as two run(3): the same records and the same final state, bit for bit
    whole = run_of(be.device.type, case, specialize)
    for k in ("s_theta", "s_ll", "s_lp", "keys_prop", "keys_res", "it", "theta_prop", "maxs", "totals"):
        assert_same_run({k: stepped[k]}, {k: whole[k]}, (case, "run(1) x 6 against run(6)"))
    assert np.array_equal(whole["accepted"], takes) and H.same_bits(whole["theta"], np.stack([w["theta"] for w in want]))
    pm = make_chain(case, specialize)
    first, second = pm.run(3), pm.run(3)
    halves = snapshot(pm, types.SimpleNamespace(theta=torch.cat([first.theta, second.theta]), log_ml=torch.cat([first.log_ml, second.log_ml]),
                                                accepted=torch.cat([first.accepted, second.accepted])))
    assert_same_run(halves, whole, (case, "run(3) + run(3) against run(6)"))
    import pytest
    with pytest.raises(ValueError, match="max_iters"):
        pm.run(1)


def check_captured(be, case, specialize):
    """capture() leaves the chains where they were; replays agree with the uncaptured run bit for bit"""
    whole = run_of(be.device.type, case, specialize)
    pm = make_chain(case, specialize)
    before = [t.clone() for t in (pm.it, pm.theta, pm.ll, pm.lp, pm.rec_base, pm.status)]
    pm.capture()
    assert pm.graph is not None
    for was, now in zip(before, (pm.it, pm.theta, pm.ll, pm.lp, pm.rec_base, pm.status)):
        assert torch.equal(was.cpu(), now.cpu()) or (was.dtype.is_floating_point and H.same_bits(_np(was), _np(now)))
    assert_same_run(snapshot(pm, pm.run(ITERS)), whole, (case, "captured"))


def check_device_is_the_mirror(be, case):
    """every record slab, the final state, the key tables and the iteration words of the device equal the mirror's"""
    import genjax_amd as G
    import tests.hostsim as hs
    from genjax_amd import _lib
    assert be.device.type == "cuda"
    pm = make_chain(case, specialize=True)
    got = snapshot(pm, pm.run(ITERS))
    G.clear_caches()
    hs.install()
    try:
        pm = make_chain(case, specialize=False)
        want = snapshot(pm, pm.run(ITERS))
    finally:
        hs.uninstall()
        G.clear_caches()
        _lib.install(None)
    assert_same_run(got, want, (case, "device against mirror"))


# --- the API's refusals -----------------------------------------------------------------------------------------------------------
def check_api_refusals(be):
    import pytest
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleMH
    init, step, prior, addrs = models(2)
    R, n, T = 3, 8, 2
    ys = _data(T)
    th0 = tuple(torch.from_numpy(start_of(R, 2)[p].copy()) for p in range(2))

    def make(**kw):
        a = dict(init=init, step=step, prior=prior, n_particles=n, n_chains=R, T=T, param_addrs=addrs, step_size=STEP_SIZE,
                 specialize=False)
        a.update(kw)
        return ParticleMH(**a)
    pm = make()
    with pytest.raises(ValueError, match="ONE key"):
        pm.prepare(G.split(G.key(1), R), ys, th0, 4)
    for bad in (th0[:1], (th0[0], th0[1][:2]), (th0[0].reshape(1, R), th0[1])):
        with pytest.raises(ValueError, match="theta0"):
            pm.prepare(G.key(1), ys, bad, 4)
    for bad in ((0.1,), (0.1, 0.0), (0.1, -0.2), (0.1, math.nan), 0.1):
        with pytest.raises(ValueError, match="step_size"):
            make(step_size=bad)
    with pytest.raises(NotImplementedError, match="between 1 and 8"):
        make(param_addrs=tuple("p%d" % i for i in range(9)), step_size=(0.1,) * 9)
    with pytest.raises(NotImplementedError, match="between 1 and 8"):
        make(param_addrs=(), step_size=())
    _i1, _s1, prior1, _a1 = models(1)
    with pytest.raises(ValueError, match="param_addrs"):            # the prior has no site "sx"
        make(prior=prior1).prepare(G.key(1), ys, th0, 4)
    with pytest.raises(ValueError, match="param_addrs"):            # the prior samples "sx", which is not a parameter
        i1, s1, _p1, a1 = models(1)
        ParticleMH(i1, s1, prior, n, R, T, a1, STEP_SIZE[:1], specialize=False).prepare(G.key(1), ys, th0[:1], 4)
    for bad in (0, 2 ** 32):
        with pytest.raises(ValueError, match="max_iters"):
            pm.prepare(G.key(1), ys, th0, bad)
    pm.prepare(G.key(1), ys, th0, 2)
    pm.run(2)
    with pytest.raises(ValueError, match="max_iters"):
        pm.run(1)
    for kw in (dict(rejuvenate=object()), dict(history=True), dict(comm=object()), dict(noise_ahead=True)):
        with pytest.raises(NotImplementedError, match="BootstrapBank"):
            make(**kw)
    with pytest.raises(NotImplementedError, match="1024"):
        make(n_particles=1025, ess_threshold=0.5)


# --- the law ---------------------------------------------------------------------------------------------------------------------
LAW_R, LAW_N, LAW_T, LAW_ITERS, LAW_STEP, LAW_SEED = 1024, 64, 8, 200, 0.15, 777


def law_start():
    lo, hi = PRIOR[0]
    return (lo + (hi - lo) * (np.arange(LAW_R) + 0.5) / LAW_R).astype(np.float32)      # dispersed over the prior's support


@functools.lru_cache(maxsize=None)
def exact_posterior():
    """(mean, sd, second moment, sd of the second moment) of the transition coefficient given the data: the Kalman likelihood
    on a fine grid times the uniform prior, float64"""
    from genjax_amd import workloads
    ys = workloads.lgssm_data(LAW_T)
    lo, hi = PRIOR[0]
    a = np.linspace(lo, hi, 20001)
    ll = np.array([workloads.kalman_log_ml(ys, dict(workloads.LGSSM, a=float(v))) for v in a])
    w = np.exp(ll - ll.max())
    w[0] *= 0.5
    w[-1] *= 0.5
    w /= w.sum()
    m1, m2, m4 = float(np.sum(w * a)), float(np.sum(w * a ** 2)), float(np.sum(w * a ** 4))
    return m1, math.sqrt(m2 - m1 * m1), m2, math.sqrt(m4 - m2 * m2)


def law_z_scores(a_last):
    a_last = np.asarray(a_last, np.float64)
    m1, sd1, m2, sd2 = exact_posterior()
    return (a_last.mean() - m1) / (sd1 / math.sqrt(a_last.size)), ((a_last ** 2).mean() - m2) / (sd2 / math.sqrt(a_last.size))


def numpy_pmmh_reference(seed=1):
    """The same design in float64 numpy with numpy's own generator (a bootstrap filter with multinomial resampling at every
    step): theta of the R chains after LAW_ITERS iterations.  What says that 200 iterations at this step size leave no
    burn-in bias the bound could see."""
    from genjax_amd import workloads
    p = workloads.LGSSM
    ys = workloads.lgssm_data(LAW_T).astype(np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = PRIOR[0]
    R, n = LAW_R, LAW_N

    def evidence(a):
        x = p["s0"] * rng.normal(size=(R, n))
        out = np.zeros((R,))
        for t in range(LAW_T):
            if t > 0:
                x = a[:, None] * x + p["sx"] * rng.normal(size=(R, n))
            lw = -0.5 * ((ys[t] - x) / p["sy"]) ** 2 - math.log(p["sy"]) - 0.5 * math.log(2 * math.pi)
            m = lw.max(axis=1, keepdims=True)
            w = np.exp(lw - m)
            out += m[:, 0] + np.log(w.mean(axis=1))
            c = np.cumsum(w, axis=1)
            u = rng.uniform(size=(R, n)) * c[:, -1:]
            idx = np.minimum((c[:, None, :] < u[:, :, None]).sum(axis=2), n - 1)
            x = np.take_along_axis(x, idx, axis=1)
        return out
    a = law_start().astype(np.float64)
    ll = evidence(a)
    for _ in range(1, LAW_ITERS):
        prop = a + LAW_STEP * rng.normal(size=(R,))
        inside = (prop >= lo) & (prop <= hi)
        ll_new = evidence(np.where(inside, prop, a))
        take = inside & (np.log(rng.uniform(size=(R,))) < ll_new - ll)
        a, ll = np.where(take, prop, a), np.where(take, ll_new, ll)
    return a


def check_law(be, specialize=True):
    import genjax_amd as G
    from genjax_amd.inference.smc import ParticleMH
    init, step, prior, addrs = models(1)
    pm = ParticleMH(init, step, prior, LAW_N, LAW_R, LAW_T, addrs, (LAW_STEP,), specialize=specialize)
    pm.prepare(G.key(LAW_SEED), _data(LAW_T), (torch.from_numpy(law_start()),), LAW_ITERS).capture()
    res = pm.run(LAW_ITERS)
    a_last = _np(res.theta)[-1, 0]
    lo, hi = PRIOR[0]
    assert np.all((a_last >= lo) & (a_last <= hi))
    z1, z2 = law_z_scores(a_last)
    print("law: acceptance rate", float(_np(res.accepted)[1:].mean()), "exact posterior (mean, sd, second moment, its sd)",
          exact_posterior(), "z of the mean", z1, "z of the second moment", z2)
    assert abs(z1) <= 5.0 and abs(z2) <= 5.0, (z1, z2)
