"""The site programs a fixed list of workloads builds, as digests: one line per workload — name, number of programs,
engine.program_digest().hex() — on the CPU mirror (tests/hostsim).  Two trees that print the same lines trace the same
programs word for word: what a change to the host code that BUILDS programs (static.py, engine.py, the builders in
inference/) is held to.  The list reaches every place a traced program is opened; the arguments are those of the CPU
tests.  No GPU:

    python tools/program_digests.py > profiles/program_digests_<label>.txt
"""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workloads(be):
    from tests import ancestor_checks, backward_checks, grad_checks, parity, pgbs_checks, pgibbs_checks, pmmh_checks
    sweep = dict(ancestors_equal=True, x_equal=True, totals_equal=True)

    def lgssm(**kw):
        res = parity.check_lgssm_sweep(**kw)
        assert all(res[k] for k in sweep), res

    W = [("check_scan(257, 6)", lambda: parity.check_scan(n=257, T=6)),
         ("check_scan_long(257, 100)", lambda: parity.check_scan_long(n=257, T=100)),
         ("check_scan_long(64, 17)", lambda: parity.check_scan_long(n=64, T=17))]
    W += [("check_many_sites(%d)" % ns, lambda ns=ns: parity.check_many_sites(ns=ns)) for ns in (32, 40, 200)]
    W += [("check_many_sites(67, 130, seed=8)",
           lambda: parity.check_many_sites(ns=67, B=130, seed=8, kinds=("normal", "flip", "normal", "uniform"))),
          ("check_deferred_plate(64, 4096)", lambda: parity.check_deferred_plate(B=64, n=4096)),
          ("check_deferred_plate(37, 8195, seed=5)", lambda: parity.check_deferred_plate(B=37, n=4096 * 2 + 3, seed=5)),
          ("check_plates_long(130, 40)", lambda: parity.check_plates_long(n=130, P=40)),
          ("check_plates_long(33, 17, seed=2)", lambda: parity.check_plates_long(n=33, P=17, seed=2)),
          ("check_plate_edits(257)", lambda: parity.check_plate_edits(n=257)),
          ("check_nlssm_mh(1200, 4)", lambda: parity.check_nlssm_mh(n=1200, T=4)),
          ("check_nlssm_mh_sweep(1500, 4)", lambda: parity.check_nlssm_mh_sweep(n=1500, T=4)),
          ("check_nlssm_mh_sweep(1500, 5, chained)",
           lambda: parity.check_nlssm_mh_sweep(n=1500, T=5, want_chained=True, chain_mh=True)),
          ("check_nlssm_mh_sweep(1500, 5, two launches)",
           lambda: parity.check_nlssm_mh_sweep(n=1500, T=5, want_chained=False, chain_mh=False)),
          ("check_nlssm_mh_sweep(1500, 7, noise_ahead)", lambda: parity.check_nlssm_mh_sweep(n=1500, T=7, noise_ahead=True)),
          ("check_lgssm_sweep(3000, 5)", lambda: lgssm(n=3000, T=5)),
          ("check_lgssm_sweep(3000, 23, noise_ahead)", lambda: lgssm(n=3000, T=23, noise_ahead=True)),
          ("check_lgssm_sweep(3000, 23, noise_ahead, stratified)",
           lambda: lgssm(n=3000, T=23, noise_ahead=True, resample="stratified")),
          ("check_hmc(257)", lambda: parity.check_hmc(n=257)),
          ("check_mixture_gibbs_through_the_plate(5000)", lambda: parity.check_mixture_gibbs_through_the_plate(n=5000)),
          ("grad_checks.check_constant_gradients_are_tensors", lambda: grad_checks.check_constant_gradients_are_tensors(be)),
          ("backward_checks.check_backward_lgssm", lambda: backward_checks.check_backward_lgssm(False))]
    W += [("ancestor_checks.check_oracle_replay(%d)" % n,
           lambda n=n: ancestor_checks.check_oracle_replay(be, specialize=False, n=n)) for n in (200, 1500)]
    W += [("pgbs_checks.check_oracle_replay(%d, retained=%s, ancestors=%s)" % (n, r, a),
           lambda n=n, r=r, a=a: pgbs_checks.check_oracle_replay(be, specialize=False, n=n, retained=r, ancestors=a))
          for n in (200,) for r in (False, True) for a in (False, True)]
    W += [("pmmh_checks.check_chain_is_the_composition(%s)" % c,
           lambda c=c: pmmh_checks.check_chain_is_the_composition(be, c, specialize=False)) for c in ("tiny", "ess")]
    W += [("pgibbs_checks.check_chain_is_the_composition(%s)" % pgibbs_checks.chain_id(c),
           lambda c=c: pgibbs_checks.check_chain_is_the_composition(be, c, specialize=False))
          for c in (("tiny", False, False), ("tiny", True, False), ("one", False, False))]
    return W


def main():
    import tests.hostsim as hs
    from oracle import genjax_oracle as O
    O.build()
    be = hs.install()
    from genjax_amd import engine
    for name, run in workloads(be):
        engine.clear_caches()
        with engine.program_digest() as d, contextlib.redirect_stdout(sys.stderr):     # (the checks print; the lines stay clean)
            run()
        print(f"{name}\t{len(d._set)}\t{d.hex()}", flush=True)
    hs.uninstall()


if __name__ == "__main__":
    main()
