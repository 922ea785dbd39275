"""The gradient over the engine's inputs in one call (paml_amd_model_gradient) next to the branch-length gradient call
(paml_amd_gradient) on the same engine: wall time of each (the fastest of three after a warm call) and the kernels by HIP events — at
HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns at 4 states with four classes, and a
many-parameter case (HIV M0 with estimated codon frequencies, FMutSel: tests/golden/ctl/hiv_fmutsel_est.ctl);
    pamlh_gradient_full next to pamlh_gradient (the branch lengths from the engine, every other parameter differenced) on the two HIV
    cases, and their maximum-likelihood searches with pamlh_use_analytic_gradient 0 / 1 / 2: wall time, n_eval, lnL.
    python tools/modelgrad_timing.py > profiles/modelgrad_times.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, hostlib, synth      # noqa: E402

CTL = os.path.join(ROOT, "tests", "golden", "ctl")


def best_of(f, n=3):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def run(label, pb):
    eng = engine.engine_for(pb)
    t = pb.tree
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    t_grad = best_of(lambda: eng.gradient(t.branch, pb.gene_rate))
    g_ms = engine.gradient_info()["last_kernel_ms"]
    t_full = best_of(lambda: eng.model_gradient(t.branch, pb.gene_rate))
    info = engine.model_gradient_info()
    print("%-46s %2d nodes, %2d states, K %d, kernel %s: eval %.3f ms; gradient %.3f ms (kernels %.3f ms); model_gradient %.3f ms (kernels %.3f ms, %d batches)"
          " -> %.2f gradient calls, %.1f evaluations" % (label, t.n_nodes, pb.n, pb.K, eng.kernel_name, t_eval * 1e3, t_grad * 1e3, g_ms, t_full * 1e3, info["last_kernel_ms"],
                                                        info["last_batches"], t_full / t_grad, t_full / t_eval), flush=True)
    eng.close()


def host(label, ctl):
    a = hostlib.Analysis(os.path.join(CTL, ctl), "codeml")
    x = np.array(a.default_x())
    t_part = best_of(lambda: a.gradient(x))
    t_full = best_of(lambda: a.gradient_full(x))
    print("%-46s np %3d (%d branch lengths): pamlh_gradient %.3f ms; pamlh_gradient_full %.3f ms -> %.2fx" % (label, a.np, a.ntime, t_part * 1e3, t_full * 1e3, t_part / t_full), flush=True)
    for mode, name in ((0, "differences (default)"), (1, "analytic branch gradient"), (2, "full gradient, one call")):
        b = hostlib.Analysis(os.path.join(CTL, ctl), "codeml")
        t0 = time.perf_counter()
        r = b.optimize(b.default_x(), analytic_gradient=mode)
        print("%-46s %-26s %.2f s, n_eval %5d, lnL %.6f, converged %s" % (label, name, time.perf_counter() - t0, r["n_eval"], r["lnL"], r["converged"]), flush=True)


if __name__ == "__main__":
    for ctl, label in (("hiv_ns0.ctl", "HIV M0, 13 taxa x 79 codon patterns"), ("hiv_fmutsel_est.ctl", "HIV M0 FMutSel, estimated codon frequencies")):
        a = hostlib.Analysis(os.path.join(CTL, ctl), "codeml")
        run(label, a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    host("HIV M0", "hiv_ns0.ctl")
    host("HIV M0 FMutSel, estimated codon frequencies", "hiv_fmutsel_est.ctl")
