"""The branch-length gradient in one engine call (paml_amd_gradient) next to what it replaces, in the same process:
    one evaluation (paml_amd_eval), the batch of 2 (n_nodes - 1) branch-perturbed evaluations of a central-difference gradient
    (paml_amd_eval_batch), and the gradient call — wall time of each (the fastest of three after a warm call) and the gradient's kernels by
    HIP events (paml_amd_gradient_info) — at HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns
    at 4 states with four classes;
    the maximum-likelihood searches of HIV M0, HIV M2a and lysozyme branch-site A (pamlh_optimize) with and without
    pamlh_use_analytic_gradient: wall time, n_eval, lnL.
    python tools/gradient_timing.py > profiles/gradient_times.txt"""
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
    rows = []
    for v in range(t.n_nodes):
        if v != t.root:
            for s in (1, -1):
                b = t.branch.copy()
                b[v] += s * 1e-6 * (b[v] + 1)
                rows.append(b)
    rows = np.stack(rows)
    gr = None if pb.n_genes == 1 else np.tile(pb.gene_rate, (len(rows), 1))
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    t_batch = best_of(lambda: eng.eval_batch(rows, gene_rate=gr))
    t_grad = best_of(lambda: eng.gradient(t.branch, pb.gene_rate))
    info = engine.gradient_info()
    t_scores = best_of(lambda: eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True))
    print("%-44s %2d nodes, kernel %s: eval %.3f ms; eval_batch of %d %.3f ms; gradient %.3f ms (kernels %.3f ms, %d batches; with lnf and scores returned %.3f ms)"
          " -> %.1f evaluations, %.2fx the batch" % (label, t.n_nodes, eng.kernel_name, t_eval * 1e3, len(rows), t_batch * 1e3, t_grad * 1e3, info["last_kernel_ms"],
                                                   info["last_batches"], t_scores * 1e3, t_grad / t_eval, t_batch / t_grad), flush=True)
    eng.close()


def search(label, ctl, prog):
    for analytic in (False, True):
        a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
        t0 = time.perf_counter()
        r = a.optimize(a.default_x(), analytic_gradient=analytic)
        print("%-28s %-26s %.2f s, n_eval %5d, lnL %.6f, converged %s" % (label, "analytic branch gradient" if analytic else "differences (default)", time.perf_counter() - t0,
                                                                       r["n_eval"], r["lnL"], r["converged"]), flush=True)


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    search("HIV M0", "hiv_ns0.ctl", "codeml")
    search("HIV M2a", "hiv_ns2.ctl", "codeml")
    search("lysozyme branch-site A", "lyso_bsa.ctl", "codeml")
