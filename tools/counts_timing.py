"""Expected substitution counts in one call (paml_amd_subst_counts) next to the branch-length gradient call (paml_amd_gradient), the
curvature call and the model-gradient call on the same engine: wall time of each (the fastest of three after a warm call) and the kernels
by HIP events — at HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon patterns and 32 taxa x 10^5 patterns at 4 states with four
classes; with 2 and with 8 labels, with and without the per-pattern array.  Every time is also given in gradient calls, beside the
product count's estimate: the passes (model_gradient's, of which the W products are not run: the estimate takes the gradient call for
them) plus n_lab x (curvature - gradient), the cost of one more product and dot product per non-root node and class.
    python tools/counts_timing.py > profiles/counts_times.txt"""
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


def labels(n, n_lab):
    rng = np.random.default_rng(n_lab)
    M = (rng.random((n_lab, n, n)) < 0.5).astype(np.float64)
    M[-1] = np.eye(n)
    return M


def run(label, pb):
    eng = engine.engine_for(pb)
    t = pb.tree
    t_grad = best_of(lambda: eng.gradient(t.branch, pb.gene_rate))
    g_ms = engine.gradient_info()["last_kernel_ms"]
    t_curv = best_of(lambda: eng.curvature(t.branch, pb.gene_rate))
    c_ms = engine.curvature_info()["last_kernel_ms"]
    t_mg = best_of(lambda: eng.model_gradient(t.branch, pb.gene_rate))
    m_ms = engine.model_gradient_info()["last_kernel_ms"]
    print("%s: %d nodes, %d states, K %d, %d patterns, kernel %s\n  gradient %.3f ms (kernels %.3f ms); curvature %.3f ms (kernels %.3f ms); model_gradient %.3f ms (kernels %.3f ms)"
          % (label, t.n_nodes, pb.n, pb.K, pb.n_patt, eng.kernel_name, t_grad * 1e3, g_ms, t_curv * 1e3, c_ms, t_mg * 1e3, m_ms), flush=True)
    for n_lab in (2, 8):
        M = labels(pb.n, n_lab)
        for sites in (False, True):
            t_c = best_of(lambda: eng.subst_counts(t.branch, pb.gene_rate, labels=M, want_sites=sites))
            info = engine.subst_counts_info()
            est_ms = g_ms + n_lab * (c_ms - g_ms)
            print("  %d labels, %s: subst_counts %.3f ms (kernels %.3f ms, %d batches) -> %.2f gradient calls wall, %.2f by kernels; estimate %.2f by kernels"
                  % (n_lab, "with site_counts" if sites else "totals only    ", t_c * 1e3, info["last_kernel_ms"], info["last_batches"], t_c / t_grad,
                     info["last_kernel_ms"] / g_ms, est_ms / g_ms), flush=True)
    eng.close()


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
