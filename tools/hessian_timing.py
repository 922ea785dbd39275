"""The Hessian call (paml_amd_hessian: lnL, gradient and every second derivative over the branch lengths in one engine call) and what the
host builds on it, next to what they stand beside, in the same process:
    the engine call against 2 n_b paml_amd_gradient calls — the central-difference route to the same matrix; one gradient call is timed
    and multiplied — wall time of each (the fastest of three after a warm call) and the kernels by HIP events, at HIV M0 (13 taxa x 79
    codon patterns), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns at 4 states with four classes;
    pamlh_standard_errors_exact against pamlh_standard_errors method 1 on HIV M0, and by itself on MHC M0 with its branch lengths free
    (383 parameters: method 1's stencil there is 2 x 383^2 + 1 = 293 379 evaluations in one batch and is not attempted);
    pamlh_newton_full against pamlh_newton_branches from the same start (the maximum with its branch block multiplied alternately by
    1.6 and 0.5), e = 1e-8: sweeps, engine calls, wall time (fastest of three), lnL — HIV M0, MHC M0 with free branch lengths, the mtCDNA
    branch model.
    python tools/hessian_timing.py > profiles/hessian_times.txt"""
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
    nb = t.n_nodes - 1
    t_grad = best_of(lambda: eng.gradient(t.branch, pb.gene_rate))
    k_grad = engine.gradient_info()["last_kernel_ms"]
    t_curv = best_of(lambda: eng.curvature(t.branch, pb.gene_rate))
    t_hess = best_of(lambda: eng.hessian(t.branch, pb.gene_rate))
    info = engine.hessian_info()
    print("%-44s %2d branches, %d pairs, kernel %s: gradient %.3f ms (kernels %.3f ms); curvature %.3f ms; hessian %.3f ms (kernels %.3f ms, %d batches)"
          " = %.1fx a gradient; 2 n_b = %d gradient calls %.1f ms = %.2fx the hessian call"
          % (label, nb, nb * (nb - 1) // 2, eng.kernel_name, t_grad * 1e3, k_grad, t_curv * 1e3, t_hess * 1e3, info["last_kernel_ms"], info["last_batches"],
             t_hess / t_grad, 2 * nb, 2 * nb * t_grad * 1e3, 2 * nb * t_grad / t_hess), flush=True)
    eng.close()


def timed(f):
    f()
    ts, r = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), r


def errors(label, ctl, prog, overrides=None, method1=True):
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog, overrides=overrides)
    x = (a.optimize(a.default_x()) if method1 else a.optimize_newton(a.default_x()))["x"]
    t_e, r = timed(lambda: a.standard_errors_exact(x))
    line = "%-38s %3d parameters (%d branch lengths): standard_errors_exact %9.2f ms, %d left out at a bound" % (label, a.np, a.ntime, t_e * 1e3, int((r["se"] == -1).sum()))
    if method1:
        t_1, (se1, _) = timed(lambda: a.standard_errors(x, method=1))
        live = se1 != -1
        line += "; method 1 (%d evaluations in one batch) %9.2f ms = %.2fx; largest relative difference of the two se %.2e" % (
            2 * int(live.sum()) ** 2 + 1, t_1 * 1e3, t_1 / t_e, float(np.max(np.abs(r["se"][live] - se1[live]) / se1[live])))
    else:
        line += "; method 1 not attempted (%d evaluations in one batch)" % (2 * a.np ** 2 + 1)
    print(line, flush=True)


def search(label, ctl, prog, overrides=None, with_optimize=True):
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog, overrides=overrides)
    star = a.optimize(a.default_x()) if with_optimize else a.optimize_newton(a.default_x())
    nt = a.ntime
    lo, hi = a.bounds()
    start = star["x"].copy()
    start[:nt] = np.clip(start[:nt] * np.where(np.arange(nt) % 2 == 0, 1.6, 0.5), lo[:nt], hi[:nt])
    t_b, rb = timed(lambda: a.newton_branches(start, e=1e-8))
    t_f, rf = timed(lambda: a.newton_full(start, e=1e-8))
    print("%-38s %3d branches, lnL* %.6f, start %.6f" % (label, nt, star["lnL"], a.eval_gpu(start, want_lnf=False)[0]))
    print("    newton_branches      %9.2f ms, %4d engine calls (%d sweeps, %d rejected), lnL %.8f" % (t_b * 1e3, rb["calls"], rb["sweeps"], rb["rejected"], rb["lnL"]))
    print("    newton_full          %9.2f ms, %4d engine calls (%d sweeps, %d rejected), lnL %.8f" % (t_f * 1e3, rf["calls"], rf["sweeps"], rf["rejected"], rf["lnL"]))
    sys.stdout.flush()


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    errors("HIV M0", "hiv_ns0.ctl", "codeml")
    search("HIV M0", "hiv_ns0.ctl", "codeml")
    search("mtCDNA branch model", "mtcdna_branch.ctl", "codeml")
    search("MHC M0, 192 taxa, free branch lengths", "mhc_m0.ctl", "codeml", overrides="fix_blength = 0", with_optimize=False)
    errors("MHC M0, 192 taxa, free branch lengths", "mhc_m0.ctl", "codeml", overrides="fix_blength = 0", method1=False)
