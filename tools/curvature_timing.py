"""The curvature call (paml_amd_curvature: lnL, gradient and second derivative along every branch in one engine call) and the lock-step
Newton optimiser built on it, next to what they stand beside, in the same process:
    the engine call against paml_amd_gradient on the same engine — wall time of each (the fastest of three after a warm call) and the
    kernels by HIP events — and against one pass of paml_amd_eval_branch over every branch (one trial length each: half of the least a
    pamlh_minbranches sweep makes), at HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns at 4
    states with four classes;
    pamlh_newton_branches against pamlh_minbranches and against pamlh_optimize from the same start (the maximum with its branch block
    multiplied alternately by 1.6 and 0.5), to the same lnL: wall time (fastest of three), engine calls or evaluations, lnL — on the
    example data sets the host library loads (HIV M0; MHC M0 with its 381 branch lengths free, without pamlh_optimize; the mtCDNA
    branch model).
    python tools/curvature_timing.py > profiles/curvature_times.txt"""
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
    k_grad = engine.gradient_info()["last_kernel_ms"]
    t_curv = best_of(lambda: eng.curvature(t.branch, pb.gene_rate))
    info = engine.curvature_info()
    nodes = [v for v in range(t.n_nodes) if v != t.root]

    def walk():
        for v in nodes:
            eng.eval_branch(v, np.array([t.branch[v]]), t.branch, pb.gene_rate)
    t_walk = best_of(walk)
    print("%-44s %2d nodes, kernel %s: eval %.3f ms; gradient %.3f ms (kernels %.3f ms); curvature %.3f ms (kernels %.3f ms, %d batches) = %.2fx the gradient"
          " (kernels %.2fx); eval_branch once on each of %d branches %.3f ms = %.1fx the curvature call"
          % (label, t.n_nodes, eng.kernel_name, t_eval * 1e3, t_grad * 1e3, k_grad, t_curv * 1e3, info["last_kernel_ms"], info["last_batches"], t_curv / t_grad,
             info["last_kernel_ms"] / k_grad, len(nodes), t_walk * 1e3, t_walk / t_curv), flush=True)
    eng.close()


def search(label, ctl, prog, overrides=None, with_optimize=True):
    """with_optimize False (hundreds of branch lengths: BFGS by differences on all of x would run for minutes): the maximum is
    optimize_newton's and pamlh_optimize is left out of the comparison."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog, overrides=overrides)
    star = a.optimize(a.default_x()) if with_optimize else a.optimize_newton(a.default_x())
    nt = a.ntime
    lo, hi = a.bounds()
    start = star["x"].copy()
    start[:nt] = np.clip(start[:nt] * np.where(np.arange(nt) % 2 == 0, 1.6, 0.5), lo[:nt], hi[:nt])
    res = {}

    def timed(key, f):
        f()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            res[key] = f()
            ts.append(time.perf_counter() - t0)
        return min(ts)
    t_n = timed("n", lambda: a.newton_branches(start, e=1e-8))
    t_m = timed("m", lambda: a.minbranches(start, e=1e-8))
    t_o = timed("o", lambda: a.optimize(start)) if with_optimize else None
    print("%-38s %3d branches, lnL* %.6f, start %.6f" % (label, nt, star["lnL"], a.eval_gpu(start, want_lnf=False)[0]))
    print("    newton_branches      %8.2f ms, %4d engine calls (%d sweeps, %d rejected), lnL %.6f" % (t_n * 1e3, res["n"]["calls"], res["n"]["sweeps"], res["n"]["rejected"], res["n"]["lnL"]))
    print("    minbranches          %8.2f ms, %4d eval_branch calls, lnL %.6f" % (t_m * 1e3, res["m"]["branch_calls"], res["m"]["lnL"]))
    # the two boxes differ: pamlh_bounds (newton_branches, optimize) holds a branch at 4e-6 or more, minbranches at 1e-8 or more
    c = a.curvature(res["n"]["x"])
    at = res["n"]["x"][:nt] <= lo[:nt] * 1.0001
    print("    newton_branches leaves %d branches at the box's lower bound %g (minbranches goes down to 1e-8: %d below %g); to first order"
          " that is worth sum g (1e-8 - %g) = %.6f in lnL" % (at.sum(), lo[0], int((res["m"]["x"][:nt] < lo[:nt]).sum()), lo[0], lo[0],
                                                            float(np.sum(c["grad"][at] * (1e-8 - lo[:nt][at])))))
    if with_optimize:
        print("    optimize (all of x)  %8.2f ms, %4d evaluations, lnL %.6f" % (t_o * 1e3, res["o"]["n_eval"], res["o"]["lnL"]))
    sys.stdout.flush()


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    search("HIV M0", "hiv_ns0.ctl", "codeml")
    search("MHC M0, 192 taxa, free branch lengths", "mhc_m0.ctl", "codeml", overrides="fix_blength = 0", with_optimize=False)
    search("mtCDNA branch model", "mtcdna_branch.ctl", "codeml")
