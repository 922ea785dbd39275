"""The scores of every configuration of every edge at trial lengths, with two derivatives, in one engine call (paml_amd_edge_scores)
next to one nni_scores call and one evaluation on the same engine, per configuration: the call's wall time (the fastest of three after
a warm call) and its kernels by HIP events (paml_amd_edge_info).  Rows: every edge of edge_list x its three configurations, all five
branches overridden at the tree's own lengths, u = v.  Configurations: HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon
patterns, 32 taxa x 10^5 patterns at 4 states with four classes.  Then the whole branch_supports of the C host on HIV M0 at the
estimates (engine calls, sweeps, wall time) against apply_nni + pamlh_optimize on a sample of two neighbours; the figure for all
2 (ns - 3) neighbours is an extrapolation from that sample and is printed as one.
    python tools/edge_timing.py > profiles/edge_times.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, hostlib, synth      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


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
    edges, five = t.edge_configs()
    rows = np.array([[cfg[0], cfg[1], cfg[2], cfg[0]] for e in range(len(edges)) for cfg in edges[e]], dtype=np.int32)
    on = np.repeat(five, 3, axis=0)
    ot = t.branch[on]
    plain = rows.copy()
    plain[:, 3] = -1
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    t_nni = best_of(lambda: eng.nni_scores(t.branch, pb.gene_rate))
    k_nni = engine.nni_info()["last_kernel_ms"]
    t_plain = best_of(lambda: eng.edge_scores(t.branch, pb.gene_rate, plain, on, ot))
    k_plain = engine.edge_info()["last_kernel_ms"]
    t_call = best_of(lambda: eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot))
    info = engine.edge_info()
    got = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot)
    nni = eng.nni_scores(t.branch, pb.gene_rate, swaps=np.ascontiguousarray(rows[rows[:, 1] >= 0][:, :3]))
    dev = float(np.max(np.abs(got["lnL"][rows[:, 1] >= 0] - nni["lnL"]) / np.abs(nni["lnL"])))
    print("%-44s %2d tips, %3d edges, %3d rows, kernel %s: one eval %.3f ms; nni_scores (%d swaps) %.3f ms (kernels %.3f ms); edge_scores with u = v %.3f ms "
          "(kernels %.3f ms, %d batches) = %.1f evaluations = %.2f nni_scores calls; with u = -1 %.3f ms (kernels %.3f ms); largest relative difference of "
          "the swap rows' lnL to nni_scores %.1e" % (label, t.n_tips, len(edges), len(rows), eng.kernel_name, t_eval * 1e3, len(t.nni_swaps()), t_nni * 1e3, k_nni,
                                                     t_call * 1e3, info["last_kernel_ms"], info["last_batches"], t_call / t_eval, t_call / t_nni, t_plain * 1e3, k_plain, dev), flush=True)
    eng.close()


def supports():
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "hiv_ns0.ctl"), "codeml")
    t0 = time.perf_counter()
    opt = a.optimize(a.default_x())
    t_opt = time.perf_counter() - t0
    x = np.array(opt["x"])
    a.branch_supports(x, n_rep=1000, seed=1)      # (warm)
    t0 = time.perf_counter()
    eo = a.edge_optimize(x)
    t_eo = time.perf_counter() - t0
    t0 = time.perf_counter()
    sup = a.branch_supports(x, n_rep=1000, seed=1)
    t_sup = time.perf_counter() - t0
    swaps = a.nni_scores(x)["swaps"]
    sample, t_nb, gains = [0, len(swaps) // 2], [], []
    for i in sample:
        v, s, xx = (int(c) for c in swaps[i])
        a.apply_nni(v, s, xx)
        t0 = time.perf_counter()
        o = a.optimize(x)
        t_nb.append(time.perf_counter() - t0)
        a.apply_nni(v, xx, s)
        e = list(sup["edge_node"]).index(v)
        cfg = [tuple(int(c) for c in c3) for c3 in eo["edges"][e]].index((v, s, xx)) if (v, s, xx) in [tuple(int(c) for c in c3) for c3 in eo["edges"][e]] else None
        gains.append((o["lnL"], None if cfg is None else eo["lnL"][e][cfg]))
    per = float(np.mean(t_nb))
    print("HIV M0 at the estimates (pamlh_optimize of the tree itself: %.2f s, lnL %.4f): branch_supports of %d edges with 1000 replicates %.3f s, of which "
          "edge_optimize %.3f s (%d sweeps, %d engine calls, %d rows at a bound); supports %s"
          % (t_opt, opt["lnL"], len(sup["edge_node"]), t_sup, t_eo, eo["sweeps"], eo["calls"], eo["rows_at_bound"], np.array2string(sup["support"], precision=3)), flush=True)
    print("apply_nni + pamlh_optimize per neighbour, a sample of %d of the %d neighbours: %s s each (fully maximised lnL, five-branch lnL of the same "
          "configuration: %s); EXTRAPOLATED to all %d neighbours: %.1f s = %.0fx the whole branch_supports"
          % (len(sample), len(swaps), ", ".join("%.2f" % v for v in t_nb), "; ".join("%.4f, %s" % (g[0], "-" if g[1] is None else "%.4f" % g[1]) for g in gains),
             len(swaps), per * len(swaps), per * len(swaps) / t_sup), flush=True)


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    supports()
