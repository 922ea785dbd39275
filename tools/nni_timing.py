"""The scores of every NNI neighbour in one engine call (paml_amd_nni_scores) next to the only way there was before it, in the same
process: set_tree + eval per neighbour on one engine.  Per configuration: the call's wall time (the fastest of three after a warm call)
and its kernels by HIP events (paml_amd_nni_info); the per-neighbour way's FIRST pass over the neighbours (every topology new to the
engine: tree programs and, on the fast paths, per-tree kernels are acquired) and its SECOND pass over the same trees (kernels cached),
separately; one evaluation of the present tree for scale.  Configurations: HIV M0 (13 taxa x 79 codon patterns), 16 taxa x 10^5 codon
patterns, 32 taxa x 10^5 patterns at 4 states with four classes.  Then the NNI search of the brown golden from its two starting trees
(pamlh_nni_search): wall time, moves, screening calls, neighbours maximised.
    python tools/nni_timing.py > profiles/nni_times.txt"""
import json
import os
import sys
import tempfile
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
    swaps = t.nni_swaps()
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    t_call = best_of(lambda: eng.nni_scores(t.branch, pb.gene_rate))
    info = engine.nni_info()
    got = eng.nni_scores(t.branch, pb.gene_rate)
    trees = [t.nni(*sw) for sw in swaps]
    passes, lnl = [], np.zeros(len(swaps))
    for _ in range(2):
        t0 = time.perf_counter()
        for i, q in enumerate(trees):
            eng.set_tree(q, pb.scale_node)
            lnl[i] = eng.eval(t.branch, pb.gene_rate)["lnL"]
            if i % 8 == 7:
                print("  ... %s: pass %d, %d of %d trees, %.1f s" % (label, len(passes) + 1, i + 1, len(trees), time.perf_counter() - t0), file=sys.stderr, flush=True)
        passes.append(time.perf_counter() - t0)
    dev = float(np.max(np.abs(lnl - got["lnL"]) / np.abs(lnl)))
    print("%-44s %2d tips, %3d swaps, kernel %s: one eval %.3f ms; nni_scores %.3f ms (kernels %.3f ms, %d batches) = %.1f evaluations; "
          "set_tree + eval per neighbour: first pass %.1f ms, second pass %.1f ms -> %.1fx / %.1fx the call; largest relative difference of lnL %.1e"
          % (label, t.n_tips, len(swaps), eng.kernel_name, t_eval * 1e3, t_call * 1e3, info["last_kernel_ms"], info["last_batches"], t_call / t_eval,
             passes[0] * 1e3, passes[1] * 1e3, passes[0] / t_call, passes[1] / t_call, dev), flush=True)
    eng.close()


def search():
    g = json.load(open(os.path.join(GOLDEN, "brown_nni_search.json")))
    with tempfile.TemporaryDirectory() as d:
        for r in g["runs"]:
            with open(os.path.join(d, "start.trees"), "w") as f:
                f.write("%d 1\n%s\n" % (len(g["names"]), r["start"]))
            with open(os.path.join(d, "start.ctl"), "w") as f:
                f.write("seqfile = %s\ntreefile = start.trees\nmodel = 4\nfix_kappa = 0\nkappa = 5\nfix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\n"
                        % os.path.join(GOLDEN, "data", "brown.nuc"))
            a = hostlib.Analysis(os.path.join(d, "start.ctl"), "baseml")
            t0 = time.perf_counter()
            out = a.nni_search(a.default_x())
            print("NNI search, brown.nuc HKY85 from %-52s %.2f s, %d moves, %d screening calls, %d neighbours maximised, lnL %.4f (reference %.4f)"
                  % (r["start"], time.perf_counter() - t0, out["moves"], out["screening_calls"], out["optimisations"], out["lnL"], r["best_lnL"]), flush=True)


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "hiv_ns0.ctl"), "codeml")
    run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())))
    run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000))
    search()
