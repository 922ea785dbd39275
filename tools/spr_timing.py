"""The scores of every SPR neighbour in one engine call (paml_amd_spr_scores) next to the only way there was before it, in the same
process: set_tree + eval per neighbour on one engine.  Per configuration: the call's wall time for the unlimited list and for the
radius-1 list (the fastest of three after a warm call) and its kernels by HIP events (paml_amd_spr_info); nni_scores on the same tree,
whose neighbours the radius-1 list's are; the per-neighbour way's FIRST pass (every topology new to the engine: tree programs and, on
the fast paths, per-tree kernels are acquired) and its SECOND pass over the same trees (kernels cached), separately; one evaluation of
the present tree for scale, at branch lengths it has not seen (an evaluation repeated at the same lengths finds its matrices and
partials in place and is printed beside it, not used).  The first pass walks every move where it costs a tenth of a millisecond
a tree (the small data set) and a sample of 20 moves spread over the list at 10^5 patterns, where it acquires a kernel per tree; the
second pass walks every move, after an unreported first pass over the trees the sample left out (--second-pass N: N moves spread
over the list instead, which the line then says).  Both passes are split into the time inside set_tree and inside eval.
Configurations: HIV M0 (13 taxa x
79 codon patterns), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns at 4 states with four classes.  Then the SPR search of the
brown golden from its two starting trees (pamlh_spr_search): wall time, moves, screening calls, neighbours maximised.
    python tools/spr_timing.py > profiles/spr_times.txt      (--only hiv|codon|nuc|search, repeatable: a part of it)"""
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


def run(label, pb, sample, second):
    eng = engine.engine_for(pb)
    t = pb.tree
    moves, near = t.spr_moves(), t.spr_moves(1)
    t_same = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    nudged = [t.branch * (1 + 1e-3 * k) for k in range(1, 6)]      # (new lengths at every call: nothing of the last evaluation can be reused)
    t_eval = best_of(lambda: eng.eval(nudged.pop(), pb.gene_rate))
    t_call = best_of(lambda: eng.spr_scores(t.branch, pb.gene_rate))
    info = engine.spr_info()
    t_near = best_of(lambda: eng.spr_scores(t.branch, pb.gene_rate, radius=1))
    info_near = engine.spr_info()
    t_nni = best_of(lambda: eng.nni_scores(t.branch, pb.gene_rate))
    got = eng.spr_scores(t.branch, pb.gene_rate)

    def spread(k):
        return np.arange(len(moves)) if k <= 0 or k >= len(moves) else np.unique(np.linspace(0, len(moves) - 1, k).astype(int))

    def walk(pick, what):      # set_tree + eval of every picked neighbour: seconds in set_tree, seconds in eval, the lnL
        trees, lnl, t_set, t_ev, t0 = [t.spr(*moves[i]) for i in pick], np.zeros(len(pick)), 0.0, 0.0, time.perf_counter()
        for i, q in enumerate(trees):
            t1 = time.perf_counter()
            eng.set_tree(q, pb.scale_node)
            t2 = time.perf_counter()
            lnl[i] = eng.eval(q.branch, pb.gene_rate)["lnL"]
            t_set, t_ev = t_set + t2 - t1, t_ev + time.perf_counter() - t2
            if i % 64 == 63:
                print("  ... %s: %s, %d of %d trees, %.1f s" % (label, what, i + 1, len(trees), time.perf_counter() - t0), file=sys.stderr, flush=True)
        return t_set, t_ev, lnl

    first, rest = spread(sample), spread(second)
    f_set, f_ev, _ = walk(first, "first pass")      # (topologies new to the engine)
    walk(np.setdiff1d(rest, first), "the other trees' first pass, not reported")
    s_set, s_ev, lnl = walk(rest, "second pass")      # (every tree seen before)
    dev = float(np.max(np.abs(lnl - got["lnL"][rest]) / np.abs(lnl)))
    per_first, per_second = (f_set + f_ev) / len(first), (s_set + s_ev) / len(rest)
    print("%-44s %2d tips, kernel %s: one eval at new branch lengths %.3f ms (repeated at the same lengths %.3f ms); "
          "spr_scores of all %d moves %.3f ms (kernels %.3f ms, %d batches) = %.1f evaluations; "
          "of the %d moves at radius 1 %.3f ms (kernels %.3f ms, %d batches), nni_scores of the %d swaps %.3f ms; "
          "set_tree + eval per neighbour: first pass over %d of the moves %.3f ms a tree (set_tree %.3f + eval %.3f), "
          "second pass over %d of the moves %.3f ms a tree (set_tree %.3f + eval %.3f) -> all moves %.1f ms / %.1f ms = %.1fx / %.1fx "
          "the call; largest relative difference of lnL %.1e"
          % (label, t.n_tips, eng.kernel_name, t_eval * 1e3, t_same * 1e3, len(moves), t_call * 1e3, info["last_kernel_ms"], info["last_batches"], t_call / t_eval,
             len(near), t_near * 1e3, info_near["last_kernel_ms"], info_near["last_batches"], len(t.nni_swaps()), t_nni * 1e3,
             len(first), per_first * 1e3, f_set / len(first) * 1e3, f_ev / len(first) * 1e3,
             len(rest), per_second * 1e3, s_set / len(rest) * 1e3, s_ev / len(rest) * 1e3,
             per_first * len(moves) * 1e3, per_second * len(moves) * 1e3, per_first * len(moves) / t_call, per_second * len(moves) / t_call, dev), flush=True)
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
            out = a.spr_search(a.default_x())
            print("SPR search, brown.nuc HKY85 from %-52s %.2f s, %d moves, %d screening calls, %d neighbours maximised, lnL %.4f (the NNI search's %.4f)"
                  % (r["start"], time.perf_counter() - t0, out["moves"], out["screening_calls"], out["optimisations"], out["lnL"], r["best_lnL"]), flush=True)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["hiv", "codon", "nuc", "search"], action="append", help="a part of the table (repeatable; default: all four)")
    ap.add_argument("--second-pass", type=int, default=0, help="trees of the per-neighbour second pass at 10^5 patterns (default 0: every move)")
    args = ap.parse_args()
    parts = args.only or ["hiv", "codon", "nuc", "search"]
    if "hiv" in parts:
        a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "hiv_ns0.ctl"), "codeml")
        run("HIV M0, 13 taxa x 79 codon patterns", a.problem(np.array(a.default_x())), 0, 0)
    if "codon" in parts:
        run("synth 16 taxa x 10^5 codon patterns", synth.codon_m0_problem(n_tips=16, n_patt=100_000), 20, args.second_pass)
    if "nuc" in parts:
        run("synth 32 taxa x 10^5 patterns, 4 states, K=4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000), 20, args.second_pass)
    if "search" in parts:
        search()
