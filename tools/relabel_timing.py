"""The lnL of the tree with one branch relabelled, for every (branch, label) row in one engine call (paml_amd_relabel_scores), next to the
only way there was before it, in the same process: set_tree(relabelled) + eval per row on one engine.  Per configuration: the call's wall
time without and with the per-class values (the fastest of three after a warm call), its kernels by HIP events (paml_amd_relabel_info),
the per-row way over (at most 90 of) the same rows, one evaluation and one gradient call for scale.  Configurations: the lysozyme
foreground scan's model (19 taxa x 86 codon patterns, K = 2, 33 branches x 9 values of w2), 16 taxa x 10^5 codon patterns with the same
class table, 32 taxa x 10^5 patterns at 4 states with four classes and three labels.  Then pamlh_foreground_scan on the lysozyme data as
a whole, and set_foreground + pamlh_optimize of three branches for the cost of the search the scan stands in for.
    python tools/relabel_timing.py > profiles/relabel_times.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, hostlib, models, synth      # noqa: E402
from paml_amd.problem import EIGEN_UVROOT, MODE_LFUNDG      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GRID = hostlib.DEFAULT_OMEGA2_GRID


def best_of(f, n=3):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def scan_model(pb, kappa, w0):
    """pb with the foreground scan's class table: K = 2 (w0 and 1), label 0 the background, label 1 + g both classes at GRID[g]."""
    import copy
    q = copy.copy(pb)
    pi = pb.pi[0]
    q.eigen = []
    for w in (w0, 1.0) + tuple(GRID):
        U, V, root, _ = models.codon_m0_eigen(kappa, w, pi, scale=1.0)
        q.eigen.append(dict(kind=EIGEN_UVROOT, U=U, V=V, Root=root))
    q.mode, q.freqK, q.rate = MODE_LFUNDG, np.array([0.6, 0.4]), np.ones(2)
    q.eigen_of = np.array([[[k] + [2 + g for g in range(len(GRID))] for k in range(2)]], dtype=np.int32)
    q.qfactor = np.ones((2, 1 + len(GRID)))
    t = pb.tree
    q.tree = type(t)(t.n_tips, t.n_nodes, t.root, t.sons, t.branch, np.zeros(t.n_nodes, dtype=np.int32), t.names)
    return q


def run(label, pb, rows):
    eng = engine.engine_for(pb)
    t = pb.tree
    count = [0]

    def eval_at_new_lengths():      # (an evaluation at the lengths of the one before it is answered from what the engine kept)
        count[0] += 1
        b = np.array(t.branch)
        b[0 if t.root != 0 else 1] += 1e-9 * count[0]
        eng.eval(b, pb.gene_rate)
    t_eval = best_of(eval_at_new_lengths)
    t_grad = best_of(lambda: eng.gradient(t.branch, pb.gene_rate))
    t_call = best_of(lambda: eng.relabel_scores(t.branch, pb.gene_rate, rows=rows))
    info = engine.relabel_info()
    t_cls = best_of(lambda: eng.relabel_scores(t.branch, pb.gene_rate, rows=rows, want_classes=True))
    info_cls = engine.relabel_info()
    got = eng.relabel_scores(t.branch, pb.gene_rate, rows=rows)
    pick = np.linspace(0, len(rows) - 1, min(90, len(rows))).astype(int)
    lnl = np.zeros(len(pick))
    t0 = time.perf_counter()
    for j, i in enumerate(pick):
        eng.set_tree(t.relabelled(int(rows[i][0]), int(rows[i][1])), pb.scale_node)
        lnl[j] = eng.eval(t.branch, pb.gene_rate)["lnL"]
    per_row = (time.perf_counter() - t0) / len(pick)
    dev = float(np.max(np.abs(lnl - got["lnL"][pick]) / np.abs(lnl)))
    print("%-50s %2d tips, %3d rows, kernel %s: one eval %.3f ms, one gradient %.3f ms; relabel_scores %.3f ms (kernels %.3f ms, %d batches) = %.1f evaluations "
          "= %.1f gradients; with the class values %.3f ms (kernels %.3f ms); set_tree + eval per row %.3f ms, all rows %.1f ms -> %.1fx the call "
          "(%.1fx with the class values); largest relative difference of lnL %.1e"
          % (label, t.n_tips, len(rows), eng.kernel_name, t_eval * 1e3, t_grad * 1e3, t_call * 1e3, info["last_kernel_ms"], info["last_batches"], t_call / t_eval,
             t_call / t_grad, t_cls * 1e3, info_cls["last_kernel_ms"], per_row * 1e3, per_row * len(rows) * 1e3, per_row * len(rows) / t_call,
             per_row * len(rows) / t_cls, dev), flush=True)
    eng.close()


def all_rows(tree, labels):
    return np.asarray([(v, l) for v in range(tree.n_nodes) if v != tree.root for l in labels], dtype=np.int32)


def host_scan():
    import json
    g = json.load(open(os.path.join(GOLDEN, "lyso_bsa.json")))
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "lyso_bsa.ctl"), "codeml")
    x = np.array(g["x"])
    a.eval_gpu(x)
    t_scan = best_of(lambda: a.foreground_scan(x))
    info = engine.relabel_info()
    sc = a.foreground_scan(x)
    print("pamlh_foreground_scan, lysozyme, %d branches x %d values of w2: %.1f ms as a whole; the engine call's kernels %.3f ms (%d batches); the rest is the "
          "model set-up, the copies of the class values and %d mixture maximisations on the host" % (len(sc["node"]), len(GRID), t_scan * 1e3, info["last_kernel_ms"],
                                                                                                       info["last_batches"], sc["lnL"].size), flush=True)
    lo, hi = a.bounds()
    order = np.argsort(-sc["delta"])[:3]
    t0 = time.perf_counter()
    for b in order:
        gi = int(sc["best"][b])
        xa = a.foreground_point(x, int(sc["node"][b]), GRID[gi], sc["p0"][b][gi], sc["p1"][b][gi])
        a.set_foreground(int(sc["node"][b]))
        r = a.optimize(np.clip(xa, lo, hi))
        print("  foreground node %2d: the scan's row %.6f (delta %.4f), maximised %.6f in %d evaluations" % (sc["node"][b], sc["lnL"][b][gi], sc["delta"][b], r["lnL"], r["n_eval"]), flush=True)
    per = (time.perf_counter() - t0) / len(order)
    print("set_foreground + pamlh_optimize: %.2f s per branch over the three branches of largest delta; every one of the %d branches that way would take about %.0f s, "
          "%.0fx the scan (the search also maximises the lengths, kappa and w0 again, which the scan does not)" % (per, len(sc["node"]), per * len(sc["node"]), per * len(sc["node"]) / t_scan), flush=True)


if __name__ == "__main__":
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "lyso_bsa.ctl"), "codeml")
    pb = scan_model(a.problem(np.array(a.default_x())), 2.0, 0.1)
    labels = range(1, 1 + len(GRID))
    run("lysozyme, 19 taxa x 86 codon patterns, K=2", pb, all_rows(pb.tree, labels))
    pb = scan_model(synth.codon_m0_problem(n_tips=16, n_patt=100_000), 2.0, 0.1)
    run("synth 16 taxa x 10^5 codon patterns, K=2", pb, all_rows(pb.tree, labels))
    pb = synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000)
    pb.eigen = pb.eigen + [synth.nuc_gtr_gamma_problem(n_tips=4, n_patt=500, seed=s).eigen[0] for s in (5, 6)]
    pb.eigen_of = np.array([[[0, 1, 2]] * 4], dtype=np.int32)
    pb.qfactor = np.ones((4, 3))
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", pb, all_rows(pb.tree, range(3)))
    host_scan()
