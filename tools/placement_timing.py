"""Every query on every branch at every pendant length in one engine call (paml_amd_placement_scores) next to the only way there was
before it, in the same process: an engine with n_tips + 1 tips, set_tips per query, set_tree per branch and eval per pendant length.
Per configuration: the call's wall time (the fastest of three synchronous calls after a warm call) and its kernels by HIP events
(paml_amd_placement_info); the per-placement way's FIRST pass over the (query, branch, pendant) triples (every topology new to the
engine: tree programs and, on the fast paths, per-tree kernels are acquired) and its SECOND pass over the same triples (kernels cached),
separately; one evaluation of the present tree for scale.  Four queries and three pendant lengths each.  Configurations: HIV M0 with one
sequence taken out of the tree (12 taxa x 79 codon patterns; the queries are that sequence and three copies of it with a tenth of the
codons redrawn), 16 taxa x 10^5 codon patterns, 32 taxa x 10^5 patterns at 4 states with four classes (queries: copies of tips with a
tenth of the characters redrawn).
    python tools/placement_timing.py > profiles/placement_times.txt"""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, hostlib, synth      # noqa: E402
from paml_amd.problem import Tree, set_node_scale      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PENDANT, PHI = (0.05, 0.1, 0.2), 0.5


def best_of(f, n=3):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def without_tip(pb, k):
    """(pb on the tree without tip k — its father, left with one son, is taken out and the two branches are joined —, tip k's row)."""
    t = pb.tree
    f = int(t.father()[k])
    assert f != t.root and len(t.sons[f]) == 2, "take a tip whose father is a binary node below the root"
    c = [s for s in t.sons[f] if s != k][0]
    gone = {k, f}
    new = {old: i for i, old in enumerate(v for v in range(t.n_nodes) if v not in gone)}
    sons = [[] for _ in range(t.n_nodes - 2)]
    branch, label = np.zeros(t.n_nodes - 2), np.zeros(t.n_nodes - 2, dtype=np.int32)
    for v in range(t.n_nodes):
        if v in gone:
            continue
        sons[new[v]] = [new[c if s == f else s] for s in t.sons[v]]
        branch[new[v]], label[new[v]] = t.branch[v] + (t.branch[f] if v == c else 0.0), t.label[v]
    q = copy.copy(pb)
    q.tree = Tree(t.n_tips - 1, t.n_nodes - 2, new[t.root], sons, branch, label)
    q.z = np.ascontiguousarray(np.delete(pb.z, k, axis=0))
    if pb.scale_node is not None:
        q.scale_node = set_node_scale(q.tree, 15 if pb.n == 61 else 100)
    return q, pb.z[k].copy()


def queries_from(rows, n, rng):
    out = []
    for r in rows:
        r = r.copy()
        redraw = rng.random(len(r)) < 0.1
        r[redraw] = rng.integers(0, n, size=int(redraw.sum()))
        out.append(r)
    return out


def enlarged(pb, v, tau, qrow):
    q = copy.copy(pb)
    q.tree = pb.tree.insert_tip(int(v), PHI, tau)
    q.z = np.ascontiguousarray(np.vstack([pb.z, qrow[None, :]]), dtype=np.uint8)
    if pb.scale_node is not None:
        q.scale_node = set_node_scale(q.tree, 15 if pb.n == 61 else 100)
    return q


def run(label, pb, queries):
    queries = np.ascontiguousarray(np.stack(queries), dtype=np.uint8)
    eng = engine.engine_for(pb)
    t = pb.tree
    edges = [v for v in range(t.n_nodes) if v != t.root]
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    call = lambda: eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI)      # noqa: E731
    t_call = best_of(call)
    info = engine.placement_info()
    got = call()
    name = eng.kernel_name
    eng.close()
    big = engine.engine_for(enlarged(pb, edges[0], PENDANT[0], queries[0]))
    trees = [[pb.tree.insert_tip(v, PHI, tau) for tau in PENDANT] for v in edges]
    scale = [None if pb.scale_node is None else set_node_scale(tr[0], 15 if pb.n == 61 else 100) for tr in trees]
    passes, lnl = [], np.zeros(got["lnL"].shape)
    for _ in range(2):
        t0 = time.perf_counter()
        for qi in range(len(queries)):
            z = np.ascontiguousarray(np.vstack([pb.z, queries[qi][None, :]]), dtype=np.uint8)
            big.set_tips(z, pb.weights, pb.cleandata, pb.n_chara, pb.chara_map, pb.gene_off)
            for i in range(len(edges)):
                big.set_tree(trees[i][0], scale[i])
                for j in range(len(PENDANT)):
                    lnl[qi, i, j] = big.eval(trees[i][j].branch, pb.gene_rate)["lnL"]
            print("  ... %s: pass %d, query %d of %d, %.1f s" % (label, len(passes) + 1, qi + 1, len(queries), time.perf_counter() - t0), file=sys.stderr, flush=True)
        passes.append(time.perf_counter() - t0)
    dev = float(np.max(np.abs(lnl - got["lnL"]) / np.abs(lnl)))
    print("%-44s %2d tips, %d queries x %3d branches x %d pendants = %4d placements, kernel %s: one eval %.3f ms; placement_scores %.3f ms (kernels %.3f ms, "
          "%d batches) = %.1f evaluations; set_tips / set_tree / eval per placement on an engine of %d tips: first pass %.1f ms, second pass %.1f ms -> "
          "%.1fx / %.1fx the call; largest relative difference of lnL %.1e"
          % (label, t.n_tips, len(queries), len(edges), len(PENDANT), lnl.size, name, t_eval * 1e3, t_call * 1e3, info["last_kernel_ms"], info["last_batches"],
             t_call / t_eval, t.n_tips + 1, passes[0] * 1e3, passes[1] * 1e3, passes[0] / t_call, passes[1] / t_call, dev), flush=True)
    big.close()


if __name__ == "__main__":
    rng = np.random.default_rng(20261019)
    a = hostlib.Analysis(os.path.join(GOLDEN, "ctl", "hiv_ns0.ctl"), "codeml")
    full = a.problem(np.array(a.default_x()))
    f = full.tree.father()
    k = next(i for i in range(full.tree.n_tips) if f[i] != full.tree.root and len(full.tree.sons[f[i]]) == 2)
    hiv, row = without_tip(full, k)
    run("HIV M0 without sequence %d, 12 taxa x 79 codon patterns" % (k + 1), hiv, [row] + queries_from([row] * 3, hiv.n, rng))
    pb = synth.codon_m0_problem(n_tips=16, n_patt=100_000)
    run("synth 16 taxa x 10^5 codon patterns", pb, queries_from(list(pb.z[:4]), pb.n, rng))
    pb = synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=100_000)
    run("synth 32 taxa x 10^5 patterns, 4 states, K=4", pb, queries_from(list(pb.z[:4]), pb.n, rng))
