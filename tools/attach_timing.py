"""Attachment rows at free lengths with derivatives in one engine call (paml_amd_attach_scores), and the maximum-likelihood placement
iterated on it, next to what there was before, in the same process.  Per configuration of tools/placement_timing.py, with 4 queries:
  * one placement_scores call (every branch, three pendants) for scale, which also picks each query's 5 best branches;
  * one attach_scores call of 4 queries x 5 branches x 3 roles = 60 rows: wall time (the fastest of three synchronous calls after a warm
    call) and its kernels by HIP events (paml_amd_attach_info);
  * the whole maximum-likelihood placement of the 20 (query, branch) rows in lock step: the iteration of pamlh_place_optimize restated
    here on Engine.attach_scores (the same step, trials, tolerance and bounds), every call counted;
  * the per-placement way: an engine with n_tips + 1 tips, set_tips per query, set_tree per branch, then the same safeguarded Newton
    iteration on the three branches at the new node through eval_branch (one call per trial); FIRST pass (every topology new to the
    engine) and SECOND pass (kernels cached) separately.
    python tools/attach_timing.py > profiles/attach_times.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paml_amd import engine, hostlib, synth      # noqa: E402
from paml_amd.problem import set_node_scale      # noqa: E402
from placement_timing import GOLDEN, PENDANT, PHI, best_of, enlarged, queries_from, without_tip      # noqa: E402

KEEP, TRIALS, MAX_SWEEPS, LO, HI = 5, 4, 30, 4e-6, 50.0


def newton_trial(trial, ln, d1, d2, l, ti, tn, step):
    """pamlh_newton_trial for one row: (goes on, l, ti, tn, step)."""
    if trial == 0 or ln >= l:
        ti = tn
        if trial:
            l = ln
        s = -d1 / d2 if d2 < 0 else (ti if d1 > 0 else -0.5 * ti if d1 < 0 else 0.0)
    else:
        s = 0.5 * step
    target = min(max(ti + s, LO), HI)
    s = target - ti
    if trial == TRIALS or abs(s) < 1e-10:
        return False, l, ti, ti, s
    return True, l, ti, target, s


def ascent(score, t, n):
    """The lock-step iteration of pamlh_place_optimize over n rows: score(role[n], lengths[n][3]) -> (lnL, d1, d2); returns (t, l, calls)."""
    t = np.clip(np.array(t, dtype=np.float64), LO, HI)
    calls = 1
    l = score(np.full(n, -1), t)[0].copy()
    done = np.zeros(n, dtype=bool)
    for _ in range(MAX_SWEEPS):
        l_sweep = l.copy()
        for role in range(3):
            roles = np.where(done, -1, role)
            wait, step, tt = done.copy(), np.zeros(n), t.copy()
            for trial in range(TRIALS + 1):
                ln, d1, d2 = score(roles, tt)
                calls += 1
                for i in np.flatnonzero(~wait):
                    go, l[i], t[i, role], tt[i, role], step[i] = newton_trial(trial, ln[i], d1[i], d2[i], l[i], t[i, role], tt[i, role], step[i])
                    if not go:
                        wait[i], roles[i] = True, -1
                if wait.all():
                    break
        done |= l - l_sweep <= 1e-6
        if done.all():
            break
    return t, l, calls


def run(label, pb, queries):
    queries = np.ascontiguousarray(np.stack(queries), dtype=np.uint8)
    eng = engine.engine_for(pb)
    t = pb.tree
    edges = [v for v in range(t.n_nodes) if v != t.root]
    t_eval = best_of(lambda: eng.eval(t.branch, pb.gene_rate))
    grid_call = lambda: eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI)      # noqa: E731
    t_grid = best_of(grid_call)
    grid = grid_call()
    le = grid["lnL"].max(axis=2)
    pairs = [(q, int(e)) for q in range(len(queries)) for e in np.argsort(-le[q], kind="stable")[:KEEP]]
    start = np.array([[(1 - PHI) * t.branch[edges[e]], PHI * t.branch[edges[e]], PENDANT[int(np.argmax(grid["lnL"][q, e]))]] for q, e in pairs])
    rows3 = np.array([[q, edges[e], role] for q, e in pairs for role in range(3)], dtype=np.int32)
    one = lambda: eng.attach_scores(t.branch, pb.gene_rate, queries, rows3, np.repeat(start, 3, axis=0))      # noqa: E731
    t_one = best_of(one)
    info = engine.attach_info()

    def score(roles, lengths):
        rw = np.array([[q, edges[e], r] for (q, e), r in zip(pairs, roles)], dtype=np.int32)
        got = eng.attach_scores(t.branch, pb.gene_rate, queries, rw, lengths)
        return got["lnL"], got["d1"], got["d2"]
    ascent(score, start, len(pairs))      # (warm)
    t0 = time.perf_counter()
    t3, l, calls = ascent(score, start, len(pairs))
    t_ml = time.perf_counter() - t0
    name = eng.kernel_name
    eng.close()

    # the per-placement way: one enlarged tree after the other, its three branches by the same iteration on eval_branch
    big = engine.engine_for(enlarged(pb, edges[0], PENDANT[0], queries[0]))
    nt = t.n_tips
    passes, l_big, n_calls = [], np.zeros(len(pairs)), 0
    for _ in range(2):
        t0 = time.perf_counter()
        n_calls, last_q = 0, -1
        for i, (q, e) in enumerate(pairs):
            if q != last_q:
                big.set_tips(np.ascontiguousarray(np.vstack([pb.z, queries[q][None, :]]), dtype=np.uint8), pb.weights, pb.cleandata, pb.n_chara, pb.chara_map, pb.gene_off)
                last_q = q
            v = edges[e]
            tree = t.insert_tip(v, PHI, start[i][2])
            big.set_tree(tree, None if pb.scale_node is None else set_node_scale(tree, 15 if pb.n == 61 else 100))
            nodes = (tree.n_nodes - 1, v if v < nt else v + 1, nt)
            branch = np.array(tree.branch, dtype=np.float64)

            def score1(roles, lengths):
                for j in range(3):
                    branch[nodes[j]] = lengths[0][j]
                role = int(roles[0])
                a, b, c = big.eval_branch(nodes[max(role, 0)], np.array([lengths[0][max(role, 0)]]), branch, pb.gene_rate)
                return a, (b if role >= 0 else np.zeros(1)), (c if role >= 0 else np.zeros(1))
            _, li, c = ascent(score1, start[i:i + 1], 1)
            l_big[i], n_calls = li[0], n_calls + c
        passes.append(time.perf_counter() - t0)
        print("  ... %s: pass %d, %.1f s" % (label, len(passes), passes[-1]), file=sys.stderr, flush=True)
    dev = float(np.max(np.abs(l_big - l)))
    print("%-44s %2d tips, kernel %s: one eval %.3f ms; placement_scores (%d x %d x %d) %.3f ms; attach_scores of %d rows %.3f ms (kernels %.3f ms, %d batches) = "
          "%.2f placement_scores calls; ML placement of %d (query, branch) rows in lock step: %d attach_scores calls, %.1f ms; per placement on an engine of %d "
          "tips (set_tips / set_tree / %d eval_branch calls): first pass %.1f ms, second pass %.1f ms -> %.1fx / %.1fx the lock-step way; largest difference "
          "of the maximised lnL %.1e"
          % (label, nt, name, t_eval * 1e3, len(queries), len(edges), len(PENDANT), t_grid * 1e3, len(rows3), t_one * 1e3, info["last_kernel_ms"], info["last_batches"],
             t_one / t_grid, len(pairs), calls, t_ml * 1e3, nt + 1, n_calls, passes[0] * 1e3, passes[1] * 1e3, passes[0] / t_ml, passes[1] / t_ml, dev), flush=True)
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
