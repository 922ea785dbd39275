"""A SHA-256 of what every whole-tree call returns on a fixed list of small problems: one line per (problem, call).  Two libraries
compute the same bytes exactly when their outputs are the same file:
    python tools/whole_tree_bytes.py > profiles/whole_tree_bytes.txt
    PAML_AMD_LIB=<dir>/libpaml_amd.so python tools/whole_tree_bytes.py > profiles/whole_tree_bytes_parent.txt      (a library built from
                                                                           another commit's sources, as engine.build() documents)
Calls: gradient (grad, lnf, scores), nni_scores / placement_scores / spr_scores (lnL0, lnL, lnf), edge_scores / attach_scores (lnL0, lnL,
d1, d2, lnf) on the rows of tests/{edge,attach}_ref.all_rows, relabel_scores (lnL0, lnL, lnf, lnfk0, lnfk) on every (node, label) of the
problem with three labels added (tests/relabel_ref.add_labels; an engine of its own), ancestral_marginal (best, prob, post),
ancestral_joint on the problems of one class (states, ln_best).  The six score calls run twice: with the default workspace, and with
PAML_AMD_{NNI,PLACE,SPR,EDGE,ATTACH,RELABEL}_ARENA_MB so small that the patterns are walked in several batches and the rows in several
groups (the values of tests/test_{nni,placement,spr,edge,attach}_gpu.py: test_groups_of_*; relabel: the value of
test_groups_of_rows_on_the_lane_kernels_have_the_same_bytes, since the 1 MiB of test_batches_groups_orders_and_calls_have_the_same_bytes
holds all of a 150-pattern problem of few states); a "small" line is refused if the call was not split.  The problems are
tests/helpers.random_problem's, 150 patterns or fewer: 4 / 5 / 20 / 21 / 61 / 64 states, one and three classes, two genes, scaling every
3 nodes, a tree rooted at a tip, the 14-tip polytomy.  Reads nothing outside the repository."""
import copy
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attach_ref      # noqa: E402
import edge_ref      # noqa: E402
import helpers      # noqa: E402
import placement_ref      # noqa: E402
import relabel_ref      # noqa: E402
from paml_amd import engine      # noqa: E402
from paml_amd.problem import Tree      # noqa: E402

PHI, PENDANT = 0.3, (0.05, 0.4)


def rooted_at_tip0(pb):
    """pb with its tree re-rooted at tip 0 (the same unrooted tree and branch lengths)."""
    t = pb.tree
    father = [-1] * t.n_nodes
    for v in range(t.n_nodes):
        for s in t.sons[v]:
            father[s] = v
    nbr = [list(t.sons[v]) + ([father[v]] if father[v] >= 0 else []) for v in range(t.n_nodes)]
    sons, branch = [[] for _ in range(t.n_nodes)], np.zeros(t.n_nodes)
    stack = [(0, -1)]
    while stack:
        v, par = stack.pop()
        for w in nbr[v]:
            if w != par:
                sons[v].append(w)
                branch[w] = t.branch[v] if father[v] == w else t.branch[w]
                stack.append((w, v))
    q = copy.copy(pb)
    q.tree = Tree(t.n_tips, t.n_nodes, 0, sons, branch, t.label.copy())
    return q


# (name, problem, engine flags)
PROBLEMS = [
    ("4-K3-amb-scale3-2genes", lambda: helpers.random_problem(4, 9, 150, K=3, ambiguity=True, scale_every=3, n_genes=2, seed=213), 0),
    ("4-K3-tip-root", lambda: rooted_at_tip0(helpers.random_problem(4, 9, 140, K=3, seed=55)), 0),
    ("5-K1", lambda: helpers.random_problem(5, 9, 150, K=1, seed=214), 0),
    ("20-K3-amb-scale3", lambda: helpers.random_problem(20, 9, 150, K=3, ambiguity=True, scale_every=3, seed=229), 0),
    ("20-K1-keep-partials", lambda: helpers.random_problem(20, 9, 150, K=1, seed=71), engine.KEEP_PARTIALS),
    ("21-K1", lambda: helpers.random_problem(21, 9, 150, K=1, seed=321), 0),
    ("61-K3-amb-scale3-2genes", lambda: helpers.random_problem(61, 9, 150, K=3, ambiguity=True, scale_every=3, n_genes=2, seed=270), 0),
    ("61-K1-tip-root", lambda: rooted_at_tip0(helpers.random_problem(61, 9, 140, K=1, seed=98)), 0),
    ("61-14tips-polytomy", lambda: helpers.random_problem(61, 14, 130, polytomy=True, seed=275), 0),
    ("64-K1", lambda: helpers.random_problem(64, 9, 150, K=1, seed=364), 0),
]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def report(name, call, sha, note=""):
    print("%-26s %-22s %s%s" % (name, call, sha, note), flush=True)


def scores(name, call, env, small_mb, rows, rows_per_group, info, run, keys=("lnL", "lnf")):
    """The call with the default workspace, then with `small_mb` MiB: several batches, and `rows` in groups of `rows_per_group` or fewer.
    Hashed: lnL0, then the arrays `keys`."""
    def sha(got):
        return digest(np.float64(got["lnL0"]), *[got[k] for k in keys])
    os.environ.pop(env, None)
    got = run()
    report(name, call, sha(got), "  batches %d" % info()["last_batches"])
    os.environ[env] = "%.9f" % small_mb
    got = run()
    os.environ.pop(env)
    batches = info()["last_batches"]
    if batches < 2 or rows <= rows_per_group:
        raise SystemExit("%s %s: %d batches, %d rows in groups of %d: the small workspace does not split the call" % (name, call, batches, rows, rows_per_group))
    report(name, call + "/small", sha(got), "  batches %d" % batches)


def main():
    for name, make, flags in PROBLEMS:
        pb = make()
        t = pb.tree
        eng = engine.engine_for(pb, flags=flags)
        b, gr = t.branch, pb.gene_rate
        g = eng.gradient(b, gr, want_lnf=True, want_scores=True)
        report(name, "gradient", digest(np.float64(g["lnL"]), g["grad"], g["lnf"], g["scores"]))
        K, n_int = pb.K, t.n_nodes - t.n_tips
        ns = pb.n if pb.n <= 20 else 64      # doubles a partial takes per pattern (20 states on the matrix cores: 64, and a smaller group)
        per_row = (2 * K + 1) * 8
        fixed = 2 * K * n_int * (ns + 1) * 8
        n_swaps = len(t.nni_swaps())
        scores(name, "nni_scores", "PAML_AMD_NNI_ARENA_MB", (fixed + 5.5 * per_row) * 64 / 1048576.0, n_swaps, 4, engine.nni_info,
               lambda: eng.nni_scores(b, gr, want_lnf=True))
        queries = placement_ref.queries_of(pb, seed=3)
        per_edge = per_row * len(queries) * len(PENDANT)
        scores(name, "placement_scores", "PAML_AMD_PLACE_ARENA_MB", (fixed + per_row + 4.5 * per_edge) * 64 / 1048576.0, t.n_nodes - 1, 4,
               engine.placement_info, lambda: eng.placement_scores(b, gr, queries=queries, pendant=PENDANT, phi=PHI, want_lnf=True))
        moves = eng.spr_scores(b, gr)["moves"]
        most = int(np.bincount(moves[:, 0]).max())
        scores(name, "spr_scores", "PAML_AMD_SPR_ARENA_MB", (2 * fixed + (2 * most + 1.5) * per_row) * 64 / 1048576.0, len(moves), 2 * most,
               engine.spr_info, lambda: eng.spr_scores(b, gr, phi=PHI, want_lnf=True))
        per_row3 = (4 * K + 3) * 8      # (lnL, d1 and d2 of a row)
        rows, on, ot = edge_ref.all_rows(t, seed=5)
        scores(name, "edge_scores", "PAML_AMD_EDGE_ARENA_MB", (fixed + 5.5 * per_row3) * 64 / 1048576.0, len(rows), 4, engine.edge_info,
               lambda: eng.edge_scores(b, gr, rows, on, ot, want_lnf=True), keys=("lnL", "d1", "d2", "lnf"))
        arows, t3 = attach_ref.all_rows(pb, len(queries), seed=5)
        scores(name, "attach_scores", "PAML_AMD_ATTACH_ARENA_MB", (fixed + 4.5 * per_row3) * 64 / 1048576.0, len(arows), 3, engine.attach_info,
               lambda: eng.attach_scores(b, gr, queries, arows, t3, want_lnf=True), keys=("lnL", "d1", "d2", "lnf"))
        m = eng.ancestral_marginal(b, gr)
        report(name, "ancestral_marginal", digest(m["best"], m["prob"], m["post"]))
        if K == 1:
            j = eng.ancestral_joint(b, gr)
            report(name, "ancestral_joint", digest(j["states"], j["ln_best"]))
        eng.close()
        lpb = relabel_ref.add_labels(copy.deepcopy(pb), seed=7)      # relabel_scores wants labels that select something
        eng = engine.engine_for(lpb, flags=flags)
        scores(name, "relabel_scores", "PAML_AMD_RELABEL_ARENA_MB", (fixed + 6.5 * (3 * K + 1) * 8) * 64 / 1048576.0, 3 * (t.n_nodes - 1), 5,
               engine.relabel_info, lambda: eng.relabel_scores(lpb.tree.branch, lpb.gene_rate, want_lnf=True, want_classes=True),
               keys=("lnL", "lnf", "lnfk0", "lnfk"))
        eng.close()


if __name__ == "__main__":
    main()
