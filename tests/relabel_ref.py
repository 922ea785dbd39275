"""numpy restatement of the scores of the tree with one branch relabelled (paml_amd_relabel_scores), from the definition at the top of
paml_amd/csrc/kernels_relabel.h.  Inputs are the per-branch matrices themselves, as in nni_ref.py: P[gene][class][node] = P(t) of the
branch above `node` under the present labels, and Pnew[i][gene][class] = P'(t_v) of row i = (v, l): the matrix of the branch above v
under label l.  With f = the father of v and M_u = P_u L_u:

  down   (post-order)  L_u = prod_{c son of u} M_c                           (a tip: the indicator of its code's state set)
  outer  (pre-order)   A_root = pi (a root that is a tip: pi o its indicator);  A_u = P_u^T (A_g prod_{c sibling of u} M_c), g = father of u
  row                  H_v = A_f prod_{b son of f, b != v} M_b;   f_hk = sum_y H_v(y) (P'_v L_v)(y)
                       lnfk[i][k][h] = log f_hk;                  lnf[i][h] = log sum_k freqK_k f_hk

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import copy

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of


def all_rows(tree, n_labels):
    """Every non-root node with every label, in node order: what Engine.relabel_scores takes for rows=None."""
    return np.asarray([(v, l) for v in range(tree.n_nodes) if v != tree.root for l in range(n_labels)], dtype=np.int32).reshape(-1, 2)


def relabel_scores(P, Pnew, pi, freqK, tips, tree, weights, rows):
    """dict(rows, lnf [n_rows][n_patt], lnfk [n_rows][K][n_patt], lnL [n_rows], lnf0, lnfk0 [K][n_patt], lnL0) of the definition above."""
    z, sets, gene_off = tips
    n, nt, root, K = P.shape[-1], tree.n_tips, tree.root, len(freqK)
    father, post = _father(tree), _postorder(tree)
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.float64)
    n_patt = z.shape[1]
    with np.errstate(divide="ignore"):
        lnf, lnf0 = np.zeros((len(rows), n_patt)), np.zeros(n_patt)
        lnfk, lnfk0 = np.zeros((len(rows), K, n_patt)), np.zeros((K, n_patt))
        for g in range(len(gene_off) - 1):
            lo, hi = int(gene_off[g]), int(gene_off[g + 1])
            if hi <= lo:
                continue
            pi_g = pi[g if pi.shape[0] > 1 else 0]
            m = hi - lo
            f, f0 = np.zeros((len(rows), m)), np.zeros(m)
            for k in range(K):
                L, M, A = {}, {}, {}
                for u in post:                                   # down
                    L[u] = _indicator(z[u, lo:hi], sets, n) if u < nt else np.ones((m, n))
                    for c in tree.sons[u]:
                        L[u] = L[u] * M[c]
                    if u != root:
                        M[u] = L[u] @ P[g, k, u].T
                for u in range(nt):                              # (tips that are no one's father: not in the post-order)
                    if u not in L:
                        L[u] = _indicator(z[u, lo:hi], sets, n)
                A[root] = pi_g[None, :] * (_indicator(z[root, lo:hi], sets, n) if root < nt else np.ones((m, n)))
                fk0 = (L[root] * pi_g[None, :]).sum(axis=1)
                lnfk0[k, lo:hi] = np.log(fk0)
                f0 += freqK[k] * fk0
                for u in reversed(post):                         # outer
                    if u == root or u < nt:
                        continue
                    H = A[father[u]].copy()
                    for c in tree.sons[father[u]]:
                        if c != u:
                            H = H * M[c]
                    A[u] = H @ P[g, k, u]
                for i, (v, _) in enumerate(rows):                # rows
                    fa = father[v]
                    H = A[fa].copy()
                    for c in tree.sons[fa]:
                        if c != v:
                            H = H * M[c]
                    fk = (H * (L[v] @ Pnew[i][g, k].T)).sum(axis=1)
                    lnfk[i, k, lo:hi] = np.log(fk)
                    f[i] += freqK[k] * fk
            lnf[:, lo:hi] = np.log(f)
            lnf0[lo:hi] = np.log(f0)
    live = weights > 0
    return dict(rows=rows, lnf=lnf, lnfk=lnfk, lnL=lnf[:, live] @ weights[live], lnf0=lnf0, lnfk0=lnfk0, lnL0=float(np.dot(weights[live], lnf0[live])))


def relabelled_problem(pb, v, label):
    """pb on the tree with the branch above v relabelled (Tree.relabelled): topology, lengths and scaling marks stay."""
    q = copy.copy(pb)
    q.tree = pb.tree.relabelled(int(v), int(label))
    return q


def relabel_scores_of(pb, rows=None):
    """The restatement on a Problem, with every matrix from the CPU oracle."""
    import oracle
    import ancestral_ref as ar
    rows = all_rows(pb.tree, pb.n_labels) if rows is None else np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    Pnew = []
    for v, l in rows:
        q = relabelled_problem(pb, v, l)
        Pnew.append(np.array([[oracle.pmat_branch(q, g, k, int(v)) for k in range(pb.K)] for g in range(pb.n_genes)]))
    return relabel_scores(ar.matrices_from_oracle(pb), Pnew, pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights, rows)


def oracle_class_logs(pb, ref):
    """The logs of the oracle's class-conditional likelihoods fhK [K][n_patt]: the oracle keeps them as logs in lfun mode and on trees
    with scaling nodes, linear otherwise."""
    has_scale = pb.scale_node is not None and np.asarray(pb.scale_node).any()
    if int(pb.mode) == 0 or has_scale:
        return ref["fhK"]
    with np.errstate(divide="ignore"):
        return np.log(ref["fhK"])


def label_problem(n, K, genes, seed=None, n_tips=10, n_patt=160, n_labels=3):
    """A branch-model problem in the style of test_engine_gpu._branch_model_problem: every branch carries one of n_labels labels and
    (gene, class, label) selects one of several eigen systems and a rate factor."""
    import helpers
    seed = 400 + n + K if seed is None else seed
    return add_labels(helpers.random_problem(n, n_tips, n_patt, K=K, seed=seed, n_genes=genes), seed, n_labels)


def add_labels(pb, seed, n_labels=3):
    """pb with random branch labels, K n_labels further eigen systems, a random class table over all of them and random Qfactors."""
    import helpers
    rng = np.random.default_rng(seed)
    t = pb.tree
    pb.tree = type(t)(t.n_tips, t.n_nodes, t.root, t.sons, t.branch, rng.integers(0, n_labels, t.n_nodes).astype(np.int32), t.names)
    pb.tree.label[:3] = np.arange(3) % n_labels
    eig = [helpers.random_problem(pb.n, 4, 4, seed=seed + 100 + i).eigen[0] for i in range(pb.K * n_labels)]
    pb.eigen = [pb.eigen[0]] + eig
    pb.eigen_of = rng.integers(0, len(pb.eigen), size=(pb.n_genes, pb.K, n_labels)).astype(np.int32)
    pb.qfactor = 0.5 + rng.random((pb.K, n_labels))
    return pb


def labelled_reversible_problem(name):
    """A gradient_ref.REVERSIBLE_SHAPES problem (ambiguity codes, scaling marks, a polytomy) with three labels added."""
    import gradient_ref as gr
    return add_labels(gr.reversible_problem(name), 900 + len(name))


LABEL_SHAPES = [(4, 2, 1), (20, 1, 1), (61, 2, 2)]
REVERSIBLE_NAMES = ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"]
