"""numpy restatement of the placement scores (paml_amd_placement_scores), from the definition at the top of paml_amd/csrc/kernels_place.h.
Inputs are the per-branch matrices themselves, as in nni_ref.py: P[gene][class][node] = P(t_v) of the branch above `node` (row = the
father's state), Pup = P((1 - phi) t_v), Pdn = P(phi t_v) in the same shape, and Ppend[gene][class][j] = P_{pendant_label}(tau_j).  For the
edge v (the branch above v), f = the father of v, M_u = P_u L_u:

  down   (post-order)  L_u = prod_{c son of u} M_c                           (a tip: the indicator of its code's state set)
  outer  (pre-order)   A_root = pi (a root that is a tip: pi o its indicator);  A_u = P_u^T (A_g prod_{c sibling of u} M_c), g = father of u
  edge                 H_v = A_f prod_{c son of f, c != v} M_c;   U_v = Pup_v^T H_v;   D_v = Pdn_v L_v;   W_v = U_v o D_v
  query                f_hk = sum_y W_v(y) T_j[code_q(h)][y],  T_j[c][y] = sum_{x in set(c)} Ppend_j[y][x];   lnf = log sum_k freqK_k f_hk

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import copy

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, matrices_from_oracle, tips_of


def placement_scores(P, Pup, Pdn, Ppend, pi, freqK, tips, tree, weights, queries, edges=None):
    """dict(edges [n_e], lnf [n_q][n_e][n_pend][n_patt], lnL [n_q][n_e][n_pend], lnf0 [n_patt], lnL0) of the definition above."""
    z, sets, gene_off = tips
    n, nt, root = P.shape[-1], tree.n_tips, tree.root
    father, post = _father(tree), _postorder(tree)
    edges = [v for v in range(tree.n_nodes) if v != root] if edges is None else [int(v) for v in edges]
    queries = np.atleast_2d(np.asarray(queries, dtype=np.uint8))
    n_q, n_pend = len(queries), Ppend.shape[2]
    weights = np.asarray(weights, dtype=np.float64)
    lnf, lnf0 = np.zeros((n_q, len(edges), n_pend, z.shape[1])), np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f, f0 = np.zeros((n_q, len(edges), n_pend, m)), np.zeros(m)
        for k in range(len(freqK)):
            L, M, A = {}, {}, {}
            for u in post:                                   # down
                L[u] = _indicator(z[u, lo:hi], sets, n) if u < nt else np.ones((m, n))
                for c in tree.sons[u]:
                    L[u] = L[u] * M[c]
                if u != root:
                    M[u] = L[u] @ P[g, k, u].T
            A[root] = pi_g[None, :] * (_indicator(z[root, lo:hi], sets, n) if root < nt else np.ones((m, n)))
            f0 += freqK[k] * (L[root] * pi_g[None, :]).sum(axis=1)
            for u in reversed(post):                         # outer
                if u == root or u < nt:
                    continue
                H = A[father[u]].copy()
                for c in tree.sons[father[u]]:
                    if c != u:
                        H = H * M[c]
                A[u] = H @ P[g, k, u]
            # the tip tables of the pendant lengths: T[j][code][y]
            T = [np.stack([Ppend[g, k, j][:, s].sum(axis=1) for s in sets]) for j in range(n_pend)]
            for i, v in enumerate(edges):                    # edges
                H = A[father[v]].copy()
                for c in tree.sons[father[v]]:
                    if c != v:
                        H = H * M[c]
                Lv = L[v] if v >= nt else _indicator(z[v, lo:hi], sets, n)
                W = (H @ Pup[g, k, v]) * (Lv @ Pdn[g, k, v].T)
                for qi in range(n_q):
                    for j in range(n_pend):
                        f[qi, i, j] += freqK[k] * (W * T[j][queries[qi, lo:hi]]).sum(axis=1)
        lnf[..., lo:hi] = np.log(f)
        lnf0[lo:hi] = np.log(f0)
    live = weights > 0
    return dict(edges=np.asarray(edges, dtype=np.int32), lnf=lnf, lnL=lnf[..., live] @ weights[live], lnf0=lnf0,
                lnL0=float(np.dot(weights[live], lnf0[live])))


def _with_branch(pb, branch, label=None):
    q = copy.copy(pb)
    q.tree = copy.copy(pb.tree)
    q.tree.branch = np.asarray(branch, dtype=np.float64)
    if label is not None:
        q.tree.label = np.asarray(label, dtype=np.int32)
    return q


def placement_matrices(pb, phi, pendant, pendant_label=0):
    """(P, Pup, Pdn, Ppend) of a Problem from the CPU oracle: the tree's own lengths, their upper and lower parts, the pendant lengths
    (built in the slot of a non-root tip relabelled pendant_label)."""
    import oracle
    t = pb.tree
    P = matrices_from_oracle(pb)
    Pup = matrices_from_oracle(_with_branch(pb, (1 - phi) * t.branch))
    Pdn = matrices_from_oracle(_with_branch(pb, phi * t.branch))
    slot = 0 if t.root != 0 else 1
    Ppend = np.zeros((pb.n_genes, pb.K, len(pendant), pb.n, pb.n))
    for j, tau in enumerate(pendant):
        br, lab = t.branch.copy(), t.label.copy()
        br[slot], lab[slot] = tau, pendant_label
        q = _with_branch(pb, br, lab)
        for g in range(pb.n_genes):
            for k in range(pb.K):
                Ppend[g, k, j] = oracle.pmat_branch(q, g, k, slot)
    return P, Pup, Pdn, Ppend


def placement_scores_of(pb, queries, phi, pendant, pendant_label=0, edges=None):
    """The restatement on a Problem, its matrices from the CPU oracle."""
    P, Pup, Pdn, Ppend = placement_matrices(pb, phi, pendant, pendant_label)
    return placement_scores(P, Pup, Pdn, Ppend, pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights, queries, edges)


def inserted_problem(pb, v, phi, pendant, qrow, label=0, scale_every=None):
    """pb on the tree with the query hung on the branch above v (Tree.insert_tip), the query as tip row n_tips.  A problem made with
    `scale_every` gets the enlarged tree's own scaling marks (helpers.set_node_scale), as the host would mark a tree it loads."""
    import helpers
    q = copy.copy(pb)
    q.tree = pb.tree.insert_tip(int(v), phi, pendant, label)
    q.z = np.ascontiguousarray(np.vstack([pb.z, np.asarray(qrow, dtype=np.uint8)[None, :]]), dtype=np.uint8)
    if pb.scale_node is not None:
        assert scale_every, "a problem with scaling nodes: say the scale_every it was made with"
        q.scale_node = np.ascontiguousarray(helpers.set_node_scale(q.tree, scale_every), dtype=np.uint8)
    return q


def queries_of(pb, seed=0):
    """The three queries of the parity tests: a copy of a tip's row, a random row over all codes, and an all-"missing" row (a code whose
    set is every state) where the table has that code."""
    rng = np.random.default_rng(seed)
    rows = [pb.z[1].copy(), rng.integers(0, pb.n_codes, size=pb.n_patt).astype(np.uint8)]
    missing = [c for c in range(pb.n_codes) if pb.n_chara[c] == pb.n]
    if missing:
        rows.append(np.full(pb.n_patt, missing[0], dtype=np.uint8))
    return np.ascontiguousarray(np.stack(rows), dtype=np.uint8)
