"""numpy restatement of the scores of the nearest-neighbour-interchange neighbours (paml_amd_nni_scores), from the definition at the top of
paml_amd/csrc/kernels_nni.h.  Inputs are the per-branch matrices themselves, as in gradient_ref.py: P[gene][class][node] = P(t) of the
branch above `node` (row = the father's state).  For the swap (v, s, x), f = the father of v, M_u = P_u L_u:

  down   (post-order)  L_u = prod_{c son of u} M_c                           (a tip: the indicator of its code's state set)
  outer  (pre-order)   A_root = pi (a root that is a tip: pi o its indicator);  A_u = P_u^T (A_g prod_{c sibling of u} M_c), g = father of u
  swap                 L'_v = M_x prod_{s' son of v, s' != s} M_s';   H'_v = A_f M_s prod_{x' son of f, x' != v, x' != x} M_x'
                       f_hk = sum_y H'_v(y) (P_v L'_v)(y);            lnf[i][h] = log sum_k freqK_k f_hk

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import copy

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of


def nni_scores(P, pi, freqK, tips, tree, weights, swaps=None):
    """dict(swaps [n_swaps][3], lnf [n_swaps][n_patt], lnL [n_swaps], lnf0 [n_patt], lnL0) of the definition above."""
    z, sets, gene_off = tips
    n, nt, root = P.shape[-1], tree.n_tips, tree.root
    father, post = _father(tree), _postorder(tree)
    swaps = tree.nni_swaps() if swaps is None else np.asarray(swaps, dtype=np.int32).reshape(-1, 3)
    weights = np.asarray(weights, dtype=np.float64)
    lnf, lnf0 = np.zeros((len(swaps), z.shape[1])), np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f, f0 = np.zeros((len(swaps), m)), np.zeros(m)
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
            for i, (v, s, x) in enumerate(swaps):            # swaps
                fa = father[v]
                H = A[fa] * M[s]
                for c in tree.sons[fa]:
                    if c != v and c != x:
                        H = H * M[c]
                Lv = M[x].copy()
                for c in tree.sons[v]:
                    if c != s:
                        Lv = Lv * M[c]
                f[i] += freqK[k] * (H * (Lv @ P[g, k, v].T)).sum(axis=1)
        lnf[:, lo:hi] = np.log(f)
        lnf0[lo:hi] = np.log(f0)
    live = weights > 0
    return dict(swaps=swaps, lnf=lnf, lnL=lnf[:, live] @ weights[live], lnf0=lnf0, lnL0=float(np.dot(weights[live], lnf0[live])))


def nni_scores_of(pb, P, swaps=None):
    """The restatement on a Problem and its matrices P (ancestral_ref.matrices_from_oracle / matrices_from_engine)."""
    return nni_scores(P, pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights, swaps)


def swapped_problem(pb, v, s, x, scale_every=None):
    """pb on the rearranged tree (Tree.nni: node ids, branch lengths and labels stay).  A problem made with `scale_every` gets the
    rearranged tree's own scaling marks (helpers.set_node_scale), as the host would mark a tree it loads."""
    import helpers
    q = copy.copy(pb)
    q.tree = pb.tree.nni(int(v), int(s), int(x))
    if pb.scale_node is not None:
        assert scale_every, "a problem with scaling nodes: say the scale_every it was made with"
        q.scale_node = np.ascontiguousarray(helpers.set_node_scale(q.tree, scale_every), dtype=np.uint8)
    return q


def scale_every_of(name):
    """The scale_every keyword of a gradient_ref.REVERSIBLE_SHAPES entry (None: no scaling nodes)."""
    import gradient_ref as gr
    return dict((s[0], s[4].get("scale_every")) for s in gr.REVERSIBLE_SHAPES)[name]
