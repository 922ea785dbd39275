"""numpy restatement of the Hessian of lnL over all branch lengths (paml_amd_hessian), from the definition at the top of
paml_amd/csrc/kernels_hessian.h, built on gradient_ref.py's down and outer loops.  Inputs are the per-branch matrices themselves:
P[gene][class][node] = P(t) of the branch above `node` (row = the father's state), dP and d2P its first and second derivative with respect
to that branch length.

  source u (not the root), D_u = dP_u L_u
  up the path   L'_{a_1} = D_u o prod_{siblings of u} M_s;  L'_{a_{i+1}} = (P_{a_i} L'_{a_i}) o prod_{other sons} M_s;  m_{u,a,k} = H_a . (dP_a L'_a)
  outwards      H'_w = A_a o M'_c o prod_{other siblings of w} M_s  (M'_c = P_c L'_c, or D_u when c = u);  A'_w = P_w^T H'_w;
                H'_x = A'_w o prod_{siblings of x} M_s;  m_{u,w,k} = H'_w . (dP_w L_w)
  entries       Hess[u][v] = sum_h w_h (sum_k freqK_k m_uvk / sum_k freqK_k f_k - s_u(h) s_v(h));  Hess[v][v] = curvature_ref's curv[v]

Every ordered pair (u, v) with v not below u is computed with u as the source (`routes`), so an unrelated pair has both of its routes;
`hess` takes the engine's rule (hess_source_of, hessian_plan.h: of an unrelated pair the node with the smaller number is the source) and
mirrors.  Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of
from curvature_ref import curvature, d2matrices
from gradient_ref import dmatrices, gradient


def below(tree):
    """below[u][v]: v lies in the subtree below u (v != u)."""
    father = _father(tree)
    b = np.zeros((tree.n_nodes, tree.n_nodes), dtype=bool)
    for v in range(tree.n_nodes):
        a = father[v]
        while a is not None and a >= 0:
            b[a, v] = True
            a = father[a]
    return b


def hessian(P, dP, d2P, pi, freqK, tips, tree, weights):
    """dict(lnL, grad [n_nodes], hess [n_nodes][n_nodes], lnf [n_patt], routes [n_nodes][n_nodes] (entry [u][v]: with u as the source; nan
    where v lies below u, on the diagonal and at the root), muv [n_nodes][n_nodes][n_patt] = sum_k freqK_k m_uvk with u as the source,
    f [n_patt] = sum_k freqK_k f_k)."""
    z, sets, gene_off = tips
    n, nt, nn, root = P.shape[-1], tree.n_tips, tree.n_nodes, tree.root
    father, post = _father(tree), _postorder(tree)
    weights = np.asarray(weights, dtype=np.float64)
    diag = curvature(P, dP, d2P, pi, freqK, tips, tree, weights)
    scores = gradient(P, dP, pi, freqK, tips, tree, weights)["scores"]
    muv = np.full((nn, nn, z.shape[1]), np.nan)
    fall = np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        acc = {}
        for k in range(len(freqK)):
            L, M, A, H = {}, {}, {}, {}
            for v in post:                                   # down
                L[v] = _indicator(z[v, lo:hi], sets, n) if v < nt else np.ones((m, n))
                for s in tree.sons[v]:
                    L[v] = L[v] * M[s]
                if v != root:
                    M[v] = L[v] @ P[g, k, v].T
            A[root] = pi_g[None, :] * (_indicator(z[root, lo:hi], sets, n) if root < nt else 1.0)
            fall[lo:hi] += freqK[k] * (L[root] * pi_g[None, :]).sum(axis=1)
            for v in reversed(post):                         # outer
                if v == root:
                    continue
                H[v] = A[father[v]].copy()
                for s in tree.sons[father[v]]:
                    if s != v:
                        H[v] = H[v] * M[s]
                A[v] = H[v] @ P[g, k, v]

            def add(u, v, val):
                acc[(u, v)] = acc.get((u, v), 0.0) + freqK[k] * val

            def outwards(u, w, Hw):
                add(u, w, (Hw * (L[w] @ dP[g, k, w].T)).sum(axis=1))
                if tree.sons[w]:
                    Aw = Hw @ P[g, k, w]
                    for x in tree.sons[w]:
                        Hx = Aw.copy()
                        for s in tree.sons[w]:
                            if s != x:
                                Hx = Hx * M[s]
                        outwards(u, x, Hx)

            for u in range(nn):
                if u == root:
                    continue
                c, Mc, a = u, L[u] @ dP[g, k, u].T, father[u]
                while a is not None and a >= 0:
                    for w in tree.sons[a]:                   # outwards from the path node a
                        if w == c:
                            continue
                        Hw = A[a] * Mc
                        for s in tree.sons[a]:
                            if s != w and s != c:
                                Hw = Hw * M[s]
                        outwards(u, w, Hw)
                    if a == root:
                        break
                    Lp = Mc.copy()                           # up the path
                    for s in tree.sons[a]:
                        if s != c:
                            Lp = Lp * M[s]
                    add(u, a, (H[a] * (Lp @ dP[g, k, a].T)).sum(axis=1))
                    c, Mc, a = a, Lp @ P[g, k, a].T, father[a]
        for (u, v), val in acc.items():
            muv[u, v, lo:hi] = val
    live = weights != 0
    routes = np.full((nn, nn), np.nan)
    for u in range(nn):
        for v in range(nn):
            if not np.isnan(muv[u, v, 0]):
                term = muv[u, v] / fall - scores[u] * scores[v]
                routes[u, v] = float(np.dot(weights[live], term[live]))
    is_below = below(tree)
    hess = np.zeros((nn, nn))
    for u in range(nn):
        for v in range(nn):
            if u == root or v == root:
                continue
            if u == v:
                hess[u, u] = diag["curv"][u]
            elif is_below[u, v]:
                hess[u, v] = routes[v, u]
            elif is_below[v, u]:
                hess[u, v] = routes[u, v]
            else:
                hess[u, v] = routes[min(u, v), max(u, v)]
    return dict(lnL=diag["lnL"], grad=diag["grad"], hess=hess, lnf=diag["lnf"], routes=routes, muv=muv, f=fall)


def caterpillar_problem(n, n_tips, n_patt, seed=0, **kw):
    """helpers.random_problem's model and tips on a rooted caterpillar: the root's sons are tip 0 and an internal node, and so on down
    to the last cherry — the longest paths a tree of n_tips has."""
    import helpers
    from paml_amd.problem import Tree
    pb = helpers.random_problem(n, n_tips, n_patt, seed=seed, **kw)
    nn = 2 * n_tips - 1
    sons = [[] for _ in range(nn)]
    for i in range(n_tips - 2):
        sons[n_tips + i] = [i, n_tips + i + 1]
    sons[nn - 1] = [n_tips - 2, n_tips - 1]
    branch = np.random.default_rng(seed + 1).uniform(0.02, 0.3, size=nn)
    branch[n_tips] = 0
    pb.tree = Tree(n_tips, nn, n_tips, sons, branch, np.zeros(nn, dtype=np.int32))
    pb.scale_node = None
    return pb


def star_problem(n, n_patt, seed=0, **kw):
    """Three tips under the root: every pair is a pair of siblings and no source has a path."""
    import helpers
    pb = helpers.random_problem(n, 3, n_patt, seed=seed, **kw)
    assert pb.tree.n_nodes == 4 and len(pb.tree.sons[pb.tree.root]) == 3
    return pb


def two_tip_problem(n, n_patt, seed=0, **kw):
    """A rooted tree of two tips: one pair."""
    import helpers
    pb = helpers.random_problem(n, 2, n_patt, seed=seed, **kw)
    assert pb.tree.n_nodes == 3 and len(pb.tree.sons[pb.tree.root]) == 2
    return pb


def hessian_of(pb, P, branch=None):
    """The restatement on a Problem and its matrices P (matrices_from_oracle / matrices_from_engine) at `branch` (default: the tree's)."""
    return hessian(P, dmatrices(pb, branch), d2matrices(pb, branch), pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights)
