"""numpy restatement of the scores of the configurations of an edge at trial lengths of the five branches around it
(paml_amd_edge_scores), from the definition at the top of paml_amd/csrc/kernels_edge.h.  Inputs are the tree's per-branch matrices, as in
nni_ref.py: P[gene][class][node] = P(t) of the branch above `node` (row = the father's state); the override matrices are made here
(pmat3).  For the row (v, s, x, u) with override nodes o and lengths t, f = the father of v, M_c = P_c L_c, S'_v and S'_f the son sets
after the swap (s = x = -1: none), P_c(.) at the override length where c is listed:

  A^_f  = A_f                                            f not overridden (the root: pi, a tip root: pi o its indicator)
        = P_f(t_f)^T [ A_ff prod_{sibling b of f} M_b ]  f overridden, ff = father(f)
  Y     = A^_f prod_{c in S'_f, c != v} P_c(t_c) L_c;    X = prod_{c in S'_v} P_c(t_c) L_c
  f_hk  = sum_y Y(y) (P_v(t_v) X)(y);    f'_hk, f''_hk: P_u replaced by dP_u/dt, d2P_u/dt2
  lnf = log sum_k freqK_k f_hk;  g1 = sum_k freqK_k f'_hk / sum_k freqK_k f_hk;  g2 = sum_k freqK_k f''_hk / sum_k freqK_k f_hk - g1^2
  lnL, d1, d2 = the sums of w lnf, w g1, w g2 over the patterns of weight > 0

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of
from paml_amd.problem import EIGEN_CIJK, EIGEN_JC69LIKE, EIGEN_K80, EIGEN_UVROOT


def pmat3(pb, g, k, node, t, gene_rate=None):
    """[3][n][n] = P, dP/dt, d2P/dt2 of the branch above `node` (its label's eigen set) at length t, gene g, class k, by the formulas of
    pmat_deriv_kernel (kernels_branch.h): mu_j = gene rate x class rate x Qfactor x Root_j, P = sum_j U[:, j] e^{t mu_j} V[j, :] with the
    j = 0 term's exponential 1, the derivatives with mu_j and mu_j^2 (the Cijk form likewise; K80 and JC69-like by their two / one
    non-zero rates, Qfactor not applied)."""
    n = pb.n
    gene_rate = pb.gene_rate if gene_rate is None else np.asarray(gene_rate, dtype=np.float64)
    rate = pb.rate[g, k] if pb.rate_per_gene else pb.rate[k]
    lab = int(pb.tree.label[node])
    es = pb.eigen[int(pb.eigen_of[g, k, lab])]
    kind, t = es["kind"], float(t)
    base = gene_rate[g] * rate * (pb.qfactor[k, lab] if kind == EIGEN_UVROOT else 1.0)
    out = np.zeros((3, n, n))
    if kind in (EIGEN_UVROOT, EIGEN_CIJK):
        nR = int(es["nR"]) if kind == EIGEN_CIJK else n
        mu = base * np.asarray(es["Root"])[:nR]
        e = np.exp(t * mu)
        e[0] = 1.0
        for d in range(3):
            c = e * mu ** d
            if d:
                c[0] = 0.0
            if kind == EIGEN_UVROOT:
                out[d] = (es["U"] * c[None, :]) @ es["V"]
            else:
                out[d] = (np.asarray(es["Cijk"]).reshape(n, n, nR) * c[None, None, :]).sum(axis=2)
    elif kind in (EIGEN_K80, EIGEN_JC69LIKE):
        i, j = np.indices((n, n))
        if kind == EIGEN_K80:
            kappa = float(es["kappa"])
            m1, m2 = base * -4 / (kappa + 2), base * -2 * (kappa + 1) / (kappa + 2)
            c1 = np.where((i == j) | ((i ^ j) == 1), 0.25, -0.25)
            c2 = np.where(i == j, 0.5, np.where((i ^ j) == 1, -0.5, 0.0))
        else:
            m1, m2 = base * -n / (n - 1.0), 0.0
            c1, c2 = np.where(i == j, 1 - 1.0 / n, -1.0 / n), np.zeros((n, n))
        for d in range(3):
            out[d] = c1 * m1 ** d * np.exp(t * m1) + c2 * m2 ** d * np.exp(t * m2)
        out[0] += 1.0 / n
    else:
        raise ValueError("no derivative formula for eigen kind %d" % kind)
    return out


def tree_passes(pb, P):
    """The down partials L, the messages M = P L and the outer messages A of the present tree per (gene, class): what every row shares.
    A list of (g, k, lo, hi, pi_g, L, M, A) and lnf0 [n_patt]."""
    tree = pb.tree
    z, sets, gene_off = tips_of(pb)
    pi, freqK = pb.pi, pb.freqK
    n, nt, root = P.shape[-1], tree.n_tips, tree.root
    father, post = _father(tree), _postorder(tree)
    out, lnf0 = [], np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f0 = np.zeros(m)
        for k in range(len(freqK)):
            L, M, A = {}, {}, {}
            for c in post:                                   # down
                L[c] = _indicator(z[c, lo:hi], sets, n) if c < nt else np.ones((m, n))
                for b in tree.sons[c]:
                    L[c] = L[c] * M[b]
                if c != root:
                    M[c] = L[c] @ P[g, k, c].T
            A[root] = pi_g[None, :] * (_indicator(z[root, lo:hi], sets, n) if root < nt else np.ones((m, n)))
            f0 += freqK[k] * (L[root] * pi_g[None, :]).sum(axis=1)
            for c in reversed(post):                         # outer
                if c == root or c < nt:
                    continue
                H = A[father[c]].copy()
                for b in tree.sons[father[c]]:
                    if b != c:
                        H = H * M[b]
                A[c] = H @ P[g, k, c]
            out.append((g, k, lo, hi, pi_g, L, M, A))
        lnf0[lo:hi] = np.log(f0)
    return out, lnf0


def edge_scores(pb, P, rows, ovr_node, ovr_t, gene_rate=None, passes=None):
    """dict(lnf, g1, g2 [n_rows][n_patt]; lnL, d1, d2 [n_rows]; lnf0 [n_patt], lnL0) of the definition above (passes: tree_passes(pb, P),
    made here when None)."""
    tree = pb.tree
    freqK = pb.freqK
    n = P.shape[-1]
    father = _father(tree)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    ovr_node = np.asarray(ovr_node, dtype=np.int64).reshape(-1, 5)
    ovr_t = np.asarray(ovr_t, dtype=np.float64).reshape(-1, 5)
    weights = np.asarray(pb.weights, dtype=np.float64)
    per_class, lnf0 = tree_passes(pb, P) if passes is None else passes
    F = np.zeros((3, len(rows), len(weights)))
    for g, k, lo, hi, pi_g, L, M, A in per_class:
        m = hi - lo
        for i, (v, s, x, u) in enumerate(rows):
            v, s, x, u = int(v), int(s), int(x), int(u)
            fa = father[v]
            ovr = {int(c): pmat3(pb, g, k, int(c), t, gene_rate) for c, t in zip(ovr_node[i], ovr_t[i]) if c >= 0}

            def Pm(c, d):
                if c in ovr:
                    return ovr[c][d if c == u else 0]
                return P[g, k, c]
            Sf = [s if c == x else c for c in tree.sons[fa] if c != v]
            Sv = [x if c == s else c for c in tree.sons[v]]
            for d in range(3 if u >= 0 else 1):
                if fa in ovr:
                    H = A[father[fa]].copy()
                    for b in tree.sons[father[fa]]:
                        if b != fa:
                            H = H * M[b]
                    Y = H @ Pm(fa, d)
                else:
                    Y = A[fa].copy()
                for c in Sf:
                    Y = Y * (L[c] @ Pm(c, d).T)
                X = np.ones((m, n))
                for c in Sv:
                    X = X * (L[c] @ Pm(c, d).T)
                F[d, i, lo:hi] += freqK[k] * (Y * (X @ Pm(v, d).T)).sum(axis=1)
    lnf = np.log(F[0])
    g1 = F[1] / F[0]
    g2 = F[2] / F[0] - g1 * g1
    live = weights > 0
    return dict(lnf=lnf, g1=g1, g2=g2, lnL=lnf[:, live] @ weights[live], d1=g1[:, live] @ weights[live], d2=g2[:, live] @ weights[live],
                lnf0=lnf0, lnL0=float(np.dot(weights[live], lnf0[live])))


def coordinate_ascent(pb, P, cfg, five, tol=1e-9, lo=4e-6, hi=50.0, max_sweeps=500, passes=None):
    """(t5, lnL): the configuration cfg = (v, s, x) maximised over the lengths of the branches `five`, everything else held fixed, started
    at the tree's lengths: the branches in turn, each by a safeguarded Newton iteration of its own (Newton's step where d2 < 0, otherwise
    the length doubled or halved along the gradient; clipped to [lo, hi]; halved until the lnL does not fall), until a sweep gains less
    than tol."""
    passes = tree_passes(pb, P) if passes is None else passes
    five = [int(c) for c in five]
    t = np.clip(np.array(pb.tree.branch, dtype=np.float64)[five], lo, hi)

    def val(tt, u):
        r = edge_scores(pb, P, [[cfg[0], cfg[1], cfg[2], u]], [five], [tt], passes=passes)
        return float(r["lnL"][0]), float(r["d1"][0]), float(r["d2"][0])
    l = val(t, -1)[0]
    for _ in range(max_sweeps):
        l_sweep = l
        for j, u in enumerate(five):
            for _ in range(60):
                l, d1, d2 = val(t, u)
                step = -d1 / d2 if d2 < 0 else (t[j] if d1 > 0 else -0.5 * t[j] if d1 < 0 else 0.0)
                tn = min(max(t[j] + step, lo), hi)
                gained = 0.0
                while abs(tn - t[j]) >= 1e-13:
                    t2 = t.copy()
                    t2[j] = tn
                    l2 = val(t2, -1)[0]
                    if l2 >= l:
                        gained, t, l = l2 - l, t2, l2
                        break
                    tn = 0.5 * (tn + t[j])
                if gained <= 1e-13:
                    break
        if l - l_sweep < tol:
            break
    return t, l


def rearranged_problem(pb, v, s, x, ovr_node, ovr_t, scale_every=None):
    """pb on the tree of the row's configuration with the override lengths written into its branch lengths (nni_ref.swapped_problem for
    a swap; s = x = -1: the present tree)."""
    import nni_ref as nr
    q = nr.swapped_problem(pb, v, s, x, scale_every) if s >= 0 else copy.copy(pb)
    branch = np.array(pb.tree.branch, dtype=np.float64)
    for c, t in zip(ovr_node, ovr_t):
        if c >= 0:
            branch[int(c)] = t
    q.tree = dataclasses.replace(q.tree, branch=branch)
    return q


def all_rows(tree, seed=1):
    """Every edge of tree.edge_configs(), all three configurations, each of the five branches around it as u, at lengths drawn in
    [0.5, 2] x the tree's (one draw per edge and configuration, shared by its five rows): (rows [n][4], ovr_node [n][5], ovr_t [n][5])."""
    rng = np.random.default_rng(seed)
    edges, five = tree.edge_configs()
    rows, on, ot = [], [], []
    for e in range(len(edges)):
        for cfg in edges[e]:
            t5 = tree.branch[five[e]] * rng.uniform(0.5, 2.0, 5)
            for u in five[e]:
                rows.append([cfg[0], cfg[1], cfg[2], u])
                on.append(list(five[e]))
                ot.append(t5)
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), np.asarray(on, dtype=np.int32).reshape(-1, 5), np.asarray(ot, dtype=np.float64).reshape(-1, 5)
