"""numpy restatement of the curvature along every branch (paml_amd_curvature), from the definition at the top of
paml_amd/csrc/kernels_curvature.h, built on gradient_ref.py's down and outer loops.  Inputs are the per-branch matrices themselves:
P[gene][class][node] = P(t) of the branch above `node` (row = the father's state), dP and d2P its first and second derivative with respect
to that branch length.

  e_vk   = sum_y H_v(y) (d2P_v L_v)(y)             beside f_hk and d_vk of gradient_ref.py
  c_v(h) = sum_k freqK_k e_vk / sum_k freqK_k f_hk - s_v(h)^2;        curv[v] = sum_h w_h c_v(h)

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of
from gradient_ref import dmatrices
from paml_amd.problem import EIGEN_CIJK, EIGEN_JC69LIKE, EIGEN_K80, EIGEN_UVROOT


def d2matrices(pb, branch=None, gene_rate=None):
    """d2P[gene][class][node] = d^2 P(t) / d branch[node]^2: gradient_ref.dmatrices' formulas with mu_k^2 in the place of mu_k."""
    n, t = pb.n, pb.tree
    branch = t.branch if branch is None else np.asarray(branch, dtype=np.float64)
    gene_rate = pb.gene_rate if gene_rate is None else np.asarray(gene_rate, dtype=np.float64)
    d2P = np.zeros((pb.n_genes, pb.K, t.n_nodes, n, n))
    for g in range(pb.n_genes):
        for k in range(pb.K):
            rate = pb.rate[g, k] if pb.rate_per_gene else pb.rate[k]
            for v in range(t.n_nodes):
                if v == t.root:
                    continue
                lab = int(t.label[v])
                es = pb.eigen[int(pb.eigen_of[g, k, lab])]
                kind, tv = es["kind"], float(branch[v])
                base = gene_rate[g] * rate * (pb.qfactor[k, lab] if kind == EIGEN_UVROOT else 1.0)
                if kind == EIGEN_UVROOT:
                    mu = base * np.asarray(es["Root"])
                    c = mu * mu * np.exp(tv * mu)
                    d2P[g, k, v] = (es["U"][:, 1:] * c[None, 1:]) @ es["V"][1:, :]
                elif kind == EIGEN_CIJK:
                    nR = int(es["nR"])
                    mu = base * np.asarray(es["Root"])[:nR]
                    c = mu * mu * np.exp(tv * mu)
                    d2P[g, k, v] = (np.asarray(es["Cijk"]).reshape(n, n, nR)[:, :, 1:] * c[None, None, 1:]).sum(axis=2)
                elif kind in (EIGEN_K80, EIGEN_JC69LIKE):
                    i, j = np.indices((n, n))
                    if kind == EIGEN_K80:
                        kappa = float(es["kappa"])
                        m1, m2 = base * -4 / (kappa + 2), base * -2 * (kappa + 1) / (kappa + 2)
                        c1 = np.where((i == j) | ((i ^ j) == 1), 0.25, -0.25)
                        c2 = np.where(i == j, 0.5, np.where((i ^ j) == 1, -0.5, 0.0))
                        d2P[g, k, v] = c1 * m1 * m1 * np.exp(tv * m1) + c2 * m2 * m2 * np.exp(tv * m2)
                    else:
                        m1 = base * -n / (n - 1.0)
                        d2P[g, k, v] = np.where(i == j, 1 - 1.0 / n, -1.0 / n) * m1 * m1 * np.exp(tv * m1)
                else:
                    raise ValueError("no derivative formula for eigen kind %d" % kind)
    return d2P


def curvature(P, dP, d2P, pi, freqK, tips, tree, weights):
    """dict(lnL, grad [n_nodes], curv [n_nodes], lnf [n_patt]) of the definition above.  lnL, grad and lnf are gradient_ref.gradient's
    statements, so they equal its results exactly."""
    z, sets, gene_off = tips
    n, nt, nn, root = P.shape[-1], tree.n_tips, tree.n_nodes, tree.root
    father, post = _father(tree), _postorder(tree)
    weights = np.asarray(weights, dtype=np.float64)
    lnf = np.zeros(z.shape[1])
    scores = np.zeros((nn, z.shape[1]))
    curvs = np.zeros((nn, z.shape[1]))
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f, d, e = np.zeros(m), np.zeros((nn, m)), np.zeros((nn, m))
        for k in range(len(freqK)):
            L, M, A = {}, {}, {}
            for v in post:                                   # down
                L[v] = _indicator(z[v, lo:hi], sets, n) if v < nt else np.ones((m, n))
                for s in tree.sons[v]:
                    L[v] = L[v] * M[s]
                if v != root:
                    M[v] = L[v] @ P[g, k, v].T
            A[root] = pi_g[None, :] * (_indicator(z[root, lo:hi], sets, n) if root < nt else 1.0)
            f += freqK[k] * (L[root] * pi_g[None, :]).sum(axis=1)
            for v in reversed(post):                         # outer + both derivatives
                if v == root:
                    continue
                H = A[father[v]].copy()
                for s in tree.sons[father[v]]:
                    if s != v:
                        H = H * M[s]
                d[v] += freqK[k] * (H * (L[v] @ dP[g, k, v].T)).sum(axis=1)
                e[v] += freqK[k] * (H * (L[v] @ d2P[g, k, v].T)).sum(axis=1)
                A[v] = H @ P[g, k, v]
        lnf[lo:hi] = np.log(f)
        scores[:, lo:hi] = d / f[None, :]
        curvs[:, lo:hi] = e / f[None, :] - scores[:, lo:hi] ** 2
    scores[:, weights == 0] = 0
    curvs[:, weights == 0] = 0
    return dict(lnL=float(np.dot(weights[weights != 0], lnf[weights != 0])), grad=scores @ weights, curv=curvs @ weights, lnf=lnf)


def curvature_of(pb, P, branch=None):
    """The restatement on a Problem and its matrices P (matrices_from_oracle / matrices_from_engine) at `branch` (default: the tree's)."""
    return curvature(P, dmatrices(pb, branch), d2matrices(pb, branch), pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights)


# The batching case of tests/test_curvature_gpu.py and the bytes a pattern takes in the workspace (curv_bytes_per_pattern,
# kernels_curvature.h): 2 K n_int (n_s + 1) doubles for the down partials and the outer messages with their log factors (n_s = 64 on
# the matrix cores), 4 K n_nodes doubles for f, d, e and their log factor per class, one for lnf.
BATCHING_CASE = dict(n=61, tips=9, patterns=3000, K=1)


def bytes_per_pattern(K, n_int, n_nodes, n_s):
    return 2 * K * n_int * (n_s + 1) * 8 + 4 * K * n_nodes * 8 + 8
