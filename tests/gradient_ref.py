"""numpy restatement of the branch-length gradient and the per-pattern scores (paml_amd_gradient), from the definition at the top of
paml_amd/csrc/kernels_gradient.h.  Inputs are the per-branch matrices themselves, as in ancestral_ref.py: P[gene][class][node] = P(t) of the
branch above `node` (row = the father's state) and dP[gene][class][node] = its derivative with respect to that branch length.

  down   (post-order)  L_v = prod_{s son of v} M_s,  M_s = P_s L_s             (a tip: the indicator of its code's state set)
  outer  (pre-order)   A_root = pi (a root that is a tip: pi o its indicator);  H_v = A_f prod_{s sibling of v} M_s;  A_v = P_v^T H_v
  identity             f_hk = sum_y H_v(y) (P_v L_v)(y)  at every non-root v;   d_vk = sum_y H_v(y) (dP_v L_v)(y)
  score                s_v(h) = sum_k freqK_k d_vk / sum_k freqK_k f_hk;        grad[v] = sum_h w_h s_v(h)

Nothing is re-rooted and no reversibility is assumed: grad[v] is the derivative of the lnL of the tree as it is rooted, whatever eigen
systems its branches carry.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import numpy as np

from ancestral_ref import _father, _indicator, _postorder, tips_of      # noqa: F401  (tips_of: for the callers)
from paml_amd.problem import EIGEN_CIJK, EIGEN_JC69LIKE, EIGEN_K80, EIGEN_UVROOT


def dmatrices(pb, branch=None, gene_rate=None):
    """dP[gene][class][node] = d P(t) / d branch[node] by the formulas of pmat_deriv_kernel (kernels_branch.h): with
    mu_k = gene_rate x rate_k x qfactor(class, label) x Root_k,  dP = sum_{k >= 1} U[:, k] mu_k e^{t mu_k} V[k, :]  (the Cijk form
    likewise; K80 and JC69-like by their two / one non-zero rates, qfactor not applied)."""
    n, t = pb.n, pb.tree
    branch = t.branch if branch is None else np.asarray(branch, dtype=np.float64)
    gene_rate = pb.gene_rate if gene_rate is None else np.asarray(gene_rate, dtype=np.float64)
    dP = np.zeros((pb.n_genes, pb.K, t.n_nodes, n, n))
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
                    c = mu * np.exp(tv * mu)
                    dP[g, k, v] = (es["U"][:, 1:] * c[None, 1:]) @ es["V"][1:, :]
                elif kind == EIGEN_CIJK:
                    nR = int(es["nR"])
                    mu = base * np.asarray(es["Root"])[:nR]
                    c = mu * np.exp(tv * mu)
                    dP[g, k, v] = (np.asarray(es["Cijk"]).reshape(n, n, nR)[:, :, 1:] * c[None, None, 1:]).sum(axis=2)
                elif kind in (EIGEN_K80, EIGEN_JC69LIKE):
                    i, j = np.indices((n, n))
                    if kind == EIGEN_K80:
                        kappa = float(es["kappa"])
                        m1, m2 = base * -4 / (kappa + 2), base * -2 * (kappa + 1) / (kappa + 2)
                        c1 = np.where((i == j) | ((i ^ j) == 1), 0.25, -0.25)
                        c2 = np.where(i == j, 0.5, np.where((i ^ j) == 1, -0.5, 0.0))
                        dP[g, k, v] = c1 * m1 * np.exp(tv * m1) + c2 * m2 * np.exp(tv * m2)
                    else:
                        m1 = base * -n / (n - 1.0)
                        dP[g, k, v] = np.where(i == j, 1 - 1.0 / n, -1.0 / n) * m1 * np.exp(tv * m1)
                else:
                    raise ValueError("no derivative formula for eigen kind %d" % kind)
    return dP


def gradient(P, dP, pi, freqK, tips, tree, weights):
    """dict(lnL, grad [n_nodes], lnf [n_patt], scores [n_nodes][n_patt]) of the definition above."""
    z, sets, gene_off = tips
    n, nt, nn, root = P.shape[-1], tree.n_tips, tree.n_nodes, tree.root
    father, post = _father(tree), _postorder(tree)
    weights = np.asarray(weights, dtype=np.float64)
    lnf = np.zeros(z.shape[1])
    scores = np.zeros((nn, z.shape[1]))
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f, d = np.zeros(m), np.zeros((nn, m))
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
            for v in reversed(post):                         # outer + derivative
                if v == root:
                    continue
                H = A[father[v]].copy()
                for s in tree.sons[father[v]]:
                    if s != v:
                        H = H * M[s]
                d[v] += freqK[k] * (H * (L[v] @ dP[g, k, v].T)).sum(axis=1)
                A[v] = H @ P[g, k, v]
        lnf[lo:hi] = np.log(f)
        scores[:, lo:hi] = d / f[None, :]
    scores[:, weights == 0] = 0
    grad = scores @ weights
    return dict(lnL=float(np.dot(weights[weights != 0], lnf[weights != 0])), grad=grad, lnf=lnf, scores=scores)


def gradient_of(pb, P):
    """The restatement on a Problem and its matrices P (matrices_from_oracle / matrices_from_engine)."""
    return gradient(P, dmatrices(pb), pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights)


# The exactly reversible shapes of the parity tests (helpers.random_problem; tests/test_gradient_cpu.py pins the restatement on them
# against oracle.eval_branch, tests/test_gradient_gpu.py takes the engine through them): (name, states, tips, patterns, keywords).
# 150 and 130 patterns leave a partial wave and a partial 64-pattern tile in every kernel family.
REVERSIBLE_SHAPES = [
    ("4-K3-amb-scale3-2genes", 4, 9, 150, dict(K=3, ambiguity=True, scale_every=3, n_genes=2)),
    ("5-K1", 5, 9, 150, dict(K=1)),
    ("20-K2-amb", 20, 9, 150, dict(K=2, ambiguity=True)),
    ("61-K2-amb-scale3", 61, 9, 150, dict(K=2, ambiguity=True, scale_every=3)),
    ("61-14tips-polytomy", 61, 14, 130, dict(polytomy=True)),
    ("33-8tips-K2", 33, 8, 70, dict(K=2)),
]


def reversible_problem(name):
    import helpers
    for nm, n, tips, patt, kw in REVERSIBLE_SHAPES:
        if nm == name:
            return helpers.random_problem(n, tips, patt, seed=200 + n + tips, **kw)
    raise KeyError(name)
