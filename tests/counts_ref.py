"""numpy + scipy restatement of paml_amd_subst_counts: posterior expected labelled substitution counts and dwell times per branch and per
pattern, from the definition at the top of paml_amd/csrc/kernels_counts.h, on gradient_ref.py's down and outer loops.  Inputs are the
per-branch matrices P[gene][class][node] as in gradient_ref.py / modelgrad_ref.py.

  B_l = A o M_l off the diagonal, (B_l)_aa = M_l[a][a] branch[v] / tau;   I_lkv = int_0^tau e^{Au} B_l e^{A(tau - u)} du
  c_lvk(h) = sum_y H_v(y) (I_lkv L_v)(y);   n_lv(h) = sum_k freqK_k c_lvk / sum_k freqK_k f_hk;   counts[l][v] = sum_h w_h n_lv(h)

I_lkv does NOT come from the divided differences of the eigenvalues the kernel uses: it is the upper right block of
scipy.linalg.expm([[A, B_l], [0, A]] tau) (Van Loan 1978), a general-purpose matrix exponential, so that the reference shares no formula
with the kernel.  A comes from the problem's eigen sets (modelgrad_ref.rate_matrix).  spectral_integral is the kernel's formula in numpy;
tests/test_counts_cpu.py holds the two against each other (they agree to 2e-15 absolute on random reversible matrices of 4 .. 64 states,
tau from 1e-6 to 5, and on fully degenerate JC-like spectra: six orders under the tolerance of the GPU tests).
Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import numpy as np
from scipy.linalg import expm

from ancestral_ref import _father, _indicator, _postorder, tips_of      # noqa: F401
from modelgrad_ref import eff_lengths, rate_matrix

PSI_SERIES = 1e-4      # MODELGRAD_PSI_SERIES


def label_rates(A, M, branch_over_tau):
    """B_l: the labelled part of the generator (off the diagonal) and the rewards (on it)."""
    B = A * M
    B[np.diag_indices(len(A))] = np.diag(M) * branch_over_tau
    return B


def van_loan(A, B, tau):
    """int_0^tau e^{Au} B e^{A(tau - u)} du as the upper right block of one matrix exponential."""
    n = len(A)
    if tau == 0:
        return np.zeros((n, n))
    X = np.zeros((2 * n, 2 * n))
    X[:n, :n] = A
    X[n:, n:] = A
    X[:n, n:] = B
    return expm(X * tau)[:n, n:]


def psi(lam, tau):
    """Psi_rs of the eigenvalues `lam` at tau, as mg_psi: from the larger of the two, phi(d) = expm1(d) / d by its series below PSI_SERIES."""
    hi = np.maximum(lam[:, None], lam[None, :])
    d = (np.minimum(lam[:, None], lam[None, :]) - hi) * tau
    small = np.abs(d) < PSI_SERIES
    safe = np.where(small, 1.0, d)
    phi = np.where(small, 1 + d * (0.5 + d * (1.0 / 6 + d * (1.0 / 24))), np.expm1(safe) / safe)
    return tau * np.exp(hi * tau) * phi


def spectral_integral(U, lam, V, B, tau):
    """The same integral by the spectral formula of the kernel: U (Psi o (V B U)) V with A = U diag(lam) V."""
    return U @ (psi(np.asarray(lam, dtype=np.float64), tau) * (V @ B @ U)) @ V


def random_reversible(n, rng, degenerate=False):
    """(A, U, lam, V) of a random reversible rate matrix with mean rate 1 (degenerate: the JC-like one, n - 1 equal eigenvalues)."""
    pi = np.full(n, 1.0 / n) if degenerate else rng.dirichlet(np.full(n, 5.0))
    S = np.ones((n, n)) if degenerate else rng.uniform(0.2, 2.0, (n, n))
    S = (S + S.T) / 2
    A = S * pi[None, :]
    A[np.diag_indices(n)] = 0
    A[np.diag_indices(n)] = -A.sum(axis=1)
    A /= -np.dot(pi, np.diag(A))
    sq = np.sqrt(pi)
    lam, R = np.linalg.eigh((sq[:, None] * A) / sq[None, :])
    return A, R / sq[:, None], lam, R.T * sq[None, :]


def label_integrals(pb, labels, branch=None, gene_rate=None):
    """I[g][k][v][l] (the root's entries 0) by Van Loan."""
    n, t = pb.n, pb.tree
    labels = np.asarray(labels, dtype=np.float64).reshape(-1, n, n)
    branch = t.branch if branch is None else np.asarray(branch, dtype=np.float64)
    tau, _ = eff_lengths(pb, branch, gene_rate)
    A = [rate_matrix(es, n) for es in pb.eigen]
    out = np.zeros((pb.n_genes, pb.K, t.n_nodes, len(labels), n, n))
    for g in range(pb.n_genes):
        for k in range(pb.K):
            for v in range(t.n_nodes):
                if v == t.root or tau[g, k, v] == 0:
                    continue
                As = A[int(pb.eigen_of[g, k, int(t.label[v])])]
                for l, M in enumerate(labels):
                    out[g, k, v, l] = van_loan(As, label_rates(As, M, branch[v] / tau[g, k, v]), tau[g, k, v])
    return out


def subst_counts(P, I, pi, freqK, tips, tree, weights):
    """dict(lnL, lnf [n_patt], counts [n_lab][n_nodes], site_counts [n_lab][n_nodes][n_patt]) of the definition above."""
    z, sets, gene_off = tips
    n, nt, nn, root = P.shape[-1], tree.n_tips, tree.n_nodes, tree.root
    n_lab = I.shape[3]
    father, post = _father(tree), _postorder(tree)
    weights = np.asarray(weights, dtype=np.float64)
    pi = np.atleast_2d(pi)
    lnf = np.zeros(z.shape[1])
    site = np.zeros((n_lab, nn, z.shape[1]))
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        m = hi - lo
        f, c = np.zeros(m), np.zeros((n_lab, nn, m))
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
            for v in reversed(post):                         # outer + the labels' products
                if v == root:
                    continue
                H = A[father[v]].copy()
                for s in tree.sons[father[v]]:
                    if s != v:
                        H = H * M[s]
                for l in range(n_lab):
                    c[l, v] += freqK[k] * (H * (L[v] @ I[g, k, v, l].T)).sum(axis=1)
                A[v] = H @ P[g, k, v]
        lnf[lo:hi] = np.log(f)
        site[:, :, lo:hi] = c / f[None, None, :]
    site[:, :, weights == 0] = 0
    live = weights != 0
    return dict(lnL=float(np.dot(weights[live], lnf[live])), lnf=lnf, counts=site @ weights, site_counts=site)


def subst_counts_of(pb, P, labels, branch=None, gene_rate=None):
    """The restatement on a Problem, its matrices P (matrices_from_oracle / matrices_from_engine) and the labels [n_lab][n][n]."""
    return subst_counts(P, label_integrals(pb, labels, branch, gene_rate), pb.pi, pb.freqK, tips_of(pb), pb.tree, pb.weights)


def mask_labels(n, seed):
    """The labels of the parity tests: a random 0 / 1 mask off the diagonal, its complement, and the identity (the dwell time)."""
    rng = np.random.default_rng(seed)
    mask = (rng.random((n, n)) < 0.5).astype(np.float64)
    mask[np.diag_indices(n)] = 0
    comp = 1.0 - mask
    comp[np.diag_indices(n)] = 0
    return np.stack([mask, comp, np.eye(n)])


def counts_bytes_per_pattern(K, n_int, n_nodes, ns, n_lab, n_query):
    """Restated from kernels_counts.h: doubles per pattern of the batch workspace, times 8."""
    partials = 2 * K * n_int * (ns + 1)      # L and G with their log factors
    outer = K * n_nodes * ns                 # H of every node
    sums = 2 * K * n_nodes                   # f_vk and sigma_vk
    tip_root = K * (ns + 2)                  # a tip root's partial, its log factor, its coefficient
    scalars = 2 + K                          # lnf and the scalar rows
    return 8.0 * (partials + outer + sums + tip_root + scalars + n_lab * n_query)
