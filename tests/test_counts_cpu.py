"""CPU-side checks of the expected-substitution-count call's references and arithmetic (no GPU): the restatement's label integral (Van Loan:
one general-purpose matrix exponential, tests/counts_ref.py) against the kernel's spectral formula restated in numpy, the dwell identity,
the workspace arithmetic, and the per-lane bodies of kernels_counts.h under the host sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import counts_ref as cref
import curvature_ref as cr
import modelgrad_ref as mr
from paml_amd import engine

REPO = helpers.REPO
TAUS = (1e-6, 1e-3, 0.1, 1.0, 5.0)


@pytest.mark.parametrize("n,degenerate", [(4, False), (20, False), (61, False), (64, False), (4, True), (20, True), (61, True)])
def test_van_loan_against_the_spectral_form(n, degenerate):
    """Random reversible matrices of 4 .. 64 states and the fully degenerate JC-like spectra (every Psi off the first row and column on its
    tau e^{lambda tau} branch), tau from 1e-6 to 5, a random 0 / 1 mask, its complement and the identity as labels: 1e-12 absolute."""
    rng = np.random.default_rng(100 + n)
    A, U, lam, V = cref.random_reversible(n, rng, degenerate)
    assert np.allclose((U * lam[None, :]) @ V, A, atol=1e-12) and np.allclose(U @ V, np.eye(n), atol=1e-12)
    worst = 0.0
    for tau in TAUS:
        for M in cref.mask_labels(n, n):
            B = cref.label_rates(A, M, 1.7)
            worst = max(worst, float(np.max(np.abs(cref.van_loan(A, B, tau) - cref.spectral_integral(U, lam, V, B, tau)))))
    print("n = %d%s: largest absolute difference %.3e" % (n, " (JC-like)" if degenerate else "", worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [4, 20, 61])
def test_the_dwell_identity(n):
    """sum_a I_{E_aa} = tau P (with branch / tau = 1), each term the time spent in a; and with the generator itself in the place of B
    the integral is tau A P, because A commutes with its exponential."""
    from scipy.linalg import expm
    rng = np.random.default_rng(7 + n)
    A, U, lam, V = cref.random_reversible(n, rng)
    for tau in (1e-3, 0.4, 3.0):
        P = expm(A * tau)
        total = np.zeros((n, n))
        for a in range(n):
            E = np.zeros((n, n))
            E[a, a] = 1
            total += cref.van_loan(A, cref.label_rates(A, E, 1.0), tau)
        assert np.max(np.abs(total - tau * P)) <= 1e-12
        assert np.max(np.abs(cref.van_loan(A, A, tau) - tau * (A @ P))) <= 1e-12


def test_the_restatement_sums_to_the_branch_length_and_is_additive():
    """On a small problem with the oracle's matrices: the identity label gives branch[v] at every live pattern, the counts of M_1 + M_2
    are the sums of the counts, and lnL is the oracle's."""
    import oracle
    pb = mr.small_problem(4, tips=6)
    t = pb.tree
    P = ar.matrices_from_oracle(pb)
    labels = cref.mask_labels(4, 3)
    ref = cref.subst_counts_of(pb, P, labels)
    live = pb.weights > 0
    assert np.allclose(ref["site_counts"][2][:, live], np.where(np.arange(t.n_nodes) == t.root, 0.0, t.branch)[:, None], rtol=0, atol=1e-12)
    both = cref.subst_counts_of(pb, P, (labels[0] + labels[1])[None])
    assert np.allclose(both["counts"][0], ref["counts"][0] + ref["counts"][1], rtol=0, atol=1e-10)
    assert not ref["counts"][:, t.root].any() and not ref["site_counts"][:, :, ~live].any()
    want = oracle.evaluate(pb)["lnL"]
    assert abs(ref["lnL"] - want) <= 1e-10 * abs(want)


def test_counts_bytes_per_pattern_against_its_restatement():
    """engine.counts_bytes_per_pattern restates counts_bytes_per_pattern of kernels_counts.h (whose arithmetic is held here as text); one
    mebibyte cannot hold the batching case of the GPU test (curvature_ref.BATCHING_CASE: 61 states, 9 tips, 3000 patterns)."""
    for K, n_int, nn, ns, n_lab, nq in [(1, 7, 16, 64, 3, 15), (3, 7, 16, 4, 2, 5), (2, 5, 12, 20, 16, 11)]:
        assert engine.counts_bytes_per_pattern(K, n_int, nn, ns, n_lab, nq) == cref.counts_bytes_per_pattern(K, n_int, nn, ns, n_lab, nq)
    src = open(os.path.join(REPO, "paml_amd", "csrc", "kernels_counts.h")).read()
    assert "8.0 * (2.0 * K * n_int * (ns + 1) + (double)K * n_nodes * ns + 2.0 * K * n_nodes + (double)K * (ns + 2) + (2.0 + K) + (double)n_lab * n_query)" in src
    c = cr.BATCHING_CASE
    n_int, n_nodes = c["tips"] - 2, 2 * c["tips"] - 2
    per_patt = cref.counts_bytes_per_pattern(c["K"], n_int, n_nodes, 64, 3, n_nodes - 1)
    assert per_patt == 8 * (2 * 7 * 65 + 16 * 64 + 2 * 16 + 66 + 3 + 45) and c["patterns"] * per_patt > 1 << 20


def test_the_host_sanitizer_program_builds_and_passes():
    """tools/counts_host_check.cpp (the per-lane bodies with no HIP at all) under ASan + UBSan as a program of its own, on the cases of
    tools/counts_host_check.py, against the restatement."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "counts_host_check.py"), "--build"], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "all cases reproduce the restatement" in r.stdout
