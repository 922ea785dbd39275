"""The yardstick of the curvature tests (tests/curvature_ref.py) pinned on the CPU, before any GPU run.  On exactly reversible models the
restatement's curv equals the oracle's branch-local d2lnL/dt2 at every branch to test_eval_branch_matches_oracle's ddl tolerances (rtol
1e-9, atol 1e-8), and its grad and lnL are gradient_ref's to the bit.  d2matrices is held against differences of dmatrices for all four
eigen kinds.  On models that are not reversible with respect to the gene's pi the branch-local form, which re-roots the tree, is no
reference: there curv[v] is held against differences of gradient_ref's own grad[v] in branch[v]."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import curvature_ref as cr
import gradient_ref as gr
import oracle
from test_gradient_cpu import _irreversible_cases
from test_oracle_golden import _closed_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracles_second_branch_derivative_on_reversible_models(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    P = ar.matrices_from_oracle(pb)
    got, plain = cr.curvature_of(pb, P), gr.gradient_of(pb, P)
    assert got["lnL"] == plain["lnL"] and got["grad"].tobytes() == plain["grad"].tobytes() and got["lnf"].tobytes() == plain["lnf"].tobytes()
    assert got["curv"][t.root] == 0
    worst = 0.0
    for b in range(t.n_nodes):
        if b == t.root:
            continue
        _, _, ddl = oracle.eval_branch(pb, b, np.array([t.branch[b]]))
        worst = max(worst, abs(got["curv"][b] - ddl[0]) / max(1.0, abs(ddl[0])))
        assert np.allclose(got["curv"][b], ddl[0], rtol=1e-9, atol=1e-8), (b, got["curv"][b], ddl[0])
    print("%s: largest deviation from the oracle's ddl, relative to max(1, |ddl|): %.3e" % (name, worst))


def _richardson(f, t, h):
    """The central difference of f at t with steps h and h / 2, extrapolated (error O(h^4))."""
    d1 = (f(t + h) - f(t - h)) / (2 * h)
    d2 = (f(t + h / 2) - f(t - h / 2)) / h
    return (4 * d2 - d1) / 3


def _kinds():
    return [("uvroot-61-K2", lambda: helpers.random_problem(61, 6, 10, K=2, seed=9)),
            ("cijk-brown", lambda: helpers.problem_from_golden(helpers.load_golden("brown_hky85"))),
            ("k80-4-K2", lambda: _closed_form(helpers.random_problem(4, 8, 50, K=2, seed=44, ambiguity=True), "k80")),
            ("jc-20", lambda: _closed_form(helpers.random_problem(20, 8, 50, K=1, seed=60), "jc"))]


@pytest.mark.parametrize("name", [k[0] for k in _kinds()])
def test_d2matrices_equal_differences_of_dmatrices(name):
    """Every branch moved together by +-1e-3 and +-5e-4 (each matrix depends on its own branch only), Richardson pair.  The
    extrapolated difference's own error: truncation h^4 |d5P| / 30 ~ 1e-13 at these rates, rounding ~ 1e-16 |dP| / h ~ 1e-12.  Measured
    here, relative to max(1, |d2P|) over all entries: 1.1e-12 (uvroot), 2.1e-13 (cijk), 2.6e-13 (k80), 9.2e-14 (jc).  Allowance 1e-9; a
    formula that dropped a factor mu_k would be off by the order of d2P itself."""
    pb = dict(_kinds())[name]()
    br = np.asarray(pb.tree.branch, dtype=np.float64)
    assert br[[v for v in range(pb.tree.n_nodes) if v != pb.tree.root]].min() >= 0.005
    fd = _richardson(lambda s: gr.dmatrices(pb, br + s), 0.0, 1e-3)
    got = cr.d2matrices(pb)
    dev = float(np.max(np.abs(got - fd) / np.maximum(1.0, np.abs(got))))
    print("%s: largest deviation of d2matrices from differences of dmatrices %.3e" % (name, dev))
    assert got.any() and dev <= 1e-9


def _grad_at(pb, P, b, tb):
    """gradient_ref's grad[b] with branch b at length tb (P(t) of that branch from the oracle, every other matrix as it is)."""
    q = copy.copy(pb)
    q.tree = copy.copy(pb.tree)
    q.tree.branch = np.array(pb.tree.branch, dtype=np.float64)
    q.tree.branch[b] = tb
    Pq = P.copy()
    for g in range(pb.n_genes):
        for k in range(pb.K):
            Pq[g, k, b] = oracle.pmat_branch(q, g, k, b)
    return gr.gradient_of(q, Pq)["grad"][b]


@pytest.mark.parametrize("name", [c[0] for c in _irreversible_cases()] + ["genes-4-K2", "genes-61-K2"])
def test_restatement_equals_differences_of_the_gradient_on_irreversible_models(name):
    """curv[v] against the central difference (steps 1e-4 and 5e-5, Richardson pair: at 2e-3 the h^4 truncation still showed, 7e-5) of
    gradient_ref's own grad[v] in branch[v], every branch >= 0.01; the deviation relative to max(1, |curv|), |curv| up to 1.7e5.  Measured
    here with the oracle's matrices: 2.6e-12 (labels, 4 states), 4.0e-11 (labels, 61 states, two genes), 1.1e-11 and 8.0e-10 (the
    tip-rooted trees at 4 and 61 states), 4.4e-10 and 1.2e-11 (a model per gene at 4 and 61 states).  Allowance 8e-9: ten times the
    largest of them."""
    cases = dict(_irreversible_cases())
    cases["genes-4-K2"] = lambda: helpers.give_genes_their_own_models(helpers.random_problem(4, 9, 150, K=2, seed=404, n_genes=3), seed=4)
    cases["genes-61-K2"] = lambda: helpers.give_genes_their_own_models(helpers.random_problem(61, 9, 150, K=2, seed=461, n_genes=3), seed=61)
    pb = cases[name]()
    t = pb.tree
    P = ar.matrices_from_oracle(pb)
    got = cr.curvature_of(pb, P)
    assert got["grad"].tobytes() == gr.gradient_of(pb, P)["grad"].tobytes()
    dev = 0.0
    for b in range(t.n_nodes):
        if b == t.root:
            continue
        assert t.branch[b] >= 0.01
        fd = _richardson(lambda tb: _grad_at(pb, P, b, tb), float(t.branch[b]), 1e-4)
        dev = max(dev, abs(got["curv"][b] - fd) / max(1.0, abs(got["curv"][b])))
    print("%s: largest deviation from differences of the gradient %.3e" % (name, dev))
    assert dev <= 8e-9


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, one class, at the bytes a pattern takes in the workspace
    (curvature_ref.bytes_per_pattern, the arithmetic of curv_bytes_per_pattern in kernels_curvature.h)."""
    c = cr.BATCHING_CASE
    n_int, n_nodes = c["tips"] - 2, 2 * c["tips"] - 2      # (an unrooted binary tree of 9 tips has 7 internal nodes)
    per_patt = cr.bytes_per_pattern(c["K"], n_int, n_nodes, 64)
    assert per_patt == 2 * 7 * 65 * 8 + 4 * 16 * 8 + 8 and c["patterns"] * per_patt > 1 << 20
    src = open(os.path.join(REPO, "paml_amd", "csrc", "kernels_curvature.h")).read()
    assert "2.0 * K * n_int * (n_s + 1) * 8 + 4.0 * K * n_nodes * 8 + 8.0" in src


def test_the_host_sanitizer_program_builds_and_passes():
    """tools/curvature_host_check.cpp (the per-lane bodies with no HIP at all) under ASan + UBSan as a program of its own, on the cases of
    tools/curvature_host_check.py, against the restatement."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "curvature_host_check.py"), "--build"], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "all cases reproduce the restatement" in r.stdout
