"""The yardstick of the model-gradient tests (tests/modelgrad_ref.py) pinned on the CPU, before any GPU run: it agrees with itself (the
identities of the weighted outer products W), with gradient_ref, with the oracle's matrices (A is the matrix whose exponential the engine
takes), and with Richardson-extrapolated central differences of the CPU oracle's lnL along one parameter of each kind of input."""
import copy

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import gradient_ref as gr
import modelgrad_ref as mr
import oracle
from paml_amd import models
from paml_amd.problem import EIGEN_UVROOT
from test_ancestral_gpu import _rooted_at_tip0
from test_oracle_golden import _closed_form

RTOL = 1e-9


def _cases():
    return [("4-K2-2genes", lambda: mr.small_problem(4, tips=9, n_genes=2)),
            ("5-K1-scale", lambda: mr.small_problem(5, tips=6, K=1, scale_every=3)),
            ("20-K2", lambda: mr.small_problem(20)),
            ("61-K2-polytomy", lambda: mr.small_problem(61, tips=8, polytomy=True)),
            ("4-K2-tiproot", lambda: _rooted_at_tip0(mr.small_problem(4, tips=9, seed=1))),
            ("4-K2-k80", lambda: _closed_form(mr.small_problem(4, tips=8, seed=2), "k80")),
            ("20-K1-jc", lambda: _closed_form(mr.small_problem(20, tips=8, K=1, seed=3, ambiguity=False), "jc")),
            ("4-cijk-brown", lambda: helpers.problem_from_golden(helpers.load_golden("brown_hky85")))]


@pytest.fixture(scope="module", params=[c[0] for c in _cases()])
def case(request):
    pb = dict(_cases())[request.param]()
    P = ar.matrices_from_oracle(pb)
    return pb, P, mr.model_gradient_of(pb, P)


def test_pairs_times_P_give_the_weights_at_every_branch(case):
    """sum_k sum_{y,x} W o P = sum_{h in g} w_h at every non-root v: f_h = sum_k freqK_k sum H P L there."""
    pb, P, ref = case
    t = pb.tree
    for g in range(pb.n_genes):
        want = pb.weights[int(pb.gene_off[g]):int(pb.gene_off[g + 1])].sum()
        for v in range(t.n_nodes):
            if v != t.root:
                got = sum(np.sum(ref["W"][g, k, v] * P[g, k, v]) for k in range(pb.K))
                assert abs(got - want) <= RTOL * want, (g, v, got, want)


def test_pairs_times_dP_and_g_eff_give_the_branch_gradient(case):
    pb, P, ref = case
    grad = gr.gradient_of(pb, P)
    dP = gr.dmatrices(pb)
    _, base = mr.eff_lengths(pb)
    scale = np.max(np.abs(grad["grad"]))
    assert np.max(np.abs(np.einsum("gkvyx,gkvyx->v", ref["W"], dP) - grad["grad"])) <= RTOL * scale
    assert np.max(np.abs((ref["g_eff"] * base).sum(axis=(0, 1)) - grad["grad"])) <= RTOL * scale
    assert abs(ref["lnL"] - grad["lnL"]) <= 1e-12 * abs(grad["lnL"])
    assert abs(np.dot(ref["g_freqK"], pb.freqK) - pb.weights.sum()) <= RTOL * pb.weights.sum()


def test_the_rate_matrix_is_the_one_the_oracle_exponentiates(case):
    from scipy.linalg import expm
    pb, P, _ = case
    tau, _ = mr.eff_lengths(pb)
    t = pb.tree
    for g in range(pb.n_genes):
        for k in range(pb.K):
            for v in range(t.n_nodes):
                if v != t.root:
                    A = mr.rate_matrix(pb.eigen[int(pb.eigen_of[g, k, int(t.label[v])])], pb.n)
                    assert np.max(np.abs(expm(A * tau[g, k, v]) - P[g, k, v])) <= 1e-12


@pytest.mark.parametrize("n", [4, 5])
def test_the_adjoint_route_equals_one_basis_element_at_a_time(n):
    pb = mr.small_problem(n, tips=5, K=1)
    A = mr.rate_matrix(pb.eigen[0], n)
    W = np.random.default_rng(n).uniform(0, 1, size=(n, n))
    a, b = mr.frechet_adjoint(A * 0.3, W), mr.frechet_by_basis(A * 0.3, W)
    assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b))


# ---- finite differences of the oracle -------------------------------------------------------------------------------------------------

def _richardson(f, h):
    """(R, bound): the Richardson extrapolation of the central differences of f at h and h / 2, and the issue's bound on what a
    derivative may differ from it: 10 |D(h) - D(h/2)| (the differences' own truncation estimate) + 1e-12 |lnL| / h (the rounding of a
    difference quotient of a sum evaluated to ~1e-12 relative)."""
    D = lambda s: (f(s) - f(-s)) / (2 * s)
    d1, d2 = D(h), D(h / 2)
    return (4 * d2 - d1) / 3, 10 * abs(d1 - d2) + 1e-12 * abs(f(0.0)) / h


def _codon_problem():
    pb = mr.small_problem(61, tips=6, seed=5)
    return _with_kappa(pb, 2.0)


def _with_kappa(pb, kappa):
    q = copy.copy(pb)
    if pb.n == 61:
        U, V, root, _ = models.codon_m0_eigen(kappa, 0.4, pb.pi[0])
    else:
        U, V, root = models.eigen_rev(models.hky_q(kappa, pb.pi[0]), pb.pi[0])
    q.eigen = [dict(kind=EIGEN_UVROOT, U=U, V=V, Root=root)]
    return q


def _lnL(pb):
    return oracle.evaluate(pb)["lnL"]


FD_DEVIATIONS = {}


def _check_fd(name, got, f, h):
    R, bound = _richardson(f, h)
    FD_DEVIATIONS[name] = (abs(got - R), bound)
    print("%s: chain rule %.12g, Richardson %.12g, deviation %.3e, bound %.3e" % (name, got, R, abs(got - R), bound))
    assert abs(got - R) <= bound


@pytest.mark.parametrize("n", [4, 61])
def test_kappa_step_of_an_hky_and_a_codon_model(n):
    """<g_A, dA / d kappa> against the oracle's lnL; dA / d kappa by central differences of A itself, built without a decomposition (a
    rational function of kappa with O(1) derivatives: step 1e-4 leaves a truncation near 1e-8 of A''' and a rounding near 1e-12)."""
    pb = _with_kappa(mr.small_problem(n, tips=6, seed=5), 2.0)
    ref = mr.model_gradient_of(pb, ar.matrices_from_oracle(pb))

    def A(kappa):
        if n == 4:
            return models.hky_q(kappa, pb.pi[0])
        Q, mean_rate = models.codon_q(kappa, 0.4, pb.pi[0])
        return Q / mean_rate
    assert np.max(np.abs(A(2.0) - mr.rate_matrix(pb.eigen[0], n))) <= 1e-12
    dA = (A(2.0 + 1e-4) - A(2.0 - 1e-4)) / 2e-4
    _check_fd("kappa-%d" % n, float(np.sum(ref["g_A"][0] * dA)), lambda s: _lnL(_with_kappa(pb, 2.0 + s)), 1e-3)


def test_steps_of_a_class_rate_freqK_and_the_root_frequencies():
    pb = mr.small_problem(20, tips=6, seed=6)
    ref = mr.model_gradient_of(pb, ar.matrices_from_oracle(pb))

    def moved(field, idx, s):
        q = copy.copy(pb)
        a = np.array(getattr(pb, field), dtype=np.float64, copy=True)
        a[idx] += s
        setattr(q, field, a)
        return q
    # d tau / d rate[1] = branch x gene rate x qfactor
    dtau = pb.tree.branch * pb.gene_rate[0] * pb.qfactor[1, 0]
    _check_fd("rate", float(np.dot(ref["g_eff"][0, 1], dtau)), lambda s: _lnL(moved("rate", 1, s)), 1e-3)
    _check_fd("freqK", float(ref["g_freqK"][0]), lambda s: _lnL(moved("freqK", 0, s)), 1e-3)
    _check_fd("pi", float(ref["g_pi"][0, 2]), lambda s: _lnL(moved("pi", (0, 2), s)), 1e-4)
