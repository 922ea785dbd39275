"""paml_amd_gradient: the derivative of lnL with respect to every branch length, and the per-pattern scores, in one engine call.
References (tests/test_gradient_cpu.py pins them on the CPU): on exactly reversible models the oracle's branch-local dlnL at rtol 1e-9 /
atol 1e-9 (test_eval_branch_matches_oracle's tolerances); everywhere the numpy restatement (tests/gradient_ref.py) fed with the matrices
paml_amd_get_pmat returns, at the same tolerances — on models with their own pi per branch label, per gene, or rooted at a tip it is the
only reference, because the branch-local form re-roots the tree.  lnf against the oracle at 1e-9, lnL against eval within 1e-10 |lnL|."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import ancestral_ref as ar
import gradient_ref as gr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_oracle_golden import _closed_form

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-9, atol=1e-9)


def _check(pb, eng=None, branch_oracle=True, restatement=True):
    """One gradient call on pb against its references; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL"] - base) <= 1e-10 * abs(base), (got["lnL"], base)
    ref = oracle.evaluate(pb)
    live = pb.weights > 0
    print("lnf: max abs error %.3e" % float(np.max(np.abs(got["lnf"] - ref["lnf"])[live])))
    assert np.max(np.abs(got["lnf"] - ref["lnf"])[live]) <= 1e-9
    assert got["grad"][t.root] == 0 and not got["scores"][t.root].any() and not got["scores"][:, ~live].any()
    if branch_oracle:
        for b in range(t.n_nodes):
            if b != t.root:
                _, dl, _ = oracle.eval_branch(pb, b, np.array([t.branch[b]]))
                assert np.allclose(got["grad"][b], dl[0], **TOL), (b, got["grad"][b], dl[0])
    if restatement:
        rs = gr.gradient_of(pb, ar.matrices_from_engine(eng, pb))      # (the matrices of the evaluation just made: the same kernels, the same arguments)
        print("scores: max abs error %.3e; grad: %.3e" % (float(np.max(np.abs(got["scores"] - rs["scores"]))), float(np.max(np.abs(got["grad"] - rs["grad"])))))
        assert np.allclose(got["scores"], rs["scores"], **TOL)
        assert np.allclose(got["grad"], rs["grad"], **TOL)
    return eng, got


# 1 ---- exactly reversible models: the oracle's branch derivative and the restatement ---------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_gradient_matches_the_oracle_on_reversible_models(name):
    _check(gr.reversible_problem(name))


@pytest.mark.parametrize("n", [64, 21])
def test_gradient_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_gradient_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 - 4 ---- models the branch-local form cannot serve: the restatement only ---------------------------------------------------------------

@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (20, 1, 1), (61, 2, 2)])
def test_gradient_with_eigen_systems_of_different_pi_per_label(n, K, genes):
    _check(_branch_model_problem(n, K, 300 + n + K, n_genes=genes), branch_oracle=False)


@pytest.mark.parametrize("n", [4, 61])
def test_gradient_with_a_model_and_pi_per_gene(n):
    pb = helpers.give_genes_their_own_models(helpers.random_problem(n, 9, 150, K=2, seed=400 + n, n_genes=3), seed=n)
    _check(pb, branch_oracle=False)


@pytest.mark.parametrize("n", [4, 61])
def test_gradient_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))), branch_oracle=False)


# 5 ---- closed-form and Cijk kinds (single-model, reversible) ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,kind", [(4, 2, "k80"), (20, 1, "jc")])
def test_gradient_of_the_closed_form_kinds(n, K, kind):
    _check(_closed_form(helpers.random_problem(n, 8, 50, K=K, seed=40 + n, ambiguity=(n == 4)), kind))


def test_gradient_of_the_cijk_kind_on_the_brown_golden():
    _check(helpers.problem_from_golden(helpers.load_golden("brown_hky85")))


# 6 ---- deep trees: the rescaled outer chain ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tips,K,every", [(20, 40, 1, 8), (61, 30, 2, 5)])
def test_gradient_deep_tree_with_rescaling(n, tips, K, every):
    _check(helpers.random_problem(n, tips, 70, K=K, seed=77 + n, scale_every=every), restatement=False)


# 7 ---- batches ------------------------------------------------------------------------------------------------------------------------------

def test_gradient_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_GRAD_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips (test_gradient_cpu.py): several batches, equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    assert engine.gradient_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_GRAD_ARENA_MB", "1")
    many = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    assert engine.gradient_info()["last_batches"] > 1
    assert np.float64(one["lnL"]).tobytes() == np.float64(many["lnL"]).tobytes()
    for key in ("grad", "lnf", "scores"):
        assert one[key].tobytes() == many[key].tobytes(), key
    _, dl, _ = oracle.eval_branch(pb, 1, np.array([t.branch[1]]))
    assert np.allclose(one["grad"][1], dl[0], **TOL)


# 8 ---- zero weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_patterns_of_weight_zero_contribute_nothing(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    full = engine_for(pb).gradient(t.branch, pb.gene_rate, want_scores=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, got = _check(pb, branch_oracle=False)
    live = pb.weights > 0
    assert not got["scores"][:, ~live].any()
    assert got["scores"][:, live].tobytes() == full["scores"][:, live].tobytes()


# 9 ---- arguments and state ---------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    br, grad, lnl = np.ascontiguousarray(t.branch), np.zeros(t.n_nodes), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(e, rc, code, text):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("gradient") and text in msg, msg
    bad(eng, L.paml_amd_gradient(eng._h, None, None, p(lnl), p(grad), None, None), EINVAL, "null argument")
    bad(eng, L.paml_amd_gradient(eng._h, p(br), None, None, p(grad), None, None), EINVAL, "null argument")
    bad(eng, L.paml_amd_gradient(eng._h, p(br), None, p(lnl), None, None, None), EINVAL, "null argument")
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, L.paml_amd_gradient(fresh._h, p(br), None, p(lnl), p(grad), None, None), EINVAL, "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    with pytest.raises(engine.EngineError, match=r"gradient: .*rate-matrix \(UNREST\)"):
        engine_for(pq).gradient(pq.tree.branch)
    # want_lnf / want_scores off; a second call has the same bytes; get_pmat afterwards returns the matrices the call used
    plain = eng.gradient(t.branch, pb.gene_rate)
    assert plain["lnf"] is None and plain["scores"] is None
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    a = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    b = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    assert np.float64(a["lnL"]).tobytes() == np.float64(b["lnL"]).tobytes() == np.float64(plain["lnL"]).tobytes()
    assert a["grad"].tobytes() == plain["grad"].tobytes()
    for key in ("grad", "lnf", "scores"):
        assert a[key].tobytes() == b[key].tobytes(), key
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    before = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert engine.gradient_info()["last_batches"] == 1 and engine.gradient_info()["last_kernel_ms"] > 0
