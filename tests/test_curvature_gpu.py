"""paml_amd_curvature: lnL, its derivative and its second derivative along every branch length in one engine call.
References (tests/test_curvature_cpu.py pins them on the CPU): everywhere the numpy restatement (tests/curvature_ref.py) fed with the
matrices paml_amd_get_pmat returns, at rtol 1e-9 / atol 1e-8 (test_eval_branch_matches_oracle's ddl tolerances); on exactly reversible
models also the oracle's branch-local d2lnL/dt2 at the same tolerances — on models with their own pi per branch label, per gene, or rooted
at a tip the restatement is the only reference, because the branch-local form re-roots the tree.  lnL against eval within 1e-10 |lnL|;
lnL and grad byte-equal to Engine.gradient on the same engine."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import ancestral_ref as ar
import curvature_ref as cr
import gradient_ref as gr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_oracle_golden import _closed_form

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-9, atol=1e-8)


def _same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _check(pb, eng=None, branch_oracle=True, restatement=True):
    """One curvature call on pb against its references; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.curvature(t.branch, pb.gene_rate, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL"] - base) <= 1e-10 * abs(base), (got["lnL"], base)
    plain = eng.gradient(t.branch, pb.gene_rate, want_lnf=True)
    assert _same_bytes(got["lnL"], plain["lnL"]) and _same_bytes(got["grad"], plain["grad"]) and _same_bytes(got["lnf"], plain["lnf"])
    assert got["grad"][t.root] == 0 and got["curv"][t.root] == 0
    if branch_oracle:
        worst = 0.0
        for b in range(t.n_nodes):
            if b != t.root:
                _, _, ddl = oracle.eval_branch(pb, b, np.array([t.branch[b]]))
                worst = max(worst, abs(got["curv"][b] - ddl[0]) / max(1.0, abs(ddl[0])))
                assert np.allclose(got["curv"][b], ddl[0], **TOL), (b, got["curv"][b], ddl[0])
        print("curv against the oracle's ddl: largest deviation relative to max(1, |ddl|) %.3e" % worst)
    if restatement:
        eng.curvature(t.branch, pb.gene_rate)
        rs = cr.curvature_of(pb, ar.matrices_from_engine(eng, pb))      # (the matrices of the call just made)
        print("curv: max abs error %.3e; grad: %.3e" % (float(np.max(np.abs(got["curv"] - rs["curv"]))), float(np.max(np.abs(got["grad"] - rs["grad"])))))
        assert np.allclose(got["curv"], rs["curv"], **TOL)
        assert np.allclose(got["grad"], rs["grad"], **TOL)
    return eng, got


# 1 ---- exactly reversible models: the oracle's second branch derivative and the restatement ----------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_curvature_matches_the_oracle_on_reversible_models(name):
    _check(gr.reversible_problem(name))


@pytest.mark.parametrize("n", [64, 21])
def test_curvature_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_curvature_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 - 4 ---- models the branch-local form cannot serve: the restatement only ---------------------------------------------------------------

@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (61, 2, 2)])
def test_curvature_with_eigen_systems_of_different_pi_per_label(n, K, genes):
    _check(_branch_model_problem(n, K, 300 + n + K, n_genes=genes), branch_oracle=False)


@pytest.mark.parametrize("n", [4, 61])
def test_curvature_with_a_model_and_pi_per_gene(n):
    pb = helpers.give_genes_their_own_models(helpers.random_problem(n, 9, 150, K=2, seed=400 + n, n_genes=3), seed=n)
    _check(pb, branch_oracle=False)


@pytest.mark.parametrize("n", [4, 61])
def test_curvature_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))), branch_oracle=False)


# 5 ---- closed-form and Cijk kinds (single-model, reversible) ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,kind", [(4, 2, "k80"), (20, 1, "jc")])
def test_curvature_of_the_closed_form_kinds(n, K, kind):
    _check(_closed_form(helpers.random_problem(n, 8, 50, K=K, seed=40 + n, ambiguity=(n == 4)), kind))


def test_curvature_of_the_cijk_kind_on_the_brown_golden():
    _check(helpers.problem_from_golden(helpers.load_golden("brown_hky85")))


# 6 ---- deep trees: the rescaled outer chain ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tips,K,every", [(20, 40, 1, 8), (61, 30, 2, 5)])
def test_curvature_deep_tree_with_rescaling(n, tips, K, every):
    _check(helpers.random_problem(n, tips, 70, K=K, seed=77 + n, scale_every=every), restatement=False)


# 7 ---- batches ------------------------------------------------------------------------------------------------------------------------------

def test_curvature_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_CURV_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips (test_curvature_cpu.py): several batches, equal bytes."""
    c = cr.BATCHING_CASE
    pb = helpers.random_problem(c["n"], c["tips"], c["patterns"], K=c["K"], seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.curvature(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.curvature_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_CURV_ARENA_MB", "1")
    many = eng.curvature(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.curvature_info()["last_batches"] > 1
    for key in ("lnL", "grad", "curv", "lnf"):
        assert _same_bytes(one[key], many[key]), key
    _, _, ddl = oracle.eval_branch(pb, 1, np.array([t.branch[1]]))
    assert np.allclose(one["curv"][1], ddl[0], **TOL)


# 8 ---- zero weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_patterns_of_weight_zero_contribute_nothing(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    full = engine_for(pb).curvature(t.branch, pb.gene_rate, want_lnf=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, got = _check(pb, branch_oracle=False)
    live = pb.weights > 0
    assert got["lnf"][live].tobytes() == full["lnf"][live].tobytes()
    assert not np.allclose(got["curv"], full["curv"], **TOL)      # (the zeroed third did count before)


# 9 ---- arguments and state ---------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_curvature.argtypes = [C.c_void_p] * 7
    br, grad, curv, lnl = np.ascontiguousarray(t.branch), np.zeros(t.n_nodes), np.zeros(t.n_nodes), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(e, rc, code, text):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("curvature:") and text in msg, msg
    bad(eng, L.paml_amd_curvature(eng._h, None, None, p(lnl), p(grad), p(curv), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_curvature(eng._h, p(br), None, None, p(grad), p(curv), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_curvature(eng._h, p(br), None, p(lnl), None, p(curv), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_curvature(eng._h, p(br), None, p(lnl), p(grad), None, None), EINVAL, "null argument")
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, L.paml_amd_curvature(fresh._h, p(br), None, p(lnl), p(grad), p(curv), None), EINVAL, "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    with pytest.raises(engine.EngineError, match=r"curvature: .*rate-matrix \(UNREST\)"):
        engine_for(pq).curvature(pq.tree.branch)
    # want_lnf off; a second call has the same bytes; get_pmat afterwards returns the matrices the call used
    before_eval = eng.eval(t.branch, pb.gene_rate)["lnL"]
    plain = eng.curvature(t.branch, pb.gene_rate)
    assert plain["lnf"] is None
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    a = eng.curvature(t.branch, pb.gene_rate, want_lnf=True)
    b = eng.curvature(t.branch, pb.gene_rate, want_lnf=True)
    for key in ("lnL", "grad", "curv"):
        assert _same_bytes(a[key], b[key]) and _same_bytes(a[key], plain[key]), key
    assert _same_bytes(a["lnf"], b["lnf"])
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == before_eval
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    fresh_eb = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(fresh_eb, after))
    eng.curvature(t.branch, pb.gene_rate)
    info = engine.curvature_info()
    assert info["last_batches"] == 1 and info["last_kernel_ms"] > 0


def test_curvature_refuses_an_engine_of_two_ranks(tmp_path):
    """Two ranks on the one GPU through the shared-memory stand-in for the collective library, as tests/test_gradient_multirank_gpu.py:
    refused with PAML_AMD_EUNSUPPORTED and a message on every rank alike, nothing written, and the ranks stay in step."""
    import json
    import os
    import subprocess
    import sys
    from test_multirank_gpu import shim_env
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "curvature_rank_worker.py")
    world = 2
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(tmp_path)], env=shim_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300)[0].decode())
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    pb = helpers.random_problem(4, 9, 2048, K=2, seed=21)
    one = float(engine_for(pb).eval(pb.tree.branch, pb.gene_rate)["lnL"])
    for r in range(world):
        res = json.load(open(tmp_path / ("out%d.json" % r)))
        assert res["rc"] == -4, res      # PAML_AMD_EUNSUPPORTED
        assert res["msg"].startswith("curvature: one rank only") and "2" in res["msg"], res
        assert res["untouched"] and abs(float.fromhex(res["eval_after"]) - one) <= 1e-10 * abs(one), res
