"""paml_amd_hessian: lnL, its gradient and its Hessian over all branch lengths in one engine call.
The reference (tests/test_hessian_cpu.py pins it on the CPU) is the numpy restatement (tests/hessian_ref.py) fed with the matrices
paml_amd_get_pmat returns, at the curvature tests' rtol 1e-9 / atol 1e-8.  lnL, grad and lnf are byte-equal to Engine.gradient's, the
diagonal to Engine.curvature's curv, hess to its transpose, a second call and a sub-list of nodes in another order to the first call."""
import ctypes as C

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import curvature_ref as cr
import gradient_ref as gr
import hessian_ref as hr
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


def _check(pb, eng=None, linear_floor=None):
    """One hessian call on pb against the restatement and the byte conditions; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.hessian(t.branch, pb.gene_rate, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL"] - base) <= 1e-10 * abs(base), (got["lnL"], base)
    H = got["hess"]
    assert H.shape == (t.n_nodes, t.n_nodes) and np.isfinite(H).all()
    plain = eng.gradient(t.branch, pb.gene_rate, want_lnf=True)
    assert _same_bytes(got["lnL"], plain["lnL"]) and _same_bytes(got["grad"], plain["grad"]) and _same_bytes(got["lnf"], plain["lnf"])
    assert _same_bytes(np.diag(H), eng.curvature(t.branch, pb.gene_rate)["curv"])
    assert _same_bytes(H, H.T)
    assert not H[t.root].any() and not H[:, t.root].any() and got["grad"][t.root] == 0
    again = eng.hessian(t.branch, pb.gene_rate, want_lnf=True)
    for key in ("lnL", "grad", "hess", "lnf"):
        assert _same_bytes(got[key], again[key]), key
    nodes = [v for v in range(t.n_nodes) if v != t.root][::-1][::2]      # a sub-list in another order
    sub = eng.hessian(t.branch, pb.gene_rate, nodes=nodes)
    assert sub["hess"].shape == (len(nodes), len(nodes)) and _same_bytes(sub["hess"], H[np.ix_(nodes, nodes)])
    assert _same_bytes(sub["grad"], got["grad"]) and _same_bytes(sub["lnL"], got["lnL"])
    rs = hr.hessian_of(pb, ar.matrices_from_engine(eng, pb))      # (the matrices of the call just made)
    if linear_floor is not None:
        assert rs["f"].min() > linear_floor, rs["f"].min()
    print("hess: max abs error %.3e (|H| max %.3e); grad: %.3e" % (float(np.max(np.abs(H - rs["hess"]))), float(np.max(np.abs(rs["hess"]))),
                                                                  float(np.max(np.abs(got["grad"] - rs["grad"])))))
    assert np.allclose(H, rs["hess"], **TOL)
    assert np.allclose(got["grad"], rs["grad"], **TOL)
    if t.n_nodes > 2:
        off = rs["hess"] - np.diag(np.diag(rs["hess"]))
        assert np.abs(off).max() > 1e-6      # (the cross terms are there to be compared)
    return eng, got


# 1 ---- the reversible shapes: every kernel family, K classes, ambiguity codes, genes, scaling nodes, a polytomy ------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_hessian_matches_the_restatement_on_reversible_models(name):
    _check(gr.reversible_problem(name))


@pytest.mark.parametrize("n", [64, 21])
def test_hessian_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_hessian_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 ---- models that are not reversible with respect to one pi ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (61, 2, 2)])
def test_hessian_with_eigen_systems_of_different_pi_per_label(n, K, genes):
    _check(_branch_model_problem(n, K, 300 + n + K, n_genes=genes))


@pytest.mark.parametrize("n", [4, 61])
def test_hessian_with_a_model_and_pi_per_gene(n):
    _check(helpers.give_genes_their_own_models(helpers.random_problem(n, 9, 150, K=2, seed=400 + n, n_genes=3), seed=n))


@pytest.mark.parametrize("n", [4, 61])
def test_hessian_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))))


# 3 ---- closed-form and Cijk kinds ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,kind", [(4, 2, "k80"), (20, 1, "jc")])
def test_hessian_of_the_closed_form_kinds(n, K, kind):
    _check(_closed_form(helpers.random_problem(n, 8, 50, K=K, seed=40 + n, ambiguity=(n == 4)), kind))


def test_hessian_of_the_cijk_kind_on_the_brown_golden():
    _check(helpers.problem_from_golden(helpers.load_golden("brown_hky85")))


# 4 ---- one pattern, one pattern past a tile ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [61, 4])
@pytest.mark.parametrize("patterns", [1, 65])
def test_hessian_of_one_pattern_and_of_one_past_a_tile(n, patterns):
    _check(helpers.random_problem(n, 9, patterns, K=2, seed=600 + n + patterns))


# 5 ---- the shapes of the plan: no path at all, the longest paths -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_hessian_of_the_three_tip_star(n):
    _check(hr.star_problem(n, 70, seed=3, K=2))


@pytest.mark.parametrize("n", [4, 61])
def test_hessian_of_the_caterpillar(n):
    _check(hr.caterpillar_problem(n, 7, 70, seed=5, K=2))


# 6 ---- deep trees: L' and A' rescaled by their largest magnitude ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tips,K,every", [(20, 40, 1, 8), (61, 30, 2, 5)])
def test_hessian_deep_tree_with_rescaling(n, tips, K, every):
    """The linear-domain restatement still holds on these: min f_h > 1e-250 is asserted before it is used."""
    _check(helpers.random_problem(n, tips, 70, K=K, seed=77 + n, scale_every=every), linear_floor=1e-250)


# 7 ---- batches and groups -----------------------------------------------------------------------------------------------------------------------

def test_hessian_batches_and_groups_have_the_same_bytes(monkeypatch):
    """PAML_AMD_HESS_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips: 64 patterns take 64 x 15208 bytes beside the rows, which
    leaves room for 72 of the 105 pairs — 47 batches and more than one group of sources; at 3 MiB two tiles per batch and one group.  Equal bytes."""
    c = cr.BATCHING_CASE
    pb = helpers.random_problem(c["n"], c["tips"], c["patterns"], K=c["K"], seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.hessian(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.hessian_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_HESS_ARENA_MB", "1")
    many = eng.hessian(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.hessian_info()["last_batches"] > 1
    for key in ("lnL", "grad", "hess", "lnf"):
        assert _same_bytes(one[key], many[key]), key
    monkeypatch.setenv("PAML_AMD_HESS_ARENA_MB", "3")
    some = eng.hessian(t.branch, pb.gene_rate)
    assert 1 < engine.hessian_info()["last_batches"]
    assert _same_bytes(one["hess"], some["hess"])


def test_hessian_groups_on_the_lane_kernels_have_the_same_bytes(monkeypatch):
    pb = helpers.random_problem(4, 9, 3000, K=3, seed=14, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.hessian(t.branch, pb.gene_rate)
    monkeypatch.setenv("PAML_AMD_HESS_ARENA_MB", "0.25")
    many = eng.hessian(t.branch, pb.gene_rate)
    assert engine.hessian_info()["last_batches"] > 1
    assert _same_bytes(one["hess"], many["hess"]) and _same_bytes(one["grad"], many["grad"])


# 8 ---- zero weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_patterns_of_weight_zero_contribute_nothing(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    full = engine_for(pb).hessian(t.branch, pb.gene_rate, want_lnf=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, got = _check(pb)
    live = pb.weights > 0
    assert got["lnf"][live].tobytes() == full["lnf"][live].tobytes()
    assert not np.allclose(got["hess"], full["hess"], **TOL)      # (the zeroed third did count before)


# 9 ---- arguments and state ---------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    import oracle
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    nn = t.n_nodes
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_hessian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    br, grad, hess, lnl = np.ascontiguousarray(t.branch), np.zeros(nn), np.zeros((nn, nn)), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(e, rc, code, text):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("hessian:") and text in msg, msg
    bad(eng, L.paml_amd_hessian(eng._h, None, None, None, 0, p(lnl), p(grad), p(hess), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_hessian(eng._h, p(br), None, None, 0, None, p(grad), p(hess), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_hessian(eng._h, p(br), None, None, 0, p(lnl), None, p(hess), None), EINVAL, "null argument")
    bad(eng, L.paml_amd_hessian(eng._h, p(br), None, None, 0, p(lnl), p(grad), None, None), EINVAL, "null argument")
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, L.paml_amd_hessian(fresh._h, p(br), None, None, 0, p(lnl), p(grad), p(hess), None), EINVAL, "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    for nodes, text in (([1, nn], "out of range"), ([-1, 2], "out of range"), ([1, t.root], "is the root"), ([1, 2, 1], "is repeated")):
        nl = np.array(nodes, dtype=np.int32)
        bad(eng, L.paml_amd_hessian(eng._h, p(br), None, p(nl), len(nl), p(lnl), p(grad), p(hess), None), EINVAL, text)
    bad(eng, L.paml_amd_hessian(eng._h, p(br), None, None, 2, p(lnl), p(grad), p(hess), None), EINVAL, "do not agree")
    assert not hess.any() and not grad.any() and lnl[0] == 0
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    with pytest.raises(engine.EngineError, match=r"hessian: .*rate-matrix \(UNREST\)"):
        engine_for(pq).hessian(pq.tree.branch)
    # want_lnf off; a list of one node; get_pmat afterwards returns the matrices the call used
    before_eval = eng.eval(t.branch, pb.gene_rate)["lnL"]
    plain = eng.hessian(t.branch, pb.gene_rate)
    assert plain["lnf"] is None
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    single = eng.hessian(t.branch, pb.gene_rate, nodes=[5])
    assert single["hess"].shape == (1, 1) and single["hess"][0, 0] == plain["hess"][5, 5]
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == before_eval
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    fresh_eb = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(fresh_eb, after))
    eng.hessian(t.branch, pb.gene_rate)
    info = engine.hessian_info()
    assert info["last_batches"] == 1 and info["last_kernel_ms"] > 0


def test_hessian_refuses_an_engine_of_two_ranks(tmp_path):
    """Two ranks on the one GPU through the shared-memory stand-in for the collective library, as tests/test_curvature_gpu.py: refused
    with PAML_AMD_EUNSUPPORTED and a message on every rank alike, nothing written, and the ranks stay in step."""
    import json
    import os
    import subprocess
    import sys
    from test_multirank_gpu import shim_env
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "hessian_rank_worker.py")
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
        assert res["msg"].startswith("hessian: one rank only") and "2" in res["msg"], res
        assert res["untouched"] and abs(float.fromhex(res["eval_after"]) - one) <= 1e-10 * abs(one), res
