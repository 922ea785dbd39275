"""paml_amd_nni_scores: the lnL and the per-pattern log likelihoods of every nearest-neighbour-interchange neighbour of the tree in one
engine call.  Reference: oracle.evaluate of the rearranged problem (nni_ref.swapped_problem; tests/test_nni_cpu.py pins the numpy
restatement of the definition on it on the CPU).  Per swap, on the patterns of weight > 0: lnf within 1e-9 (the gradient tests' bound
for lnf), hence |lnL - sum_h w_h lnf_ref| <= 1e-9 sum_h w_h; lnL0 against eval within 1e-10 |lnL|; eval keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import gradient_ref as gr
import nni_ref as nr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem

pytestmark = pytest.mark.gpu


def _check(pb, eng=None, scale_every=None):
    """One call for the canonical list of pb against the oracle on every rearranged tree; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert np.array_equal(got["swaps"], t.nni_swaps()) and len(got["swaps"]) >= 1
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    worst_f, worst_l = 0.0, 0.0
    for i, (v, s, x) in enumerate(got["swaps"]):
        ref = oracle.evaluate(nr.swapped_problem(pb, v, s, x, scale_every))
        worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        worst_l = max(worst_l, abs(got["lnL"][i] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
    print("%d swaps: lnf max abs error %.3e; lnL %.3e (allowed %.3e)" % (len(got["swaps"]), worst_f, worst_l, 1e-9 * wsum))
    assert worst_f <= 1e-9
    assert worst_l <= 1e-9 * wsum
    return eng, got


# 1 ---- the shapes of the gradient's parity tests -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_scores_match_the_oracle_on_every_rearranged_tree(name):
    _check(gr.reversible_problem(name), scale_every=nr.scale_every_of(name))


@pytest.mark.parametrize("n", [64, 21])
def test_scores_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_scores_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 ---- models that are not reversible with respect to the gene's pi ------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,seed,genes", [(4, 2, 306, 1), (61, 2, 363, 2)])
def test_scores_with_eigen_systems_of_different_pi_per_label(n, K, seed, genes):
    _check(_branch_model_problem(n, K, seed, n_genes=genes))


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))))


def _unrest_problem():
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    return pq


def test_scores_of_a_rate_matrix_set():
    """UNREST: only P(t) is used, which the evaluation's builder makes for every kind."""
    _check(_unrest_problem())


# 3 ---- a deep tree: the rescaled outer chain ---------------------------------------------------------------------------------------------------

def test_scores_on_a_deep_tree_with_rescaling():
    _check(helpers.random_problem(61, 30, 70, K=2, seed=77 + 61, scale_every=5), scale_every=5)


# 4 ---- end to end: the engine on the rearranged tree ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_eval_of_the_rearranged_tree_agrees(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    got = eng.nni_scores(t.branch, pb.gene_rate)
    tip_s = [i for i, (v, s, x) in enumerate(got["swaps"]) if s < t.n_tips]
    both_internal = [i for i, (v, s, x) in enumerate(got["swaps"]) if s >= t.n_tips and x >= t.n_tips]
    assert tip_s and both_internal
    for i in (tip_s[0], both_internal[0]):
        q = nr.swapped_problem(pb, *got["swaps"][i], nr.scale_every_of(name))
        eng.set_tree(q.tree, q.scale_node)
        lnl = eng.eval(t.branch, pb.gene_rate)["lnL"]
        assert abs(lnl - got["lnL"][i]) <= 1e-10 * abs(lnl), (i, lnl, got["lnL"][i])


# 5 ---- bytes ------------------------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    assert a["lnL"].tobytes() == b["lnL"].tobytes() and a["lnf"].tobytes() == b["lnf"].tobytes()


def test_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_NNI_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips with all swaps (test_nni_cpu.py): several batches, equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.nni_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_NNI_ARENA_MB", "1")
    many = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.nni_info()["last_batches"] > 1
    _same(one, many)
    ref = oracle.evaluate(nr.swapped_problem(pb, *one["swaps"][3]))
    assert np.max(np.abs(one["lnf"][3] - ref["lnf"])) <= 1e-9


@pytest.mark.parametrize("n", [4, 61])
def test_groups_of_swaps_have_the_same_bytes(n, monkeypatch):
    """A workspace that one tile of patterns with all swaps does not fit walks the swaps in groups."""
    pb = helpers.random_problem(n, 9, 150, K=2, seed=600 + n, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    K, n_int, ns = 2, t.n_nodes - t.n_tips, 64 if n == 61 else n
    fixed, per_row = 2 * K * n_int * (ns + 1) * 8, (2 * K + 1) * 8
    mb = (fixed + 5.5 * per_row) * 64 / 1048576.0      # room for one tile with four swaps and the present tree
    assert len(one["swaps"]) > 4
    monkeypatch.setenv("PAML_AMD_NNI_ARENA_MB", "%.9f" % mb)
    _same(one, eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True))
    assert engine.nni_info()["last_batches"] == 3      # (150 patterns in tiles of 64)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"])
def test_a_swap_has_the_same_bytes_wherever_it_stands(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    full = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    _same(full, eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True))      # a second call
    sw = full["swaps"]
    rev = eng.nni_scores(t.branch, pb.gene_rate, swaps=sw[::-1], want_lnf=True)
    assert rev["lnL"][::-1].tobytes() == full["lnL"].tobytes() and rev["lnf"][::-1].tobytes() == full["lnf"].tobytes()
    pick = [5, 2, 2, len(sw) - 1]
    sub = eng.nni_scores(t.branch, pb.gene_rate, swaps=sw[pick], want_lnf=True)
    assert sub["lnL"].tobytes() == full["lnL"][pick].tobytes() and sub["lnf"].tobytes() == full["lnf"][pick].tobytes()
    assert np.float64(sub["lnL0"]).tobytes() == np.float64(full["lnL0"]).tobytes() == np.float64(rev["lnL0"]).tobytes()


@pytest.mark.parametrize("n", [4, 61])
def test_live_patterns_keep_their_bytes_when_others_have_weight_zero(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    full = engine_for(pb).nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, got = _check(pb, scale_every=3)
    live = pb.weights > 0
    assert got["lnf"][:, live].tobytes() == full["lnf"][:, live].tobytes()
    assert np.isfinite(got["lnL"]).all()


# 6 ---- arguments and state -------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_nni_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    sw = t.nni_swaps()
    br, lnl, lnl0 = np.ascontiguousarray(t.branch), np.zeros(len(sw)), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(e, rc, text):
        assert rc == EINVAL, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("nni_scores") and text in msg, msg
    n = len(sw)
    bad(eng, L.paml_amd_nni_scores(eng._h, None, None, n, p(sw), p(lnl0), p(lnl), None), "null argument")
    bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, n, None, p(lnl0), p(lnl), None), "null argument")
    bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, n, p(sw), None, p(lnl), None), "null argument")
    bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, n, p(sw), p(lnl0), None, None), "null argument")
    bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, 0, p(sw), p(lnl0), p(lnl), None), "n_swaps < 1")
    f = t.father()
    v, s, x = (int(c) for c in sw[0])
    inner = next(u for u in range(t.n_tips, t.n_nodes) if u != t.root and u != v and f[u] != v and f[v] != u)
    for swap, text in [((0, s, x), "is a tip"), ((t.root, t.sons[t.root][0], x), "is the root"), ((t.n_nodes, s, x), "out of range"),
                       ((-1, s, x), "out of range"), ((v, t.sons[inner][0], x), "is not a son of %d" % v), ((v, s, v), "is not a son of the father"),
                       ((v, s, t.sons[inner][0]), "is not a son of the father"), ((v, s, t.n_nodes + 5), "is not a son of the father")]:
        one = np.array([swap], dtype=np.int32)
        bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, 1, p(one), p(lnl0), p(lnl), None), text)
        two = np.ascontiguousarray(np.vstack([sw[:1], one]), dtype=np.int32)      # (wherever it stands in the list)
        bad(eng, L.paml_amd_nni_scores(eng._h, p(br), None, 2, p(two), p(lnl0), p(lnl), None), "swap 1")
    assert not lnl.any() and not lnl0.any()
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, L.paml_amd_nni_scores(fresh._h, p(br), None, n, p(sw), p(lnl0), p(lnl), None), "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    # want_lnf off; get_pmat afterwards returns the matrices the call used
    plain = eng.nni_scores(t.branch, pb.gene_rate)
    assert plain["lnf"] is None and np.array_equal(plain["swaps"], sw)
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    a = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert a["lnL"].tobytes() == plain["lnL"].tobytes() and np.float64(a["lnL0"]).tobytes() == np.float64(plain["lnL0"]).tobytes()
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    before = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert engine.nni_info()["last_batches"] == 1 and engine.nni_info()["last_kernel_ms"] > 0
