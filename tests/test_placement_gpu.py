"""paml_amd_placement_scores: the lnL and the per-pattern log likelihoods of the tree with a query tip hung on a branch, for every query,
every branch and every pendant length in one engine call.  Reference: oracle.evaluate of the problem on the enlarged tree
(placement_ref.inserted_problem; tests/test_placement_cpu.py pins the numpy restatement of the definition on it on the CPU).  Per (query,
edge, pendant), on the patterns of weight > 0: lnf within 1e-9 (the NNI tests' bound for lnf), hence |lnL - sum_h w_h lnf_ref| <= 1e-9
sum_h w_h; lnL0 against eval within 1e-10 |lnL|; eval keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import gradient_ref as gr
import nni_ref as nr
import placement_ref as pr
from paml_amd import engine
from paml_amd.engine import engine_for
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_nni_gpu import _unrest_problem

pytestmark = pytest.mark.gpu

PHI, PENDANT = 0.3, (0.05, 0.4)


def _check(pb, eng=None, scale_every=None, queries=None, phi=PHI, pendant=PENDANT, label=0):
    """One call for every query, edge and pendant of pb against the oracle on every enlarged tree; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    queries = pr.queries_of(pb, seed=1) if queries is None else queries
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=pendant, phi=phi, pendant_label=label, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert list(got["edges"]) == [v for v in range(t.n_nodes) if v != t.root]
    assert got["lnL"].shape == (len(queries), t.n_nodes - 1, len(pendant))
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    worst_f, worst_l = 0.0, 0.0
    for qi in range(len(queries)):
        for i, v in enumerate(got["edges"]):
            for j, tau in enumerate(pendant):
                ref = oracle.evaluate(pr.inserted_problem(pb, v, phi, tau, queries[qi], label, scale_every))
                worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][qi, i, j] - ref["lnf"])[live])))
                worst_l = max(worst_l, abs(got["lnL"][qi, i, j] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
    print("%d x %d x %d placements: lnf max abs error %.3e; lnL %.3e (allowed %.3e)" % (got["lnL"].shape + (worst_f, worst_l, 1e-9 * wsum)))
    assert worst_f <= 1e-9
    assert worst_l <= 1e-9 * wsum
    return eng, got


# 1 ---- shapes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_scores_match_the_oracle_on_every_enlarged_tree(name):
    _check(gr.reversible_problem(name), scale_every=nr.scale_every_of(name))


@pytest.mark.parametrize("n", [64, 21])
def test_scores_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_scores_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 ---- eigen systems per label, roots, rate-matrix sets ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", [0, 1])
@pytest.mark.parametrize("n,K,seed,genes", [(4, 2, 306, 1), (61, 2, 363, 2)])
def test_scores_with_eigen_systems_of_different_pi_per_label(n, K, seed, genes, label):
    _check(_branch_model_problem(n, K, seed, n_genes=genes), label=label)


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))))


def test_scores_of_a_rate_matrix_set():
    """UNREST: only P(t) is used, which the evaluation's builder makes for every kind."""
    _check(_unrest_problem())


# 3 ---- a deep tree: the rescaled outer chain ---------------------------------------------------------------------------------------------------

def test_scores_on_a_deep_tree_with_rescaling():
    pb = helpers.random_problem(61, 30, 70, K=2, seed=77 + 61, scale_every=5)
    _check(pb, scale_every=5, queries=pr.queries_of(pb, seed=2)[:2], pendant=(0.2,))


# 4 ---- the ends of the range; invariants --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
@pytest.mark.parametrize("phi,pendant", [(0.0, (0.05, 0.4)), (1.0, (0.0, 0.4)), (0.3, (0.0, 0.4))])
def test_scores_at_the_ends_of_the_branch_and_a_pendant_of_zero(name, phi, pendant):
    """phi = 0 (the new node on the branch's lower node), phi = 1 (on its father) and a pendant of length 0 (the query is the new node's
    state).  phi = 0 together with a pendant of 0 is left to the invariants below: on a tip's branch the query is then the tip itself, and
    a query that differs from the tip where both are one state has likelihood exactly 0 — log 0 on both sides, nothing to compare."""
    _check(gr.reversible_problem(name), scale_every=nr.scale_every_of(name), phi=phi, pendant=pendant)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_a_query_without_data_and_a_copy_of_a_tip_change_nothing(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    lnf0 = eng.eval(t.branch, pb.gene_rate, want_lnf=True)["lnf"]
    live = pb.weights > 0
    missing = next(c for c in range(pb.n_codes) if pb.n_chara[c] == pb.n)
    for phi in (0.0, 0.3, 1.0):
        got = eng.placement_scores(t.branch, pb.gene_rate, queries=np.full((1, pb.n_patt), missing, dtype=np.uint8), pendant=(0.0, 0.7), phi=phi,
                                   want_lnf=True)
        assert np.max(np.abs(got["lnf"] - lnf0)[..., live]) <= 1e-9
    v = 2
    got = eng.placement_scores(t.branch, pb.gene_rate, queries=pb.z[v:v + 1], edges=[v], pendant=(0.0,), phi=0.0, want_lnf=True)
    assert np.max(np.abs(got["lnf"][0, 0, 0] - lnf0)[live]) <= 1e-9


# 5 ---- end to end: the engine on the enlarged tree ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_eval_of_the_enlarged_tree_agrees(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    queries = pr.queries_of(pb, seed=1)[1:2]
    got = engine_for(pb).placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI)
    for v in (1, t.n_tips + 2):      # a tip's edge and an internal edge
        assert v != t.root
        q = pr.inserted_problem(pb, v, PHI, PENDANT[1], queries[0], 0, nr.scale_every_of(name))
        lnl = engine_for(q).eval(q.tree.branch, q.gene_rate)["lnL"]
        mine = got["lnL"][0, list(got["edges"]).index(v), 1]
        assert abs(lnl - mine) <= 1e-10 * abs(lnl), (v, lnl, mine)


# 6 ---- bytes ------------------------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    assert a["lnL"].tobytes() == b["lnL"].tobytes() and a["lnf"].tobytes() == b["lnf"].tobytes()


def _byte_case(n_q, pendant):
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    rng = np.random.default_rng(5)
    queries = np.ascontiguousarray(np.vstack([pb.z[:1], rng.integers(0, pb.n, size=(n_q - 1, pb.n_patt))]), dtype=np.uint8)
    return pb, queries, engine_for(pb), dict(queries=queries, pendant=pendant, phi=PHI, want_lnf=True)


def test_batches_have_the_same_bytes(monkeypatch):
    """Case A.  PAML_AMD_PLACE_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips with the 90 rows of 3 queries x 15 edges x 2
    pendants, one tile of them fits (test_placement_cpu.py): several batches, equal bytes."""
    pb, queries, eng, kw = _byte_case(3, PENDANT)
    t = pb.tree
    one = eng.placement_scores(t.branch, pb.gene_rate, **kw)
    assert engine.placement_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_PLACE_ARENA_MB", "1")
    many = eng.placement_scores(t.branch, pb.gene_rate, **kw)
    assert engine.placement_info()["last_batches"] > 1
    _same(one, many)
    ref = oracle.evaluate(pr.inserted_problem(pb, one["edges"][3], PHI, PENDANT[1], queries[1]))
    assert np.max(np.abs(one["lnf"][1, 3, 1] - ref["lnf"])) <= 1e-9


def test_groups_of_edges_have_the_same_bytes(monkeypatch):
    """Case B.  8 queries x 15 edges x 4 pendants: at 1 MiB one tile with all 480 rows does not fit, one with an edge's 32 rows does
    (test_placement_cpu.py): the edges are walked in groups on the batch's partials and messages."""
    pb, queries, eng, kw = _byte_case(8, (0.0, 0.05, 0.4, 1.5))
    t = pb.tree
    one = eng.placement_scores(t.branch, pb.gene_rate, **kw)
    assert engine.placement_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_PLACE_ARENA_MB", "1")
    _same(one, eng.placement_scores(t.branch, pb.gene_rate, **kw))
    assert engine.placement_info()["last_batches"] == (3000 + 63) // 64      # (one tile per batch)


@pytest.mark.parametrize("n", [4, 61])
def test_groups_of_edges_on_a_tree_with_classes_and_scaling(n, monkeypatch):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=600 + n, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    kw = dict(queries=pr.queries_of(pb, seed=3), pendant=PENDANT, phi=PHI, want_lnf=True)
    one = eng.placement_scores(t.branch, pb.gene_rate, **kw)
    K, n_int, ns = 2, t.n_nodes - t.n_tips, 64 if n == 61 else n
    rows_edge = len(kw["queries"]) * 2
    fixed, per_edge = 2 * K * n_int * (ns + 1) * 8 + (2 * K + 1) * 8, (2 * K + 1) * 8 * rows_edge
    mb = (fixed + 4.5 * per_edge) * 64 / 1048576.0      # room for one tile with four edges' rows
    monkeypatch.setenv("PAML_AMD_PLACE_ARENA_MB", "%.9f" % mb)
    _same(one, eng.placement_scores(t.branch, pb.gene_rate, **kw))
    assert engine.placement_info()["last_batches"] == 3      # (150 patterns in tiles of 64)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"])
def test_an_element_has_the_same_bytes_wherever_it_stands(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb, seed=1)
    kw = dict(phi=PHI, want_lnf=True)
    full = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, **kw)
    _same(full, eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, **kw))      # a second call
    ed = full["edges"]
    rev = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, edges=ed[::-1], pendant=PENDANT, **kw)
    assert rev["lnL"][:, ::-1].tobytes() == full["lnL"].tobytes() and rev["lnf"][:, ::-1].tobytes() == full["lnf"].tobytes()
    pick = [5, 2, 2, len(ed) - 1]
    sub = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, edges=ed[pick], pendant=PENDANT, **kw)
    assert sub["lnL"].tobytes() == full["lnL"][:, pick].tobytes() and sub["lnf"].tobytes() == full["lnf"][:, pick].tobytes()
    one_q = eng.placement_scores(t.branch, pb.gene_rate, queries=queries[1:2], pendant=PENDANT, **kw)
    assert one_q["lnL"].tobytes() == full["lnL"][1:2].tobytes() and one_q["lnf"].tobytes() == full["lnf"][1:2].tobytes()
    one_p = eng.placement_scores(t.branch, pb.gene_rate, queries=queries[::-1], pendant=PENDANT[1:], **kw)
    assert one_p["lnL"].tobytes() == full["lnL"][::-1, :, 1:].tobytes() and one_p["lnf"].tobytes() == full["lnf"][::-1, :, 1:].tobytes()
    for other in (rev, sub, one_q, one_p):
        assert np.float64(other["lnL0"]).tobytes() == np.float64(full["lnL0"]).tobytes()


def test_more_pendants_than_the_tree_has_tips():
    """The pendant lengths' matrices are built a tree's worth of tips at a time: a longer list takes several runs of the builder."""
    pb = gr.reversible_problem("33-8tips-K2")
    t = pb.tree
    eng = engine_for(pb)
    pend = tuple(0.03 * (j + 1) for j in range(2 * t.n_tips + 1))
    queries = pr.queries_of(pb, seed=1)[:1]
    full = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, edges=[1, t.n_tips + 1], pendant=pend, phi=PHI, want_lnf=True)
    for j in (0, t.n_tips - 1, t.n_tips, 2 * t.n_tips):
        one = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, edges=[1, t.n_tips + 1], pendant=pend[j:j + 1], phi=PHI, want_lnf=True)
        assert one["lnf"].tobytes() == full["lnf"][:, :, j:j + 1].tobytes()
    ref = oracle.evaluate(pr.inserted_problem(pb, t.n_tips + 1, PHI, pend[-1], queries[0]))
    assert np.max(np.abs(full["lnf"][0, 1, -1] - ref["lnf"])) <= 1e-9


# 7 ---- arguments and state -------------------------------------------------------------------------------------------------------------------------

def test_argument_errors():
    pb = gr.reversible_problem("4-K3-amb-scale3-2genes")
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_placement_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    br = np.ascontiguousarray(t.branch)
    qz = np.ascontiguousarray(pb.z[:2])
    ed = np.array([v for v in range(t.n_nodes) if v != t.root], dtype=np.int32)
    pend = np.array([0.1, 0.2])
    lnl, lnl0 = np.zeros((2, len(ed), 2)), np.zeros(1)
    EINVAL = -1

    def call(e=eng, branch=br, n_q=2, q=qz, n_e=len(ed), edges=ed, n_p=2, pe=pend, phi=0.5, label=0, l0=lnl0, l=lnl):
        return L.paml_amd_placement_scores(e._h, p(branch), None, n_q, p(q), n_e, p(edges), n_p, p(pe), phi, label, p(l0), p(l), None)

    def bad(rc, text, e=eng):
        assert rc == EINVAL, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("placement_scores") and text in msg, msg
    for kw in (dict(branch=None), dict(q=None), dict(pe=None), dict(l0=None), dict(l=None)):
        bad(call(**kw), "null argument")
    bad(call(n_q=0), "n_q < 1")
    bad(call(n_e=0), "n_edges < 1")
    bad(call(n_p=0), "n_pend < 1")
    q2 = qz.copy()
    q2[1, 7] = pb.n_codes
    bad(call(q=q2), "character code %d >= n_codes" % pb.n_codes)
    for v, text in [(t.root, "is the root"), (t.n_nodes, "is out of range"), (-1, "is out of range")]:
        e2 = ed.copy()
        e2[3] = v
        bad(call(edges=e2), "edge 3: node %d %s" % (v, text))
    for phi in (-1e-9, 1.0 + 1e-9, float("nan")):
        bad(call(phi=phi), "outside [0, 1]")
    for tau in (-0.1, float("inf"), float("nan")):
        bad(call(pe=np.array([0.1, tau])), "pendant 1 is negative or not finite")
    for label in (-1, pb.n_labels):
        bad(call(label=label), "pendant_label = %d is outside" % label)
    bad(call(edges=None, n_e=3), "with a null list")
    assert not lnl.any() and not lnl0.any()
    fresh = engine.Engine(4, 9, 150)      # a model that is not set yet
    bad(call(e=fresh), "before set_tips/set_tree/set_pi/set_classes/set_eigen", fresh)
    # a code with an empty state set
    nch, cmap = pb.n_chara.copy(), pb.chara_map.copy()
    empty = pb.n_codes - 1
    z = np.where(pb.z == empty, 0, pb.z).astype(np.uint8)
    nch[empty] = 0
    e3 = engine_for(pb)
    e3.set_tips(z, pb.weights, 0, nch, cmap, pb.gene_off)
    q3 = qz.copy()
    q3[0, 5] = empty
    bad(call(e=e3, q=q3), "character code %d has an empty state set" % empty, e3)


def test_state_after_the_call():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb, seed=1)
    g0 = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    n0 = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    plain = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI)
    assert plain["lnf"] is None
    assert engine.placement_info()["last_batches"] == 1 and engine.placement_info()["last_kernel_ms"] > 0
    # get_pmat afterwards returns the tree's own matrices
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    g1 = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
    assert g1["lnL"] == g0["lnL"] and all(g1[k].tobytes() == g0[k].tobytes() for k in ("grad", "lnf", "scores"))
    eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI)
    n1 = eng.nni_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert n1["lnL0"] == n0["lnL0"] and n1["lnL"].tobytes() == n0["lnL"].tobytes() and n1["lnf"].tobytes() == n0["lnf"].tobytes()
    a = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=PENDANT, phi=PHI, want_lnf=True)
    assert a["lnL"].tobytes() == plain["lnL"].tobytes() and np.float64(a["lnL0"]).tobytes() == np.float64(plain["lnL0"]).tobytes()
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    before = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
