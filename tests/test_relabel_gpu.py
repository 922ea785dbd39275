"""paml_amd_relabel_scores: the lnL, the per-pattern log likelihoods and the per-class values of the tree with one branch relabelled, for
every (non-root node, label) row in one engine call.  Reference: oracle.evaluate of the relabelled problem (relabel_ref.relabelled_problem;
tests/test_relabel_cpu.py pins the numpy restatement of the definition on it on the CPU).  Per row, on the patterns of weight > 0: lnf
within 1e-9 (the family's bound), hence |lnL - sum_h w_h lnf_ref| <= 1e-9 sum_h w_h; lnfk within 1e-9 of the logs of the oracle's class
values where those are finite; lnL0 against eval within 1e-10 |lnL|; eval keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import relabel_ref as rr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT
from test_ancestral_gpu import _rooted_at_tip0

pytestmark = pytest.mark.gpu


def _changed(pb, v, l):
    """[n_genes][K]: does label l on the branch above v change the class of the gene (its eigen set or its Qfactor)?"""
    now = int(pb.tree.label[v])
    return (pb.eigen_of[:, :, l] != pb.eigen_of[:, :, now]) | (pb.qfactor[:, l] != pb.qfactor[:, now])[None, :]


def _check(pb, eng=None):
    """One call for every (non-root node, label) of pb against the oracle on every relabelled tree; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.relabel_scores(t.branch, pb.gene_rate, want_lnf=True, want_classes=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert np.array_equal(got["rows"], rr.all_rows(t, pb.n_labels)) and len(got["rows"]) == (t.n_nodes - 1) * pb.n_labels
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    ref0 = oracle.evaluate(pb, want_fhk=True)
    rk0 = rr.oracle_class_logs(pb, ref0)
    fin0 = np.isfinite(rk0) & live[None, :]
    worst_k0 = float(np.max(np.abs(got["lnfk0"] - rk0)[fin0]))
    gene_of = np.repeat(np.arange(pb.n_genes), np.diff(pb.gene_off))
    worst_f, worst_l, worst_k, same = 0.0, 0.0, 0.0, 0
    for i, (v, l) in enumerate(got["rows"]):
        ref = oracle.evaluate(rr.relabelled_problem(pb, v, l), want_fhk=True)
        worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        worst_l = max(worst_l, abs(got["lnL"][i] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
        rk = rr.oracle_class_logs(pb, ref)
        fin = np.isfinite(rk) & live[None, :]
        worst_k = max(worst_k, float(np.max(np.abs(got["lnfk"][i] - rk)[fin])))
        ch = _changed(pb, v, l)[gene_of].T      # [K][n_patt]
        # a class that does not change has the present tree's bytes; a row in which none changes has them in lnf and lnL
        assert np.array_equal(got["lnfk"][i][~ch].view(np.uint64), got["lnfk0"][~ch].view(np.uint64)), (v, l)
        if not ch.any():
            same += 1
            assert np.float64(got["lnL"][i]).tobytes() == np.float64(got["lnL0"]).tobytes(), (v, l)
            assert got["lnf"][i].tobytes() == got["lnf"][int(np.flatnonzero((got["rows"][:, 0] == v) & (got["rows"][:, 1] == t.label[v]))[0])].tobytes()
    print("%d rows (%d with the present label or its model): lnf max abs error %.3e; lnL %.3e (allowed %.3e); lnfk %.3e, lnfk0 %.3e"
          % (len(got["rows"]), same, worst_f, worst_l, 1e-9 * wsum, worst_k, worst_k0))
    assert same >= t.n_nodes - 1
    assert worst_f <= 1e-9
    assert worst_l <= 1e-9 * wsum
    assert worst_k <= 1e-9 and worst_k0 <= 1e-9
    return eng, got


# 1 ---- the label problems of the CPU tests ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,genes", rr.LABEL_SHAPES)
def test_scores_match_the_oracle_on_every_relabelled_tree(n, K, genes):
    _check(rr.label_problem(n, K, genes))


@pytest.mark.parametrize("n", [64, 21])
def test_scores_at_the_ends_of_the_matrix_core_range(n):
    _check(rr.label_problem(n, 1, 1, seed=300 + n))


def test_scores_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split).
    (Measured: lnf 5.8e-12, lnfk 9.8e-10, the other shapes 3e-11 or below.  The numpy restatement on the oracle's matrices is within
    7e-15 of the oracle here, so the difference is in P(t) itself: a class that needs an entry of P' far below 1 carries that entry's
    absolute rounding error, 1e-16, as a relative one; the class has under 1 % of the pattern's likelihood, and lnf does not see it.)"""
    pb = rr.label_problem(20, 2, 1, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


@pytest.mark.parametrize("name", rr.REVERSIBLE_NAMES)
def test_scores_with_ambiguity_codes_a_polytomy_and_scaling_marks(name):
    _check(rr.labelled_reversible_problem(name))


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(rr.label_problem(n, 2, 1, seed=55 + (n == 61))))


def test_scores_on_a_deep_tree_with_rescaling():
    _check(rr.add_labels(helpers.random_problem(61, 30, 70, K=2, seed=77 + 61, scale_every=5), 78))


# 2 ---- classes that do not change, base labels ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_a_label_that_changes_one_class_leaves_the_other_its_bytes(n):
    """Label 1 differs from label 0 in class 1 only (the shape of branch-site model A's classes 0 and 1)."""
    pb = rr.label_problem(n, 2, 1, seed=88, n_labels=2)
    pb.tree.label[:] = 0
    pb.eigen_of = np.array([[[1, 1], [2, 3]]], dtype=np.int32)
    pb.qfactor = np.array([[0.8, 0.8], [1.1, 1.3]])
    eng, got = _check(pb)
    to1 = got["rows"][:, 1] == 1
    assert np.array_equal(got["lnfk"][to1][:, 0], np.broadcast_to(got["lnfk0"][0], got["lnfk"][to1][:, 0].shape))
    assert (np.abs(got["lnfk"][to1][:, 1] - got["lnfk0"][1]).max(axis=1) > 1e-6).all()


def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    for key in ("lnL", "lnf", "lnfk0", "lnfk"):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("n", [4, 61])
def test_base_labels_have_the_bytes_of_a_tree_set_with_them(n):
    pb = rr.label_problem(n, 2, 1, seed=91)
    t = pb.tree
    eng = engine_for(pb)
    before = eng.eval(t.branch, pb.gene_rate)["lnL"]
    other = np.ascontiguousarray((t.label + 1 + (np.arange(t.n_nodes) % 2)) % 3, dtype=np.int32)
    with_base = eng.relabel_scores(t.branch, pb.gene_rate, base_label=other, want_lnf=True, want_classes=True)
    # the tree's own labels and matrices are the engine's again
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == before
    q = rr.relabelled_problem(pb, 0, 0)
    q.tree.label[:] = other
    eng.set_tree(q.tree, q.scale_node)
    _same(with_base, eng.relabel_scores(t.branch, pb.gene_rate, want_lnf=True, want_classes=True))
    ref = oracle.evaluate(rr.relabelled_problem(q, 4, 2))
    i = int(np.flatnonzero((with_base["rows"][:, 0] == 4) & (with_base["rows"][:, 1] == 2))[0])
    assert np.max(np.abs(with_base["lnf"][i] - ref["lnf"])) <= 1e-9


# 3 ---- end to end: the engine on the relabelled tree -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (61, 2, 2)])
def test_eval_of_the_relabelled_tree_agrees(n, K, genes):
    pb = rr.label_problem(n, K, genes)
    t = pb.tree
    eng = engine_for(pb)
    got = eng.relabel_scores(t.branch, pb.gene_rate)
    inner = next(v for v in range(t.n_tips, t.n_nodes) if v != t.root)
    for v in (1, inner):
        l = (int(t.label[v]) + 1) % 3
        i = int(np.flatnonzero((got["rows"][:, 0] == v) & (got["rows"][:, 1] == l))[0])
        q = rr.relabelled_problem(pb, v, l)
        eng.set_tree(q.tree, q.scale_node)
        lnl = eng.eval(t.branch, pb.gene_rate)["lnL"]
        assert abs(lnl - got["lnL"][i]) <= 1e-10 * abs(lnl), (v, l, lnl, got["lnL"][i])
        assert abs(lnl - got["lnL0"]) > 1e-6 * abs(lnl)      # (and the label did move the likelihood)


# 4 ---- bytes ----------------------------------------------------------------------------------------------------------------------------------

def test_batches_groups_orders_and_calls_have_the_same_bytes(monkeypatch):
    """PAML_AMD_RELABEL_ARENA_MB=1 holds neither 3000 patterns of 61 states x 9 tips nor one tile with all 45 rows
    (test_relabel_cpu.py): several batches and several groups of rows, equal bytes; so a reversed list, a sub-list, a second call."""
    pb = rr.label_problem(61, 2, 1, seed=13, n_tips=9, n_patt=3000)
    t = pb.tree
    eng = engine_for(pb)
    kw = dict(want_lnf=True, want_classes=True)
    one = eng.relabel_scores(t.branch, pb.gene_rate, **kw)
    assert engine.relabel_info()["last_batches"] == 1 and engine.relabel_info()["last_kernel_ms"] > 0
    rows = one["rows"]
    assert len(rows) == 45
    monkeypatch.setenv("PAML_AMD_RELABEL_ARENA_MB", "1")
    many = eng.relabel_scores(t.branch, pb.gene_rate, **kw)
    assert engine.relabel_info()["last_batches"] > 1
    _same(one, many)
    _same(many, eng.relabel_scores(t.branch, pb.gene_rate, **kw))      # a second call
    rev = eng.relabel_scores(t.branch, pb.gene_rate, rows=rows[::-1], **kw)
    assert rev["lnL"][::-1].tobytes() == one["lnL"].tobytes() and rev["lnf"][::-1].tobytes() == one["lnf"].tobytes()
    assert rev["lnfk"][::-1].tobytes() == one["lnfk"].tobytes() and rev["lnfk0"].tobytes() == one["lnfk0"].tobytes()
    pick = [40, 5, 2, 2, 44, 17]
    monkeypatch.delenv("PAML_AMD_RELABEL_ARENA_MB")
    sub = eng.relabel_scores(t.branch, pb.gene_rate, rows=rows[pick], **kw)
    assert sub["lnL"].tobytes() == one["lnL"][pick].tobytes() and sub["lnf"].tobytes() == one["lnf"][pick].tobytes()
    assert sub["lnfk"].tobytes() == one["lnfk"][pick].tobytes()
    assert np.float64(sub["lnL0"]).tobytes() == np.float64(one["lnL0"]).tobytes() == np.float64(rev["lnL0"]).tobytes()
    plain = eng.relabel_scores(t.branch, pb.gene_rate)      # nothing per pattern asked for
    assert plain["lnf"] is None and plain["lnfk"] is None and plain["lnL"].tobytes() == one["lnL"].tobytes()
    v, l = (int(c) for c in rows[7])
    ref = oracle.evaluate(rr.relabelled_problem(pb, v, l))
    assert np.max(np.abs(one["lnf"][7] - ref["lnf"])) <= 1e-9


@pytest.mark.parametrize("n", [4, 20])
def test_groups_of_rows_on_the_lane_kernels_have_the_same_bytes(n, monkeypatch):
    """A workspace that one tile of patterns with all rows does not fit walks the rows in groups: a node's rows may fall into two."""
    pb = rr.label_problem(n, 2, 1, seed=600 + n)
    t = pb.tree
    eng = engine_for(pb, flags=engine.KEEP_PARTIALS if n == 20 else 0)
    kw = dict(want_lnf=True, want_classes=True)
    one = eng.relabel_scores(t.branch, pb.gene_rate, **kw)
    K, n_int = 2, t.n_nodes - t.n_tips
    fixed, per_row = 2 * K * n_int * (n + 1) * 8, (3 * K + 1) * 8
    mb = (fixed + 6.5 * per_row) * 64 / 1048576.0      # room for one tile with five rows and the present tree
    monkeypatch.setenv("PAML_AMD_RELABEL_ARENA_MB", "%.9f" % mb)
    _same(one, eng.relabel_scores(t.branch, pb.gene_rate, **kw))
    assert engine.relabel_info()["last_batches"] == 3      # (160 patterns in tiles of 64)


# 5 ---- arguments and state ---------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = rr.label_problem(4, 2, 1, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_relabel_scores.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6
    rows = rr.all_rows(t, 3)
    n = len(rows)
    br, lnl, lnl0, kk = np.ascontiguousarray(t.branch), np.zeros(n), np.zeros(1), np.zeros((n + 1, 2, pb.n_patt))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL, EUNSUPPORTED = -1, -4

    def bad(e, rc, text, code=EINVAL):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("relabel_scores") and text in msg, msg
    bad(eng, L.paml_amd_relabel_scores(eng._h, None, None, None, n, p(rows), p(lnl0), p(lnl), None, None, None), "null argument")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, n, None, p(lnl0), p(lnl), None, None, None), "null argument")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, n, p(rows), None, p(lnl), None, None, None), "null argument")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, n, p(rows), p(lnl0), None, None, None, None), "null argument")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, 0, p(rows), p(lnl0), p(lnl), None, None, None), "n_rows < 1")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, n, p(rows), p(lnl0), p(lnl), None, p(kk), None), "together")
    bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, n, p(rows), p(lnl0), p(lnl), None, None, p(kk)), "together")
    for row, text in [((t.root, 0), "is the root"), ((t.n_nodes, 0), "out of range"), ((-1, 0), "out of range"), ((1, 3), "label 3"), ((1, -1), "label -1")]:
        one = np.array([row], dtype=np.int32)
        bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, 1, p(one), p(lnl0), p(lnl), None, None, None), text)
        two = np.ascontiguousarray(np.vstack([rows[:1], one]), dtype=np.int32)      # (wherever it stands in the list)
        bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, None, 2, p(two), p(lnl0), p(lnl), None, None, None), "row 1")
    for v, wrong in ((2, 3), (t.n_nodes - 1, -1)):
        base = np.zeros(t.n_nodes, dtype=np.int32)
        base[v] = wrong
        bad(eng, L.paml_amd_relabel_scores(eng._h, p(br), None, p(base), n, p(rows), p(lnl0), p(lnl), None, None, None), "base_label of node %d" % v)
    assert not lnl.any() and not lnl0.any()
    fresh = engine.Engine(4, 10, 160)      # a model that is not set yet
    bad(fresh, L.paml_amd_relabel_scores(fresh._h, p(br), None, None, n, p(rows), p(lnl0), p(lnl), None, None, None),
        "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    # a rate-matrix (UNREST) set, as edge_scores
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    eq = engine_for(pq)
    one = np.array([[1, 0]], dtype=np.int32)
    bad(eq, L.paml_amd_relabel_scores(eq._h, p(np.ascontiguousarray(pq.tree.branch)), None, None, 1, p(one), p(lnl0), p(lnl), None, None, None), "UNREST", EUNSUPPORTED)
    # (more than 64 states cannot be reached through the ABI: paml_amd_create refuses n > 64; two ranks: tests/test_relabel_multirank_gpu.py)
    # get_pmat afterwards returns the tree's own matrices; the other whole-tree calls and eval_branch find their state
    nni_before = engine_for(pb).nni_scores(t.branch, pb.gene_rate)
    plain = eng.relabel_scores(t.branch, pb.gene_rate)
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    assert eng.nni_scores(t.branch, pb.gene_rate)["lnL"].tobytes() == nni_before["lnL"].tobytes()
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    before = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    eng.relabel_scores(t.branch, pb.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert plain["lnL"].shape == (n,)
