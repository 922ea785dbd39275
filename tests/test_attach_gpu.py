"""paml_amd_attach_scores: the lnL of the tree with a query tip hung on a branch at the row's own lengths of the three branches around the
new node, with the first and second derivative along one of them, for many rows in one engine call.  Reference: oracle.evaluate of the
enlarged problem with the three lengths written into its tree (attach_ref.attached_problem) and oracle.eval_branch on it at the role's
node; on models that are not reversible with respect to the gene's pi the numpy restatement (tests/attach_ref.py, which
tests/test_attach_cpu.py pins on the oracle and on central differences on the CPU).  Per row, on the patterns of weight > 0: lnf within
1e-9, hence |lnL - sum_h w_h lnf_ref| <= 1e-9 sum_h w_h; d1 and d2 within rtol 1e-9, atol 1e-9; lnL0 against eval within 1e-10 |lnL|;
eval keeps its bits (the edge tests' bounds)."""
import copy
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import attach_ref as at
import gradient_ref as gr
import nni_ref as nr
import placement_ref as pr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import parse_newick
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_nni_gpu import _unrest_problem

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)


def _check(pb, eng=None, scale_every=None, derivatives="oracle"):
    """One call for every non-root v and all four roles at lengths drawn in [0.5, 2] x (t_v / 2, t_v / 2, 0.1), against the oracle on
    every enlarged tree; returns (engine, queries, rows, t3, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    queries = pr.queries_of(pb)
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    rows, t3 = at.all_rows(pb, len(queries), seed=7)
    assert len(rows) == 4 * (t.n_nodes - 1)
    got = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert np.isfinite(got["lnL"]).all() and np.isfinite(got["d1"]).all() and np.isfinite(got["d2"]).all() and np.isfinite(got["lnf"]).all()
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    restated = at.attach_scores(pb, queries, rows, t3) if derivatives == "restatement" else None
    worst_f = worst_l = worst_d = 0.0
    for i in range(len(rows)):
        q, v, role = (int(c) for c in rows[i])
        big, nodes = at.attached_problem(pb, v, t3[i], queries[q], 0, scale_every)
        ref = oracle.evaluate(big)
        worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        worst_l = max(worst_l, abs(got["lnL"][i] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
        if role < 0:
            assert got["d1"][i] == 0 and got["d2"][i] == 0
            continue
        if derivatives == "oracle":
            _, dl, ddl = oracle.eval_branch(big, nodes[role], np.array([t3[i][role]]))
            d1, d2 = dl[0], ddl[0]
        else:
            d1, d2 = restated["d1"][i], restated["d2"][i]
            assert np.max(np.abs(got["lnf"][i] - restated["lnf"][i])[live]) <= 1e-9
        worst_d = max(worst_d, abs(got["d1"][i] - d1), abs(got["d2"][i] - d2))
        assert np.allclose(got["d1"][i], d1, **TOL), (i, rows[i], got["d1"][i], d1)
        assert np.allclose(got["d2"][i], d2, **TOL), (i, rows[i], got["d2"][i], d2)
    print("%d rows: lnf max abs error %.3e; lnL %.3e (allowed %.3e); d1, d2 max abs error %.3e" % (len(rows), worst_f, worst_l, 1e-9 * wsum, worst_d))
    assert worst_f <= 1e-9
    assert worst_l <= 1e-9 * wsum
    return eng, queries, rows, t3, got


# 1 ---- parity with the oracle: the shapes of the gradient's parity tests ---------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_scores_and_derivatives_match_the_oracle_on_every_enlarged_tree(name):
    _check(gr.reversible_problem(name), scale_every=nr.scale_every_of(name))


@pytest.mark.parametrize("n", [64, 21])
def test_scores_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150))


def test_scores_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


# 2 ---- models that are not reversible with respect to the gene's pi ------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,seed,genes", [(4, 2, 306, 1), (61, 2, 363, 2)])
def test_scores_with_eigen_systems_of_different_pi_per_label(n, K, seed, genes):
    _check(_branch_model_problem(n, K, seed, n_genes=genes), derivatives="restatement")


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))), derivatives="restatement")


# 3 ---- agreement with the grid call ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_split_lengths_agree_with_placement_scores(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb)
    phi, tau = 0.3, 0.07
    grid = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=(tau,), phi=phi, want_lnf=True)
    grad = eng.gradient(t.branch, pb.gene_rate)
    rows = np.array([[q, v, -1] for q in range(len(queries)) for v in grid["edges"]], dtype=np.int32)
    t3 = np.array([[(1 - phi) * t.branch[v], phi * t.branch[v], tau] for _, v, _ in rows])
    got = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    ref_l, ref_f = grid["lnL"][:, :, 0].reshape(-1), grid["lnf"][:, :, 0].reshape(len(rows), -1)
    assert np.all(np.abs(got["lnL"] - ref_l) <= 1e-10 * np.abs(ref_l)), (got["lnL"], ref_l)
    assert np.max(np.abs(got["lnf"] - ref_f)[:, pb.weights > 0]) <= 1e-9
    assert not got["d1"].any() and not got["d2"].any()
    again = eng.placement_scores(t.branch, pb.gene_rate, queries=queries, pendant=(tau,), phi=phi, want_lnf=True)
    assert again["lnL"].tobytes() == grid["lnL"].tobytes() and again["lnf"].tobytes() == grid["lnf"].tobytes()
    assert eng.gradient(t.branch, pb.gene_rate)["grad"].tobytes() == grad["grad"].tobytes()


# 4 ---- bytes ------------------------------------------------------------------------------------------------------------------------------------

KEYS = ("lnL", "d1", "d2", "lnf")


def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_ATTACH_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips with all rows (test_attach_cpu.py): several batches, equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=5)
    one = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    assert engine.attach_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_ATTACH_ARENA_MB", "1")
    many = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    assert engine.attach_info()["last_batches"] > 1
    _same(one, many)
    big, _ = at.attached_problem(pb, rows[7][1], t3[7], queries[rows[7][0]])
    assert np.max(np.abs(one["lnf"][7] - oracle.evaluate(big)["lnf"])) <= 1e-9


@pytest.mark.parametrize("n", [4, 61])
def test_groups_of_rows_have_the_same_bytes(n, monkeypatch):
    """A workspace that one tile of patterns with all rows does not fit walks the rows in groups (which cut the runs of a node's rows)."""
    pb = helpers.random_problem(n, 9, 150, K=2, seed=600 + n, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=5)
    one = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    K, n_int, ns = 2, t.n_nodes - t.n_tips, 64 if n == 61 else n
    fixed, per_row = 2 * K * n_int * (ns + 1) * 8, (4 * K + 3) * 8
    mb = (fixed + 4.5 * per_row) * 64 / 1048576.0      # room for one tile with three rows and the present tree
    monkeypatch.setenv("PAML_AMD_ATTACH_ARENA_MB", "%.9f" % mb)
    _same(one, eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True))
    assert engine.attach_info()["last_batches"] == 3      # (150 patterns in tiles of 64)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"])
def test_a_row_has_the_same_bytes_wherever_it_stands(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=5)
    full = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    _same(full, eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True))      # a second call
    rev = eng.attach_scores(t.branch, pb.gene_rate, queries, rows[::-1], t3[::-1], want_lnf=True)
    pick = [5, 2, 2, len(rows) - 1]
    sub = eng.attach_scores(t.branch, pb.gene_rate, queries, rows[pick], t3[pick], want_lnf=True)
    for key in KEYS:
        assert rev[key][::-1].tobytes() == full[key].tobytes(), key
        assert sub[key].tobytes() == full[key][pick].tobytes(), key
    assert np.float64(sub["lnL0"]).tobytes() == np.float64(full["lnL0"]).tobytes() == np.float64(rev["lnL0"]).tobytes()
    # the queries in another order, and a sub-list of them
    perm = np.arange(len(queries))[::-1]
    r2 = rows.copy()
    r2[:, 0] = perm[rows[:, 0]]      # (perm is its own inverse)
    _same(full, eng.attach_scores(t.branch, pb.gene_rate, queries[perm], r2, t3, want_lnf=True))
    only = rows[:, 0] == 1
    r3 = rows[only].copy()
    r3[:, 0] = 0
    one_q = eng.attach_scores(t.branch, pb.gene_rate, queries[1:2], r3, t3[only], want_lnf=True)
    for key in KEYS:
        assert one_q[key].tobytes() == full[key][only].tobytes(), key
    # role -1: no derivatives, and the very same lnf (the three factors of f_hk are formed the same way for every role)
    plain = rows.copy()
    plain[:, 2] = -1
    none = eng.attach_scores(t.branch, pb.gene_rate, queries, plain, t3, want_lnf=True)
    assert none["lnf"].tobytes() == full["lnf"].tobytes() and not none["d1"].any() and not none["d2"].any()


# 5 ---- the reference's printed maximum ---------------------------------------------------------------------------------------------------------

def test_the_references_maximum_of_brown_hky85_is_a_maximum_of_the_placement():
    """The golden brown_hky85 (5 taxa, lnL -2665.422858 at the reference's printed MLEs) with Human taken out: the branches above node 7
    and above Chimpanzee become one branch of length 0.017471 + 0.053761; pi, kappa and the other lengths are the golden's.  Human placed
    on that branch at (0.017471, 0.053761, 0.041370) is the reference's tree: its lnL within the golden bound of
    tests/test_oracle_golden.py, and along each of the three branches Newton's step |d1 / d2| <= 5e-6 (the CPU oracle on the 5-taxon
    golden gives steps of -1.42e-6 (pendant), 1.9e-8 (dn) and -4.3e-7 (up): what the six printed decimals leave)."""
    g = helpers.load_golden("brown_hky85")
    pb5 = helpers.problem_from_golden(g)
    pb = copy.copy(pb5)
    pb.tree = parse_newick("((Chimpanzee: %.6f, Gorilla: 0.057580): 0.053057, Orangutan: 0.100159, Gibbon: 0.138990);" % (0.017471 + 0.053761), names=g["names"][1:])
    pb.z = np.ascontiguousarray(pb5.z[1:])
    eng = engine_for(pb)
    rows = np.array([[0, 0, role] for role in (0, 1, 2)], dtype=np.int32)
    t3 = np.tile([0.017471, 0.053761, 0.041370], (3, 1))
    got = eng.attach_scores(pb.tree.branch, pb.gene_rate, pb5.z[:1], rows, t3)
    print("lnL %r (printed %r); Newton steps up, dn, pendant: %r" % (got["lnL"], g["lnL"], -got["d1"] / got["d2"]))
    assert np.all(np.abs(got["lnL"] - g["lnL"]) <= 2e-6 + 1e-9 * abs(g["lnL"]))
    assert np.all(got["d2"] < 0) and np.all(np.abs(got["d1"] / got["d2"]) <= 5e-6)


# 6 ---- arguments and state -------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_attach_scores.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=7)
    n = len(rows)
    br, lnl, d1, d2, lnl0 = np.ascontiguousarray(t.branch), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(1)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    EINVAL, EUNSUPPORTED = -1, -4

    def call(e, n_q, n_rows, branch, qz, rw, tt, l0, l, a1, a2, label=0):
        return L.paml_amd_attach_scores(e._h, p(branch), None, n_q, p(qz), n_rows, p(rw), p(tt), label, p(l0), p(l), p(a1), p(a2), None)

    def bad(e, rc, text, code=EINVAL):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("attach_scores") and text in msg, msg
    good = [br, queries, rows, t3, lnl0, lnl, d1, d2]
    for k in range(len(good)):
        bad(eng, call(eng, len(queries), n, *[None if j == k else a for j, a in enumerate(good)]), "null argument")
    bad(eng, call(eng, 0, n, *good), "n_q < 1")
    bad(eng, call(eng, len(queries), 0, *good), "n_rows < 1")
    for label in (-1, pb.n_labels):
        bad(eng, call(eng, len(queries), n, *good, label=label), "pendant_label = %d is outside" % label)
    badq = queries.copy()
    badq[0, 5] = pb.n_codes
    cases = [((len(queries), 1, 0), (0.1, 0.1, 0.1), queries, "query %d is out of range" % len(queries)), ((-1, 1, 0), (0.1, 0.1, 0.1), queries, "is out of range"),
             ((0, t.root, 0), (0.1, 0.1, 0.1), queries, "is the root"), ((0, t.n_nodes, 0), (0.1, 0.1, 0.1), queries, "out of range"),
             ((0, -1, 0), (0.1, 0.1, 0.1), queries, "out of range"), ((0, 1, 3), (0.1, 0.1, 0.1), queries, "role 3"), ((0, 1, -2), (0.1, 0.1, 0.1), queries, "role -2"),
             ((0, 1, 0), (-0.1, 0.1, 0.1), queries, "length 0"), ((0, 1, 0), (0.1, np.nan, 0.1), queries, "length 1"), ((0, 1, 0), (0.1, 0.1, np.inf), queries, "length 2"),
             ((0, 1, 0), (0.1, 0.1, 0.1), badq, "pattern 5: character code %d >= n_codes" % pb.n_codes)]
    for row, lengths, qz, text in cases:
        one, t1 = np.array([row], dtype=np.int32), np.array([lengths], dtype=np.float64)
        bad(eng, call(eng, len(queries), 1, br, qz, one, t1, lnl0, lnl, d1, d2), "row 0")
        bad(eng, call(eng, len(queries), 1, br, qz, one, t1, lnl0, lnl, d1, d2), text)
        two, t2 = np.ascontiguousarray(np.vstack([[[1, 2, 1]], one]).astype(np.int32)), np.ascontiguousarray(np.vstack([t3[:1], t1]))
        bad(eng, call(eng, len(queries), 2, br, qz, two, t2, lnl0, lnl, d1, d2), "row 1")      # (wherever it stands in the list)
    # a code with an empty state set, in a query that a row names (a query no row names is not read)
    pa = gr.reversible_problem("4-K3-amb-scale3-2genes")
    nch, empty = pa.n_chara.copy(), pa.n_codes - 1
    nch[empty] = 0
    e3 = engine_for(pa)
    e3.set_tips(np.where(pa.z == empty, 0, pa.z).astype(np.uint8), pa.weights, 0, nch, pa.chara_map.copy(), pa.gene_off)
    q3 = np.ascontiguousarray(pa.z[:2])
    q3 = np.where(q3 == empty, 0, q3).astype(np.uint8)
    q3[1, 5] = empty
    ra, ta, la = np.array([[0, 2, 0], [1, 2, 1]], dtype=np.int32), np.full((2, 3), 0.1), np.zeros(2)
    bad(e3, call(e3, 2, 2, np.ascontiguousarray(pa.tree.branch), q3, ra, ta, lnl0, la, la.copy(), la.copy()), "row 1: query 1, pattern 5: character code %d has an empty state set" % empty)
    assert call(e3, 2, 1, np.ascontiguousarray(pa.tree.branch), q3, ra, ta, lnl0, la, la.copy(), la.copy()) == 0 and la[0] < 0
    lnl0[:] = 0
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, call(fresh, len(queries), n, *good), "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    pq = _unrest_problem()
    engq = engine_for(pq)
    qq = pr.queries_of(pq)
    rq, tq = at.all_rows(pq, len(qq), seed=7)
    bad(engq, call(engq, len(qq), len(rq), np.ascontiguousarray(pq.tree.branch), qq, rq, tq, lnl0, np.zeros(len(rq)), np.zeros(len(rq)), np.zeros(len(rq))),
        "rate-matrix (UNREST)", EUNSUPPORTED)
    assert not lnl.any() and not lnl0.any() and not d1.any() and not d2.any()
    # want_lnf off; get_pmat afterwards returns the tree's own matrices; the other calls keep their results
    before = dict(nni=eng.nni_scores(t.branch, pb.gene_rate), grad=eng.gradient(t.branch, pb.gene_rate), spr=eng.spr_scores(t.branch, pb.gene_rate),
                  place=eng.placement_scores(t.branch, pb.gene_rate, queries=queries))
    plain = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3)
    assert plain["lnf"] is None
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    a = eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3, want_lnf=True)
    assert all(a[k].tobytes() == plain[k].tobytes() for k in ("lnL", "d1", "d2")) and np.float64(a["lnL0"]).tobytes() == np.float64(plain["lnL0"]).tobytes()
    assert eng.nni_scores(t.branch, pb.gene_rate)["lnL"].tobytes() == before["nni"]["lnL"].tobytes()
    assert eng.gradient(t.branch, pb.gene_rate)["grad"].tobytes() == before["grad"]["grad"].tobytes()
    assert eng.spr_scores(t.branch, pb.gene_rate)["lnL"].tobytes() == before["spr"]["lnL"].tobytes()
    assert eng.placement_scores(t.branch, pb.gene_rate, queries=queries)["lnL"].tobytes() == before["place"]["lnL"].tobytes()
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    ref = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    eng.attach_scores(t.branch, pb.gene_rate, queries, rows, t3)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x_, y_) for x_, y_ in zip(ref, after))
    assert engine.attach_info()["last_batches"] == 1 and engine.attach_info()["last_kernel_ms"] > 0
