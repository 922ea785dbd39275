"""paml_amd_edge_scores: the lnL of every configuration of every edge at trial lengths of the five branches around it, with the first
and second derivative along one of them, in one engine call.  Reference: oracle.evaluate of the rearranged problem with the override
lengths written into its tree (edge_ref.rearranged_problem) and oracle.eval_branch on it at the row's length; on models that are not
reversible with respect to the gene's pi the derivatives are held against the numpy restatement (tests/edge_ref.py, which
tests/test_edge_cpu.py pins on the oracle on the CPU).  Per row, on the patterns of weight > 0: lnf within 1e-9 (the gradient tests'
bound for lnf), hence |lnL - sum_h w_h lnf_ref| <= 1e-9 sum_h w_h; d1 and d2 within rtol 1e-9, atol 1e-9 (the gradient tests' TOL);
lnL0 against eval within 1e-10 |lnL|; eval keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import ancestral_ref as ar
import edge_ref as er
import gradient_ref as gr
import nni_ref as nr
from paml_amd import engine
from paml_amd.engine import engine_for
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_nni_gpu import _unrest_problem

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)


def _check(pb, eng=None, scale_every=None, derivatives="oracle", one_role=False):
    """One call for every edge, configuration and role of u (one_role: one u per configuration, in turn) at lengths drawn in
    [0.5, 2] x the tree's, against the oracle on every rearranged tree; returns (engine, rows, ovr_node, ovr_t, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    rows, on, ot = er.all_rows(t, seed=7)
    if one_role:
        keep = np.array([i0 + (i0 // 5) % 5 for i0 in range(0, len(rows), 5)])
        rows, on, ot = rows[keep], on[keep], ot[keep]
    assert len(rows) >= (3 if one_role else 15)
    got = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert np.isfinite(got["lnL"]).all() and np.isfinite(got["d1"]).all() and np.isfinite(got["d2"]).all() and np.isfinite(got["lnf"]).all()
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    restated = er.edge_scores(pb, ar.matrices_from_oracle(pb), rows, on, ot) if derivatives == "restatement" else None
    worst_f = worst_l = worst_d = 0.0
    ref, ref_of = None, None
    for i in range(len(rows)):
        v, s, x, u = (int(c) for c in rows[i])
        key = (v, s, x, ot[i].tobytes())
        if key != ref_of:      # (the five roles of one edge and configuration share their lengths: one evaluation of the oracle)
            q = er.rearranged_problem(pb, v, s, x, on[i], ot[i], scale_every)
            ref, ref_of = oracle.evaluate(q), key
        worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        worst_l = max(worst_l, abs(got["lnL"][i] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
        if derivatives == "oracle":
            _, dl, ddl = oracle.eval_branch(q, u, np.array([q.tree.branch[u]]))
            d1, d2 = dl[0], ddl[0]
        elif derivatives == "restatement":
            d1, d2 = restated["d1"][i], restated["d2"][i]
        else:
            continue
        worst_d = max(worst_d, abs(got["d1"][i] - d1), abs(got["d2"][i] - d2))
        assert np.allclose(got["d1"][i], d1, **TOL), (i, rows[i], got["d1"][i], d1)
        assert np.allclose(got["d2"][i], d2, **TOL), (i, rows[i], got["d2"][i], d2)
    print("%d rows: lnf max abs error %.3e; lnL %.3e (allowed %.3e); d1, d2 max abs error %.3e" % (len(rows), worst_f, worst_l, 1e-9 * wsum, worst_d))
    assert worst_f <= 1e-9
    assert worst_l <= 1e-9 * wsum
    return eng, rows, on, ot, got


# 1 ---- parity with the oracle: the shapes of the gradient's parity tests ---------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_scores_and_derivatives_match_the_oracle_on_every_rearranged_tree(name):
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
    _check(_branch_model_problem(n, K, seed, n_genes=genes), derivatives="restatement")


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))), derivatives="restatement")


# 3 ---- cross-checks against the existing calls ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_overrides_equal_to_the_trees_lengths_agree_with_nni_scores_and_the_gradient(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    edges, five = t.edge_configs()
    rows = np.array([[cfg[0], cfg[1], cfg[2], u] for e in range(len(edges)) for cfg in edges[e] for u in five[e]], dtype=np.int32)
    on = np.repeat(five, 15, axis=0)
    ot = t.branch[on]
    got = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot)
    swaps = np.ascontiguousarray(rows[rows[:, 1] >= 0][::5, :3])
    nni = eng.nni_scores(t.branch, pb.gene_rate, swaps=swaps)
    mine = got["lnL"][rows[:, 1] >= 0][::5]
    assert len(swaps) == 2 * len(edges) and np.all(np.abs(mine - nni["lnL"]) <= 1e-10 * np.abs(nni["lnL"])), (mine, nni["lnL"])
    grad = eng.gradient(t.branch, pb.gene_rate)
    present = rows[:, 1] < 0
    assert present.sum() == 5 * len(edges)
    assert np.allclose(got["d1"][present], grad["grad"][rows[present, 3]], **TOL)
    assert np.all(np.abs(got["lnL"][present] - grad["lnL"]) <= 1e-10 * abs(grad["lnL"]))


# 4 ---- a deep tree: the rescaled outer chain ---------------------------------------------------------------------------------------------------

def test_scores_on_a_deep_tree_with_rescaling():
    _check(helpers.random_problem(61, 30, 70, K=2, seed=77 + 61, scale_every=5), scale_every=5, derivatives=None, one_role=True)


# 5 ---- bytes ------------------------------------------------------------------------------------------------------------------------------------

KEYS = ("lnL", "d1", "d2", "lnf")


def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_EDGE_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips with all rows (test_edge_cpu.py): several batches, equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    rows, on, ot = er.all_rows(t, seed=5)
    one = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    assert engine.edge_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_EDGE_ARENA_MB", "1")
    many = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    assert engine.edge_info()["last_batches"] > 1
    _same(one, many)
    ref = oracle.evaluate(er.rearranged_problem(pb, *rows[7][:3], on[7], ot[7]))
    assert np.max(np.abs(one["lnf"][7] - ref["lnf"])) <= 1e-9


@pytest.mark.parametrize("n", [4, 61])
def test_groups_of_rows_have_the_same_bytes(n, monkeypatch):
    """A workspace that one tile of patterns with all rows does not fit walks the rows in groups."""
    pb = helpers.random_problem(n, 9, 150, K=2, seed=600 + n, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    rows, on, ot = er.all_rows(t, seed=5)
    one = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    K, n_int, ns = 2, t.n_nodes - t.n_tips, 64 if n == 61 else n
    fixed, per_row = 2 * K * n_int * (ns + 1) * 8, (4 * K + 3) * 8
    mb = (fixed + 5.5 * per_row) * 64 / 1048576.0      # room for one tile with four rows and the present tree
    assert len(rows) > 4
    monkeypatch.setenv("PAML_AMD_EDGE_ARENA_MB", "%.9f" % mb)
    _same(one, eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True))
    assert engine.edge_info()["last_batches"] == 3      # (150 patterns in tiles of 64)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"])
def test_a_row_has_the_same_bytes_wherever_it_stands(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    rows, on, ot = er.all_rows(t, seed=5)
    full = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    _same(full, eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True))      # a second call
    rev = eng.edge_scores(t.branch, pb.gene_rate, rows[::-1], on[::-1], ot[::-1], want_lnf=True)
    pick = [5, 2, 2, len(rows) - 1]
    sub = eng.edge_scores(t.branch, pb.gene_rate, rows[pick], on[pick], ot[pick], want_lnf=True)
    for key in KEYS:
        assert rev[key][::-1].tobytes() == full[key].tobytes(), key
        assert sub[key].tobytes() == full[key][pick].tobytes(), key
    assert np.float64(sub["lnL0"]).tobytes() == np.float64(full["lnL0"]).tobytes() == np.float64(rev["lnL0"]).tobytes()
    # the slots of a row in another order: the same bytes; u = -1: no derivatives, and the same lnf to rounding (the factor of u is
    # multiplied in last: another order of the same products, a few ulp of |lnf| < 1e3, so 1e-12)
    perm = [4, 0, 3, 1, 2]
    mixed = eng.edge_scores(t.branch, pb.gene_rate, rows[:5], on[:5][:, perm], ot[:5][:, perm], want_lnf=True)
    plain = rows[:5].copy()
    plain[:, 3] = -1
    none = eng.edge_scores(t.branch, pb.gene_rate, plain, on[:5], ot[:5], want_lnf=True)
    for key in KEYS:
        assert mixed[key].tobytes() == full[key][:5].tobytes(), key
    assert np.max(np.abs(none["lnf"] - full["lnf"][:5])) <= 1e-12 and not none["d1"].any() and not none["d2"].any()


@pytest.mark.parametrize("n", [4, 61])
def test_live_patterns_keep_their_bytes_when_others_have_weight_zero(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    rows, on, ot = er.all_rows(t, seed=7)
    full = engine_for(pb).edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, rows2, on2, ot2, got = _check(pb, scale_every=3)
    assert np.array_equal(rows, rows2) and np.array_equal(ot, ot2)
    live = pb.weights > 0
    assert got["lnf"][:, live].tobytes() == full["lnf"][:, live].tobytes()
    assert np.isfinite(got["lnL"]).all()


# 6 ---- arguments and state -------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    L.paml_amd_edge_scores.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 8
    rows, on, ot = er.all_rows(t, seed=7)
    n = len(rows)
    br, lnl, d1, d2, lnl0 = np.ascontiguousarray(t.branch), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(1)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    EINVAL, EUNSUPPORTED = -1, -4

    def call(e, n_rows, *arrays):
        return L.paml_amd_edge_scores(e._h, p(arrays[0]), None, n_rows, *[p(a) for a in arrays[1:]], None)

    def bad(e, rc, text, code=EINVAL):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("edge_scores") and text in msg, msg
    good = [br, rows, on, ot, lnl0, lnl, d1, d2]
    for k in range(len(good)):
        bad(eng, call(eng, n, *[None if j == k else a for j, a in enumerate(good)]), "null argument")
    bad(eng, call(eng, 0, *good), "n_rows < 1")
    f = t.father()
    edges, five = t.edge_configs()
    e0 = next(e for e in range(len(edges)) if f[edges[e][0][0]] != t.root)      # an edge whose father is not the root
    v, s, x = (int(c) for c in edges[e0][1])
    fv = int(f[v])
    inner = next(u for u in range(t.n_tips, t.n_nodes) if u != t.root and u != v and f[u] != v and f[v] != u and u != fv and f[u] != fv and f[fv] != u)
    far = int(t.sons[inner][0])
    under_root = next(int(edges[e][0][0]) for e in range(len(edges)) if f[edges[e][0][0]] == t.root)
    o5 = [int(c) for c in five[e0]]
    cases = [((0, s, x, -1), o5, "is a tip"), ((t.root, t.sons[t.root][0], x, -1), o5, "is the root"), ((t.n_nodes, s, x, -1), o5, "out of range"),
             ((-1, s, x, -1), o5, "out of range"), ((v, far, x, -1), o5, "is not a son of %d" % v), ((v, s, v, -1), o5, "is not a son of the father"),
             ((v, s, far, -1), o5, "is not a son of the father"), ((v, s, t.n_nodes + 5, -1), o5, "is not a son of the father"),
             ((v, -1, x, -1), o5, "is not a son of %d" % v), ((v, s, -1, -1), o5, "is not a son of the father"),
             ((v, s, x, -1), o5[:4] + [far], "is not a branch around the edge"), ((v, s, x, -1), o5[:4] + [t.n_nodes], "is not a branch around the edge"),
             ((v, s, x, -1), o5[:4] + [-2], "is not a branch around the edge"), ((v, s, x, -1), o5[:4] + [o5[1]], "is listed twice"),
             ((under_root, -1, -1, -1), [under_root, t.root, -1, -1, -1], "is the root: no branch above it"),
             ((v, s, x, far), o5, "is not among the override nodes"), ((v, s, x, o5[0]), [-1] + o5[1:], "is not among the override nodes")]
    for row, nodes, text in cases:
        one, o1, t1 = np.array([row], dtype=np.int32), np.array([nodes], dtype=np.int32), np.full((1, 5), 0.1)
        bad(eng, call(eng, 1, br, one, o1, t1, lnl0, lnl, d1, d2), text)
        two, o2, t2 = np.ascontiguousarray(np.vstack([rows[:1], one])), np.ascontiguousarray(np.vstack([on[:1], o1])), np.ascontiguousarray(np.vstack([ot[:1], t1]))
        bad(eng, call(eng, 2, br, two, o2, t2, lnl0, lnl, d1, d2), "row 1")      # (wherever it stands in the list)
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, call(fresh, n, *good), "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    pq = _unrest_problem()
    engq = engine_for(pq)
    bad(engq, call(engq, n, np.ascontiguousarray(pq.tree.branch), *good[1:]), "rate-matrix (UNREST)", EUNSUPPORTED)
    assert not lnl.any() and not lnl0.any() and not d1.any() and not d2.any()
    # want_lnf off; get_pmat afterwards returns the tree's own matrices; the other calls keep their results
    before = dict(nni=eng.nni_scores(t.branch, pb.gene_rate), grad=eng.gradient(t.branch, pb.gene_rate), spr=eng.spr_scores(t.branch, pb.gene_rate))
    plain = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot)
    assert plain["lnf"] is None
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb, 0, 1, 1), atol=1e-13)
    a = eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot, want_lnf=True)
    assert all(a[k].tobytes() == plain[k].tobytes() for k in ("lnL", "d1", "d2")) and np.float64(a["lnL0"]).tobytes() == np.float64(plain["lnL0"]).tobytes()
    assert eng.nni_scores(t.branch, pb.gene_rate)["lnL"].tobytes() == before["nni"]["lnL"].tobytes()
    assert eng.gradient(t.branch, pb.gene_rate)["grad"].tobytes() == before["grad"]["grad"].tobytes()
    assert eng.spr_scores(t.branch, pb.gene_rate)["lnL"].tobytes() == before["spr"]["lnL"].tobytes()
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    ref = engine_for(pb).eval_branch(node, ts, t.branch, pb.gene_rate)
    eng.edge_scores(t.branch, pb.gene_rate, rows, on, ot)
    after = eng.eval_branch(node, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x_, y_) for x_, y_ in zip(ref, after))
    assert engine.edge_info()["last_batches"] == 1 and engine.edge_info()["last_kernel_ms"] > 0
