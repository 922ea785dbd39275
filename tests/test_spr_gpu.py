"""paml_amd_spr_scores: the lnL and the per-pattern log likelihoods of subtree-prune-and-regraft neighbours of the tree in one engine
call.  Reference: oracle.evaluate of the rearranged problem (spr_ref.moved_problem; tests/test_spr_cpu.py pins the numpy restatement of
the definition on it on the CPU).  Per move, on the patterns of weight > 0: lnf within 1e-9 (the gradient tests' bound for lnf), hence
|lnL - sum_h w_h lnf_ref| <= 1e-9 sum_h w_h; lnL0 against eval within 1e-10 |lnL|; eval keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle
import gradient_ref as gr
import nni_ref as nr
import spr_ref as sr
from paml_amd import engine
from paml_amd.engine import engine_for
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_nni_gpu import _unrest_problem

pytestmark = pytest.mark.gpu


def _check(pb, eng=None, scale_every=None, phi=0.5, pick=None):
    """One call for the canonical list of pb (or its moves `pick`) against the oracle on every rearranged tree; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    moves = t.spr_moves() if pick is None else t.spr_moves()[pick]
    got = eng.spr_scores(t.branch, pb.gene_rate, moves=None if pick is None else moves, phi=phi, want_lnf=True)
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base), (got["lnL0"], base)
    assert np.array_equal(got["moves"], moves) and len(moves) >= 1
    live = pb.weights > 0
    wsum = float(pb.weights[live].sum())
    worst_f, worst_l = 0.0, 0.0
    for i, (s, x) in enumerate(got["moves"]):
        ref = oracle.evaluate(sr.moved_problem(pb, s, x, phi, scale_every))
        worst_f = max(worst_f, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        worst_l = max(worst_l, abs(got["lnL"][i] - float(np.dot(pb.weights[live], ref["lnf"][live]))))
    print("%d moves, phi %.1f: lnf max abs error %.3e; lnL %.3e (allowed %.3e)" % (len(moves), phi, worst_f, worst_l, 1e-9 * wsum))
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


def test_scores_beside_a_polytomy_below_the_root():
    """The sons of a polytomy cannot be pruned; everything else in such a tree can, and the polytomy's sons are targets."""
    import copy
    from paml_amd.problem import parse_newick
    pb = copy.copy(helpers.random_problem(4, 9, 140, K=2, seed=3))
    pb.tree = parse_newick("((1: 0.1, 2: 0.2, 3: 0.1): 0.1, (4: 0.1, (5: 0.3, 6: 0.1): 0.1): 0.2, 7: 0.1, (8: 0.2, 9: 0.1): 0.1);")
    eng, got = _check(pb)
    assert {0, 1, 2} <= set(int(x) for x in got["moves"][:, 1]) and not {0, 1, 2} & set(int(s) for s in got["moves"][:, 0])


@pytest.mark.parametrize("n", [4, 61])
def test_scores_on_a_tree_rooted_at_a_tip(n):
    _check(_rooted_at_tip0(helpers.random_problem(n, 9, 140, K=2, seed=55 + (n == 61))))


def test_scores_of_a_rate_matrix_set():
    """UNREST: only P(t) is used, which the evaluation's builder makes for every kind."""
    _check(_unrest_problem())


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
@pytest.mark.parametrize("phi", [0.0, 1.0, 0.3])
def test_scores_at_other_splits(name, phi):
    _check(gr.reversible_problem(name), scale_every=nr.scale_every_of(name), phi=phi)


# 3 ---- a deep tree: the rescaled chains ----------------------------------------------------------------------------------------------------------

def test_scores_on_a_deep_tree_with_rescaling():
    """Every 17th move of the unlimited list and all moves of the prunable s farthest from the root (the longest path): the cap keeps the
    test at seconds."""
    pb = helpers.random_problem(61, 30, 70, K=2, seed=77 + 61, scale_every=5)
    t = pb.tree
    moves, fa = t.spr_moves(), t.father()

    def depth(v):
        d = 0
        while fa[v] >= 0:
            v, d = fa[v], d + 1
        return d
    deepest = max(set(int(s) for s in moves[:, 0]), key=lambda s: (depth(s), -s))
    pick = sorted(set(range(0, len(moves), 17)) | set(int(i) for i in np.nonzero(moves[:, 0] == deepest)[0]))
    assert depth(deepest) >= 6 and len(pick) > len(moves) // 17 + 20
    _check(pb, scale_every=5, pick=pick)


# 4 ---- end to end: the engine on the rearranged tree ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-K2-amb-scale3"])
def test_eval_of_the_rearranged_tree_agrees(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    got = eng.spr_scores(t.branch, pb.gene_rate)
    fa = t.father()

    def on_path(s, x):      # x is an ancestor of the father of s
        u = fa[fa[s]]
        while u >= 0:
            if u == x:
                return True
            u = fa[u]
        return False
    tip_s = [i for i, (s, x) in enumerate(got["moves"]) if s < t.n_tips]
    internal_s = [i for i, (s, x) in enumerate(got["moves"]) if s >= t.n_tips and on_path(s, x)]
    assert tip_s and internal_s
    for i in (tip_s[0], internal_s[0]):
        q = sr.moved_problem(pb, *got["moves"][i], 0.5, nr.scale_every_of(name))
        eng.set_tree(q.tree, q.scale_node)
        lnl = eng.eval(q.tree.branch, pb.gene_rate)["lnL"]
        assert abs(lnl - got["lnL"][i]) <= 1e-10 * abs(lnl), (i, lnl, got["lnL"][i])


# 5 ---- bytes ------------------------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    assert np.float64(a["lnL0"]).tobytes() == np.float64(b["lnL0"]).tobytes()
    assert a["lnL"].tobytes() == b["lnL"].tobytes() and a["lnf"].tobytes() == b["lnf"].tobytes()


def test_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_SPR_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips (the partials alone take 14 KB a pattern):
    several batches, as the library reports them, and equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.spr_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_SPR_ARENA_MB", "1")
    many = eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True)
    assert engine.spr_info()["last_batches"] > 1
    _same(one, many)
    ref = oracle.evaluate(sr.moved_problem(pb, *one["moves"][3]))
    assert np.max(np.abs(one["lnf"][3] - ref["lnf"])) <= 1e-9


@pytest.mark.parametrize("n", [4, 61])
def test_groups_of_prunes_have_the_same_bytes(n, monkeypatch):
    """A workspace that one tile of patterns with all rows does not fit walks the moves in groups of whole prunes: here room for one
    tile, the present tree and twice the rows of the prune with the most targets."""
    pb = helpers.random_problem(n, 9, 150, K=2, seed=600 + n, scale_every=3)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True)
    K, n_int, ns = 2, t.n_nodes - t.n_tips, 64 if n == 61 else n
    most = int(np.bincount(one["moves"][:, 0]).max())
    fixed, per_row = 4 * K * n_int * (ns + 1) * 8, (2 * K + 1) * 8
    mb = (fixed + (2 * most + 1.5) * per_row) * 64 / 1048576.0
    assert len(one["moves"]) > 4 * most
    monkeypatch.setenv("PAML_AMD_SPR_ARENA_MB", "%.9f" % mb)
    _same(one, eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True))
    assert engine.spr_info()["last_batches"] == 3      # (150 patterns in tiles of 64)


@pytest.mark.parametrize("name", ["4-K3-amb-scale3-2genes", "61-14tips-polytomy"])
def test_a_move_has_the_same_bytes_wherever_it_stands(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    eng = engine_for(pb)
    full = eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True)
    _same(full, eng.spr_scores(t.branch, pb.gene_rate, want_lnf=True))      # a second call
    mv = full["moves"]
    rev = eng.spr_scores(t.branch, pb.gene_rate, moves=mv[::-1], want_lnf=True)
    assert rev["lnL"][::-1].tobytes() == full["lnL"].tobytes() and rev["lnf"][::-1].tobytes() == full["lnf"].tobytes()
    pick = [5, 2, 2, len(mv) - 1, 40]
    sub = eng.spr_scores(t.branch, pb.gene_rate, moves=mv[pick], want_lnf=True)
    assert sub["lnL"].tobytes() == full["lnL"][pick].tobytes() and sub["lnf"].tobytes() == full["lnf"][pick].tobytes()
    assert np.float64(sub["lnL0"]).tobytes() == np.float64(full["lnL0"]).tobytes() == np.float64(rev["lnL0"]).tobytes()
    near = eng.spr_scores(t.branch, pb.gene_rate, radius=1, want_lnf=True)      # the radius-1 list: a sub-list too
    at = [int(np.nonzero((mv == m).all(axis=1))[0][0]) for m in near["moves"]]
    assert np.array_equal(near["moves"], t.spr_moves(1)) and near["lnf"].tobytes() == full["lnf"][at].tobytes()


@pytest.mark.parametrize("n", [4, 61])
def test_live_patterns_keep_their_bytes_when_others_have_weight_zero(n):
    pb = helpers.random_problem(n, 9, 150, K=2, seed=500 + n, scale_every=3)
    t = pb.tree
    full = engine_for(pb).spr_scores(t.branch, pb.gene_rate, want_lnf=True)
    pb.weights = pb.weights.copy()
    pb.weights[::3] = 0
    eng, got = _check(pb, scale_every=3)
    live = pb.weights > 0
    assert got["lnf"][:, live].tobytes() == full["lnf"][:, live].tobytes()
    assert np.isfinite(got["lnL"]).all()


# 6 ---- arguments and state -------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state():
    pb4 = helpers.random_problem(4, 9, 140, K=2, seed=3)
    t = pb4.tree
    eng = engine_for(pb4)
    L = eng._L
    L.paml_amd_spr_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    mv = t.spr_moves()
    br, lnl, lnl0 = np.ascontiguousarray(t.branch), np.zeros(len(mv)), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(e, rc, text):
        assert rc == EINVAL, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("spr_scores") and text in msg, msg
    n = len(mv)
    bad(eng, L.paml_amd_spr_scores(eng._h, None, None, n, p(mv), 0.5, p(lnl0), p(lnl), None), "null argument")
    bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, n, None, 0.5, p(lnl0), p(lnl), None), "null argument")
    bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, n, p(mv), 0.5, None, p(lnl), None), "null argument")
    bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, n, p(mv), 0.5, p(lnl0), None, None), "null argument")
    bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, 0, p(mv), 0.5, p(lnl0), p(lnl), None), "n_moves < 1")
    for phi in (-0.01, 1.01, float("nan"), float("inf")):
        bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, n, p(mv), phi, p(lnl0), p(lnl), None), "outside [0, 1]")
    fa = t.father()
    s, x = (int(c) for c in mv[0])
    f = int(fa[s])
    c = next(int(u) for u in t.sons[f] if u != s)
    under_root = int(t.sons[t.root][0])
    inner = next(v for v in range(t.n_tips, t.n_nodes) if v != t.root and fa[v] != t.root)
    for move, text in [((t.root, x), "is the root"), ((s, t.root), "is the root"), ((t.n_nodes, x), "out of range"), ((-1, x), "out of range"),
                       ((s, t.n_nodes + 5), "out of range"), ((s, -2), "out of range"), ((under_root, x), "father of %d is the root" % under_root),
                       ((s, f), "is the father of"), ((s, c), "is the sibling of"), ((inner, int(t.sons[inner][0])), "lies in the subtree below"),
                       ((inner, inner), "lies in the subtree below")]:
        one = np.array([move], dtype=np.int32)
        bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, 1, p(one), 0.5, p(lnl0), p(lnl), None), "move 0")
        bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, 1, p(one), 0.5, p(lnl0), p(lnl), None), text)
        two = np.ascontiguousarray(np.vstack([mv[:1], one]), dtype=np.int32)      # (wherever it stands in the list)
        bad(eng, L.paml_amd_spr_scores(eng._h, p(br), None, 2, p(two), 0.5, p(lnl0), p(lnl), None), "move 1")
    # a father that is a polytomy below the root; the tree's other prunes are served
    import copy
    from paml_amd.problem import parse_newick
    pbp = copy.copy(pb4)
    pbp.tree = tp = parse_newick("((1: 0.1, 2: 0.2, 3: 0.1): 0.1, (4: 0.1, (5: 0.3, 6: 0.1): 0.1): 0.2, 7: 0.1, (8: 0.2, 9: 0.1): 0.1);")
    engp = engine_for(pbp)
    poly = next(v for v in range(tp.n_nodes) if v != tp.root and len(tp.sons[v]) > 2)
    one = np.array([(tp.sons[poly][0], 6)], dtype=np.int32)
    bad(engp, L.paml_amd_spr_scores(engp._h, p(np.ascontiguousarray(tp.branch)), None, 1, p(one), 0.5, p(lnl0), p(lnl), None), "exactly two sons")
    assert not lnl.any() and not lnl0.any()
    fresh = engine.Engine(4, 9, 140)      # a model that is not set yet
    bad(fresh, L.paml_amd_spr_scores(fresh._h, p(br), None, n, p(mv), 0.5, p(lnl0), p(lnl), None), "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    # want_lnf off; get_pmat afterwards returns the tree's own matrices
    plain = eng.spr_scores(t.branch, pb4.gene_rate)
    assert plain["lnf"] is None and np.array_equal(plain["moves"], mv)
    assert np.allclose(eng.get_pmat(0, 1, 1), oracle.pmat_branch(pb4, 0, 1, 1), atol=1e-13)
    a = eng.spr_scores(t.branch, pb4.gene_rate, want_lnf=True)
    assert a["lnL"].tobytes() == plain["lnL"].tobytes() and np.float64(a["lnL0"]).tobytes() == np.float64(plain["lnL0"]).tobytes()
    # eval_branch's resident state starts over and agrees
    node = t.n_tips + 1
    ts = np.array([t.branch[node], 0.2])
    before = engine_for(pb4).eval_branch(node, ts, t.branch, pb4.gene_rate)
    after = eng.eval_branch(node, ts, t.branch, pb4.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert engine.spr_info()["last_batches"] == 1 and engine.spr_info()["last_kernel_ms"] > 0


def test_the_other_whole_tree_calls_return_what_they_returned_before():
    """gradient, nni_scores and placement_scores after an spr_scores call: the same bytes as on an engine that never made one."""
    pb = helpers.random_problem(61, 9, 150, K=2, seed=41, scale_every=3)
    t = pb.tree
    qz = pb.z[:1].copy()
    fresh, eng = engine_for(pb), engine_for(pb)
    eng.spr_scores(t.branch, pb.gene_rate)
    for call in (lambda e: e.gradient(t.branch, pb.gene_rate)["grad"], lambda e: e.nni_scores(t.branch, pb.gene_rate)["lnL"],
                 lambda e: e.placement_scores(t.branch, pb.gene_rate, queries=qz)["lnL"]):
        assert call(eng).tobytes() == call(fresh).tobytes()
