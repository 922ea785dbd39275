"""The matrix-core paths (21..64 states) away from 61 states, and the one-son forms of the branch contraction.

Every matrix-core kernel forks at compile time on "61 states" (the sixteenth k-block holds column 60 alone: a rank-1 term on the vector
pipe instead of four MFMAs); every other order runs all sixteen blocks.  The mitochondrial codes have 60 sense codons, icode 4 / 5 / 11
have 62 / 63 / 64, and this file runs, at 33, 60, 62, 63 and 64 states, what the rest of the suite runs at 61 only:

  1. branch_eig_kernel<NS, S0I, S1I, BTIP, T61 = false> (kernels_branch.h) in all its shapes, and its NS == 1 shapes (A has ONE son in
     the tree seen from the branch: a branch at a bifurcating root, as clock models have it) at 61 states too.  Which shape a call
     launches is computed beforehand from the host-only plan (engine.debug_branch_plan) and the union over the walks is asserted;
  2. cherry_table_kernel<false> and the table walk of the per-tree kernel;
  3. eval_batch, KEEP_PARTIALS / get_partials / eval_dirty, node_posterior, ancestral_marginal and ancestral_joint;
  (4. the device eigensolver's orders are in test_eigen_gpu.py.)

The reference is the CPU oracle throughout, the tolerances are those the 61-state tests hold the same entry points to."""
import copy

import numpy as np
import pytest

import helpers
import oracle
from paml_amd import engine
from paml_amd.engine import JIT, KEEP_PARTIALS, engine_for
from paml_amd.problem import Tree, parse_newick, set_node_scale
from test_ancestral_gpu import _check_joint, _check_marginal
from test_cherry_tables_gpu import on_off
from test_engine_gpu import check

pytestmark = pytest.mark.gpu


# ---- 1. the contraction in the eigen basis ---------------------------------------------------------------------------------------------

# Rooted trees (a bifurcating root, what a clock model passes in), 8 tips.  Seen from a branch at the root R, A = R has ONE son, the root's
# other son: internal at both root branches of ROOTED_INT and at t1's branch of ROOTED_TIP, the tip t1 at the other branch of ROOTED_TIP.
ROOTED_INT = ("((t1:0.11,(t2:0.07,t3:0.21):0.05):0.09,"
              "((t4:0.13,t5:0.3):0.06,(t6:0.02,(t7:0.17,t8:0.08):0.12):0.04):0.15);")
ROOTED_TIP = ("(t1:0.23,((t2:0.11,t3:0.07):0.05,"
              "((t4:0.13,t5:0.3):0.06,(t6:0.02,(t7:0.17,t8:0.08):0.12):0.04):0.15):0.1);")
# The two shapes no larger tree has.  (one tip son, B a tip): A's neighbours are B and that son, both tips, so the tree is A and two tips.
# (two tip sons, B a tip): A's three neighbours are tips, so the tree is the three-tip star.  (branch_ends makes A the internal end;
# eig_forest takes A's sons from the neighbours other than B.)
TWO_TIPS = "(t1:0.2,t2:0.3);"
THREE_TIPS = "(t1:0.2,t2:0.3,t3:0.15);"
# A trifurcating root with two tip sons: at the third son's branch A = the root has two tip sons and B is internal.
ROOT_TIPS = "(t1:0.14,t2:0.06,((t3:0.2,t4:0.09):0.07,((t5:0.12,t6:0.31):0.03,(t7:0.05,(t8:0.16,t9:0.1):0.08):0.11):0.13):0.04);"
TREES = {"rooted_int": (ROOTED_INT, 8), "rooted_tip": (ROOTED_TIP, 8), "root_tips": (ROOT_TIPS, 9), "two_tips": (TWO_TIPS, 2),
         "three_tips": (THREE_TIPS, 3)}

# branch_eig_kernel's template arguments (NS, S0I, S1I) by `variant` of launch_contraction (engine_branch.hip)
VARIANT_SHAPES = [(0, False, False), (1, True, False), (1, False, False), (2, True, True), (2, True, False), (2, False, False)]
ALL_SHAPES = {s + (bt,) for s in VARIANT_SHAPES for bt in (False, True)}
ONE_SON_SHAPES = {s for s in ALL_SHAPES if s[0] == 1}

# (states, tree, classes, ambiguity codes, scale_every, a third of the patterns in states >= 60)
WALKS = [
    (33, "tri", 2, True, None, False), (33, "rooted_tip", 1, False, None, False), (33, "rooted_int", 2, False, None, False),
    (60, "root_tips", 1, False, None, False), (60, "rooted_tip", 2, True, None, False), (60, "rooted_int", 1, False, None, False),
    (60, "poly", 2, False, None, False), (60, "tri", 2, False, 3, False), (60, "two_tips", 1, False, None, False),
    (60, "three_tips", 2, False, None, False),
    (62, "tri", 1, True, None, False), (62, "rooted_tip", 2, False, None, False), (62, "rooted_int", 1, True, None, False),
    (62, "tri", 1, False, None, True),
    (63, "tri", 2, False, None, False), (63, "rooted_tip", 1, True, None, False), (63, "rooted_int", 2, False, None, False),
    (63, "poly", 1, True, None, False), (63, "tri", 2, False, None, True),
    (64, "root_tips", 1, False, None, False), (64, "rooted_tip", 2, True, None, False), (64, "rooted_int", 1, False, None, False),
    (64, "poly", 2, False, None, False), (64, "tri", 1, True, 3, False), (64, "two_tips", 2, False, None, False),
    (64, "three_tips", 1, False, None, False), (64, "tri", 1, False, None, True),
    (61, "rooted_tip", 1, True, None, False), (61, "rooted_int", 2, False, None, False), (61, "two_tips", 1, False, None, False),
]


def _walk_id(w):
    n, tree, K, amb, scale, hi = w
    return "%d-%s-K%d%s%s%s" % (n, tree, K, "-amb" if amb else "", "-scale%d" % scale if scale else "", "-hi" if hi else "")


def _walk_problem(w):
    """The problem of a walk.  The pattern counts (157 .. 421) are no multiple of 16: the last 16-pattern group is ragged."""
    n, tree, K, amb, scale, hi = w
    seed = 7000 + 10 * n + K + len(tree)
    if tree in ("tri", "poly"):
        pb = helpers.random_problem(n, 11 if tree == "poly" else 10, 301 if K == 1 else 157, K=K, seed=seed, ambiguity=amb,
                                    scale_every=scale, polytomy=tree == "poly")
    else:
        text, n_tips = TREES[tree]
        pb = helpers.random_problem(n, max(n_tips, 3), 421 if n_tips <= 3 else 203, K=K, seed=seed, ambiguity=amb)
        pb.tree = parse_newick(text)
        pb.z = np.ascontiguousarray(pb.z[:n_tips])
        assert pb.tree.n_tips == pb.z.shape[0] == n_tips
        if scale:
            pb.scale_node = set_node_scale(pb.tree, scale)
    if scale:
        assert pb.scale_node is not None and pb.scale_node.sum() >= 1
    if hi:      # the whole signal of these patterns sits in the k-block the 61-state form does not compute by MFMA
        rng = np.random.default_rng(seed)
        cols = np.arange(pb.n_patt) % 5 < 2      # 40 % of the patterns, in every 16-pattern group
        pb.z = pb.z.copy()
        pb.z[:, cols] = rng.integers(60, n, size=(pb.tree.n_tips, int(cols.sum())))
        assert (pb.z[:, cols] >= 60).all() and cols.mean() >= 1 / 3
    return pb


def _walk_calls(pb, seed=3):
    """The calls of a minbranches-style walk, [(node_b, trial lengths, branch lengths at the call)]: every branch in pre-order with 1, 4
    and 7 trial lengths (7: more than one launch of the polynomial kernel handles; the order of the three rotates, so that the call
    that forms the coefficients has each of them in turn), the length moving on after most branches; then back up in reverse order,
    one call per branch (moving from a branch to the one above it finds A resident: NS == 0)."""
    t = pb.tree
    order = []

    def pre(i):
        for c in t.sons[i]:
            order.append(c)
            pre(c)
    pre(t.root)
    rng = np.random.default_rng(seed)
    br = np.array(t.branch, dtype=float)
    calls = []
    for i, b in enumerate(order):
        for nt in ((1, 4, 7), (4, 7, 1), (7, 1, 4))[i % 3]:
            ts = np.concatenate([[br[b]], br[b] * rng.uniform(0.3, 2.0, nt - 1) + 1e-3])
            calls.append((b, ts, br.copy()))
        if rng.random() < 0.6:
            br[b] = br[b] * rng.uniform(0.5, 1.6) + 1e-3
    for i, b in enumerate(order[::-1]):
        nt = (4, 1, 7)[i % 3]
        calls.append((b, np.concatenate([[br[b]], br[b] * rng.uniform(0.3, 2.0, nt - 1) + 1e-3]), br.copy()))
    return calls, br


def _predict(pb, calls):
    """What every call launches, from the host-only plan: None for a call served from the stored coefficients (no contraction), else
    branch_eig_kernel's (NS, S0I, S1I, BTIP).  Mirrors eigen_form's `hit`, eig_forest and launch_contraction's `variant`
    (engine_branch.hip).  Also the number of partials the non-hit calls form (branch_counters: n_nodes)."""
    t = pb.tree
    scaled = pb.scale_node is not None and bool(pb.scale_node.any())
    nbr = [[] for _ in range(t.n_nodes)]      # (branch_plan.h: adjacency — the order of the neighbours)
    for i, s in enumerate(t.sons):
        for c in s:
            nbr[i].append(c)
            nbr[c].append(i)
    ends, up, clean, _ = engine.debug_branch_plan(t, [(b, br) for b, _, br in calls], pb.scale_node)
    shapes, coef_node, formed = [], None, 0
    for i, (b, _, _) in enumerate(calls):
        A, B = int(ends[i, 0]), int(ends[i, 1])
        assert A >= t.n_tips and {A, B} == {b, int(t.father()[b])}
        b_tip = B < t.n_tips
        if coef_node == b and clean[i, A] and (b_tip or clean[i, B]):
            shapes.append(None)
            continue
        coef_node = b
        formed += int((clean[i, t.n_tips:] == 0).sum())
        sons = [] if clean[i, A] else [w for w in nbr[A] if w != int(up[i, A])]
        assert clean[i, A] or int(up[i, A]) == B
        if scaled or len(sons) not in (1, 2):      # A resident, or formed by the interpreter first
            variant = 0
        else:
            internal = sorted((w >= t.n_tips for w in sons), reverse=True)      # (the internal son comes first)
            variant = (1 if internal[0] else 2) if len(sons) == 1 else (3 if internal[1] else 4 if internal[0] else 5)
        shapes.append(VARIANT_SHAPES[variant] + (b_tip,))
    return shapes, formed


def test_the_walks_reach_every_instantiation_of_the_contraction_kernel():
    """The shapes the walks below launch, computed from debug_branch_plan (host only; every walk then checks the plan's hits and formed
    partials against the engine's counters): all twelve (NS, S0I, S1I, BTIP) at 60 states (three zero-padded rows) and at 64 (none),
    the three NS == 1 shapes a tree of more than two tips has at every state count, all four at 61."""
    seen = {}
    for w in WALKS:
        pb = _walk_problem(w)
        shapes, _ = _predict(pb, _walk_calls(pb)[0])
        seen.setdefault(w[0], set()).update(s for s in shapes if s is not None)
    for n, s in sorted(seen.items()):
        print(n, sorted(s))
    assert set(seen) == {33, 60, 61, 62, 63, 64}
    for n in (60, 64):
        assert seen[n] == ALL_SHAPES, (n, sorted(ALL_SHAPES - seen[n]))
    assert ONE_SON_SHAPES <= seen[61]
    for n in (33, 62, 63):
        assert ONE_SON_SHAPES - {(1, False, False, True)} <= seen[n], (n, sorted(seen[n]))


@pytest.mark.parametrize("w", WALKS, ids=_walk_id)
def test_eval_branch_walk(w, monkeypatch):
    """Every call of the walk against the oracle (lnL 1e-11 relative, dlnL 1e-9 / 1e-9, ddlnL 1e-9 / 1e-8) and against the P / dP / ddP
    form of the same build (lnL 1e-12 relative); the coefficient hits and the partials formed are those of the plan; afterwards the
    branch-local value at the current length is the tree's lnL."""
    pb = _walk_problem(w)
    t = pb.tree
    calls, br_end = _walk_calls(pb)
    shapes, formed = _predict(pb, calls)
    eng = engine_for(pb)
    monkeypatch.setenv("PAML_AMD_NO_BRANCH_EIG", "1")
    old = engine_for(pb)
    monkeypatch.delenv("PAML_AMD_NO_BRANCH_EIG")
    for i, (b, ts, br) in enumerate(calls):
        t.branch[:] = br
        l, dl, ddl = eng.eval_branch(b, ts, br, pb.gene_rate)
        rl, rdl, rddl = oracle.eval_branch(pb, b, ts)
        ol, odl, oddl = old.eval_branch(b, ts, br, pb.gene_rate)
        where = (i, b, len(ts), shapes[i])
        assert np.allclose(l, rl, rtol=1e-11, atol=0), (where, l, rl)
        assert np.allclose(dl, rdl, rtol=1e-9, atol=1e-9), (where, dl, rdl)
        assert np.allclose(ddl, rddl, rtol=1e-9, atol=1e-8), (where, ddl, rddl)
        assert np.allclose(l, ol, rtol=1e-12, atol=0), (where, l, ol)
        assert np.allclose(dl, odl, rtol=1e-9, atol=1e-9) and np.allclose(ddl, oddl, rtol=1e-9, atol=1e-8), where
    c = eng.branch_counters()
    assert c["n_calls"] == len(calls) and c["coef_hits"] == sum(s is None for s in shapes), (c, shapes)
    assert c["n_nodes"] == formed, (c, formed)
    assert old.branch_counters()["coef_hits"] == 0
    t.branch[:] = br_end
    base = eng.eval(br_end, pb.gene_rate)["lnL"]
    assert abs(base - oracle.evaluate(pb)["lnL"]) <= 1e-10 * abs(base)
    b = calls[len(calls) // 3][0]
    l, _, _ = eng.eval_branch(b, np.array([br_end[b]]), br_end, pb.gene_rate)
    assert abs(l[0] - base) <= 1e-11 * abs(base)


# ---- 2. cherry tables ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("codes64", [False, True])
@pytest.mark.parametrize("n", [60, 62, 64])
def test_cherry_tables(monkeypatch, n, codes64):
    """cherry_table_kernel<false> and the per-tree kernel's lookups off 61 states: two classes, 421 patterns (a ragged last tile), with
    the single-state codes alone and with a table of 64 codes (ambiguity codes where n < 64 leaves room): the bits of the evaluation
    without tables, the oracle's values.  (60 states: the walk's products run 15 k-blocks, and the builder is cherry_table_kernel<false, 15>.)"""
    pb = helpers.random_problem(n, 9, 421, K=2, seed=400 + n)
    if codes64:
        pb = helpers.with_code_table(pb, 64)
        assert pb.n_codes == 64
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit"
    assert used[0] >= 1 and used[1] == pb.K * used[0] * pb.n_codes ** 2 * 512


# ---- 3. the other entry points, one order below and one above 61 -----------------------------------------------------------------------

@pytest.mark.parametrize("n", [60, 63])
def test_eval_batch_matches_single_evals(n):
    """test_engine_gpu.test_eval_batch_matches_single_evals at two classes with ambiguity codes."""
    pb = helpers.random_problem(n, 9, 150, K=2, seed=80 + n, ambiguity=True)
    eng = engine_for(pb)
    rng = np.random.default_rng(5)
    B = 7
    br = np.abs(pb.tree.branch[None, :] * (1 + 0.3 * rng.standard_normal((B, pb.tree.n_nodes))))
    br[0] = pb.tree.branch
    gr = pb.gene_rate[None, :] * (1 + 0.1 * rng.random((B, pb.n_genes)))
    fk = rng.dirichlet(np.ones(pb.K), size=B)
    rt = pb.rate[None, :] * (1 + 0.2 * rng.random((B, pb.K)))
    fk[0], rt[0], gr[0] = pb.freqK, pb.rate, pb.gene_rate
    got = eng.eval_batch(br, gene_rate=gr, freqK=fk, rate=rt)
    assert abs(got[0] - oracle.evaluate(pb)["lnL"]) <= 1e-10 * abs(got[0])
    for b in range(B):
        q = copy.copy(pb)
        q.freqK, q.rate, q.gene_rate = fk[b].copy(), rt[b].copy(), gr[b].copy()
        q.tree = Tree(pb.tree.n_tips, pb.tree.n_nodes, pb.tree.root, pb.tree.sons, br[b].copy(), pb.tree.label)
        ref = oracle.evaluate(q)["lnL"]
        assert abs(got[b] - ref) <= 1e-10 * abs(ref), (b, got[b], ref)
    got2, lnf2 = eng.eval_batch(br, gene_rate=np.tile(pb.gene_rate, (B, 1)), want_lnf=True)
    one = eng.eval(br[3], pb.gene_rate, want_lnf=True)
    assert got2[3] == one["lnL"]
    assert np.array_equal(lnf2[3], one["lnf"])


def _stored_partial(eng, node, ic):
    """get_partials into a buffer with a guard behind it: n values per pattern and nothing of the padded rows n .. 63."""
    import ctypes as C
    size = eng.n_patt * eng.n
    buf = np.full(size + 64 * 8, -7.0)
    rc = eng._L.paml_amd_get_partials(eng._h, int(node), int(ic), buf.ctypes.data_as(C.c_void_p))
    assert rc == 0 and (buf[size:] == -7.0).all()
    return buf[:size].reshape(eng.n_patt, eng.n)


@pytest.mark.parametrize("flags", [KEEP_PARTIALS, KEEP_PARTIALS | JIT], ids=["interpreter", "per_tree_kernel"])
@pytest.mark.parametrize("n", [60, 63])
def test_keep_partials_and_dirty_eval(n, flags):
    """Every internal node's stored partial against the oracle's (1e-11 relative), then a dirty evaluation after one tip branch moved,
    on the interpreter (with scaling nodes) and on the per-tree kernel."""
    kw = dict(K=2, seed=31 + n, scale_every=None if flags & JIT else 3)
    pb = helpers.random_problem(n, 9, 150, **kw)
    ref = oracle.evaluate(pb, want_partials=True)
    eng, out, _ = check(pb, flags=flags)
    assert (eng.kernel_name == "mfma64_jit") == bool(flags & JIT), eng.kernel_name
    t = pb.tree
    for node in range(t.n_tips, t.n_nodes):
        for ic in range(pb.K):
            got = _stored_partial(eng, node, ic)
            assert got.shape == ref["partials"][ic, node - t.n_tips].shape == (pb.n_patt, n)
            assert np.allclose(got, ref["partials"][ic, node - t.n_tips], rtol=1e-11, atol=1e-300), (node, ic)
            assert np.array_equal(got, eng.get_partials(node, ic))
    if pb.scale_node is not None:
        assert pb.scale_node.sum() >= 1
        for k, node in enumerate(np.nonzero(pb.scale_node)[0]):
            assert np.allclose(eng.get_scale(int(node), 1), ref["scalef"][1, k], rtol=1e-12)
    father = t.father()
    tip = 3
    br = t.branch.copy()
    br[tip] *= 1.7
    clean = np.ones(t.n_nodes, dtype=np.uint8)
    node = tip
    while node != -1:
        clean[node] = 0
        node = father[node]
    lnl_dirty = eng.eval_dirty(br, clean, pb.gene_rate)
    pb2 = helpers.random_problem(n, 9, 150, **kw)
    pb2.tree.branch[:] = br
    ref2 = oracle.evaluate(pb2, want_partials=True)
    assert abs(lnl_dirty - ref2["lnL"]) <= 1e-10 * abs(ref2["lnL"])
    for node in range(t.n_tips, t.n_nodes):      # the recomputed path and the nodes left alone
        assert np.allclose(_stored_partial(eng, node, 1), ref2["partials"][1, node - t.n_tips], rtol=1e-11, atol=1e-300), node


@pytest.mark.parametrize("n", [60, 63])
def test_node_posterior_matches_oracle(n):
    pb = helpers.random_problem(n, 9, 140, K=2, seed=51 + n, ambiguity=True)
    eng = engine_for(pb)
    base = eng.eval(pb.tree.branch, pb.gene_rate)["lnL"]
    for node in (pb.tree.root, pb.tree.n_nodes - 1):
        got = eng.node_posterior(node, pb.tree.branch, pb.gene_rate)
        ref = oracle.node_posterior(pb, node)
        assert got.shape == (pb.n_patt, n)
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-13), (node, float(np.max(np.abs(got - ref))))
        assert np.allclose(got.sum(axis=1), 1)
    assert eng.eval(pb.tree.branch, pb.gene_rate)["lnL"] == base


@pytest.mark.parametrize("n", [60, 63])
def test_ancestral_marginal(n):
    _check_marginal(helpers.random_problem(n, 9, 140, K=2, seed=151 + n, ambiguity=True))


@pytest.mark.parametrize("n", [60, 63])
def test_ancestral_joint(n):
    _check_joint(helpers.random_problem(n, 9, 140, seed=190 + n, ambiguity=True))
