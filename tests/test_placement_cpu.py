"""The yardstick of the placement tests (tests/placement_ref.py) and the host-only parts pinned on the CPU, before any GPU run: the
restatement's lnf of every (query, edge, pendant) against oracle.evaluate of the problem on the enlarged tree at 1e-9 (the NNI tests' bound
for lnf; measured: see the tests' output, about 1e-14), Tree.insert_tip's trees, the arithmetic the GPU batching tests rely on, and the C
host's loading of a tree that names only some of the sequences."""
import os

import numpy as np
import pytest

import helpers
import gradient_ref as gr
import nni_ref as nr
import placement_ref as pr
import oracle
from paml_amd.problem import balanced_tree

CTL = os.path.join(helpers.GOLDEN, "ctl")
PHI, PENDANT = 0.3, (0.05, 0.4)


def _restatement_against_the_oracle(pb, scale_every=None, phi=PHI, pendant=PENDANT, label=0):
    queries = pr.queries_of(pb, seed=1)
    got = pr.placement_scores_of(pb, queries, phi, pendant, label)
    ref0 = oracle.evaluate(pb)
    assert np.max(np.abs(got["lnf0"] - ref0["lnf"])) <= 1e-9
    assert len(got["edges"]) == pb.tree.n_nodes - 1
    worst = 0.0
    for qi in range(len(queries)):
        for i, v in enumerate(got["edges"]):
            for j, tau in enumerate(pendant):
                ref = oracle.evaluate(pr.inserted_problem(pb, v, phi, tau, queries[qi], label, scale_every))
                worst = max(worst, float(np.max(np.abs(got["lnf"][qi, i, j] - ref["lnf"]))))
    print("%d queries x %d edges x %d pendants: largest |lnf - oracle| %.3e" % (len(queries), len(got["edges"]), len(pendant), worst))
    assert worst <= 1e-9
    return len(queries)


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracle_on_the_enlarged_tree(name):
    pb = gr.reversible_problem(name)
    n_q = _restatement_against_the_oracle(pb, nr.scale_every_of(name))
    assert n_q == (3 if pb.n_codes > pb.n else 2)      # (the all-"missing" query where the table has that code)


def _trees():
    out = [gr.reversible_problem(s[0]).tree for s in gr.REVERSIBLE_SHAPES]
    out += [balanced_tree(k) for k in (4, 5, 8, 13)]
    out.append(helpers.random_problem(4, 30, 4, seed=9).tree)
    return out


def test_insert_tip_keeps_a_tree():
    rng = np.random.default_rng(4)
    for t in _trees():
        t.label = rng.integers(0, 3, t.n_nodes).astype(np.int32)
        f = t.father()
        for v in range(t.n_nodes):
            if v == t.root:
                continue
            q = t.insert_tip(v, 0.3, 0.25, label=2)
            assert q.n_tips == t.n_tips + 1 and q.n_nodes == t.n_nodes + 2
            new = lambda i: i if i < t.n_tips else i + 1
            u = q.n_nodes - 1
            assert q.root == new(t.root)
            # every node has one father; every node is reached from the root; the tips are 0 .. n_tips
            count = np.zeros(q.n_nodes, dtype=int)
            for a in range(q.n_nodes):
                for c in q.sons[a]:
                    count[c] += 1
            assert count[q.root] == 0 and (np.delete(count, q.root) == 1).all()
            seen, stack = 0, [q.root]
            while stack:
                a = stack.pop()
                seen += 1
                stack.extend(q.sons[a])
            assert seen == q.n_nodes
            assert [a for a in range(q.n_nodes) if not q.sons[a]] == list(range(q.n_tips))
            # u takes v's place in the father's list; its sons are (v, the new tip)
            assert q.sons[u] == [new(v), t.n_tips]
            assert q.sons[new(int(f[v]))] == [u if c == v else new(int(c)) for c in t.sons[int(f[v])]]
            # the two halves sum to t_v, the labels are kept, every other branch is untouched
            assert abs(q.branch[u] + q.branch[new(v)] - t.branch[v]) <= 1e-15 * max(1.0, t.branch[v])
            assert q.branch[new(v)] == 0.3 * t.branch[v] and q.branch[t.n_tips] == 0.25
            assert q.label[u] == t.label[v] == q.label[new(v)] and q.label[t.n_tips] == 2
            for a in range(t.n_nodes):
                if a != v:
                    assert q.branch[new(a)] == t.branch[a] and q.label[new(a)] == t.label[a]
        with pytest.raises(ValueError):
            t.insert_tip(t.root, 0.5, 0.1)
        for phi in (-0.01, 1.01, float("nan")):
            with pytest.raises(ValueError):
                t.insert_tip(0 if t.root != 0 else 1, phi, 0.1)


def test_one_mebibyte_cannot_hold_the_batching_cases():
    """The GPU batching tests rely on it.  The bytes a pattern takes in the workspace, as DESIGN 4 W documents them: 2 K n_int (n_s + 1)
    doubles for the down partials and the outer messages (n_s = 64 on the matrix cores), 2 K + 1 doubles for the present tree, then
    2 K + 1 doubles (f_hk and its log factor per class, lnf) per row = (edge of the group, query, pendant)."""
    K, n_int, n_edges, n_patt = 1, 9 - 2, 2 * 9 - 3, 3000      # (an unrooted binary tree of 9 tips has 7 internal nodes and 15 branches)
    fixed, row = 2 * K * n_int * (64 + 1) * 8 + (2 * K + 1) * 8, (2 * K + 1) * 8
    # case A: 3 queries, all 15 edges, 2 pendants: batches of patterns, every row in one group
    per_patt = fixed + 3 * n_edges * 2 * row
    assert fixed >= 2 * 7 * 65 * 8 and n_patt * per_patt > 1 << 20
    assert 64 * per_patt <= 1 << 20
    # case B: 8 queries x 15 edges x 4 pendants: one tile with all rows does not fit, one tile with one edge's rows does
    assert 64 * (fixed + 8 * n_edges * 4 * row) > 1 << 20
    assert 64 * (fixed + 8 * 4 * row) <= 1 << 20


# ---- the C host: a tree that names only some of the sequences (all on the CPU) ----------------------------------------------------------------

BROWN = os.path.join(helpers.GOLDEN, "data", "brown.nuc")
K80_TEXT = "seqfile = %s\ntreefile = %s\nmodel = 1\nfix_kappa = 1\nkappa = 2.5\nfix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\n"
TREE4 = "((Human: 0.1, Chimpanzee: 0.2): 0.15, Orangutan: 0.4, Gibbon: 0.5);"      # Gorilla, the third of the file's five, is the query


def _brown_sequences():
    toks = open(BROWN).read().split()
    ns, ls = int(toks[0]), int(toks[1])
    seqs, i = [], 2
    for _ in range(ns):
        name, i, s = toks[i], i + 1, ""
        while len(s) < ls:
            s, i = s + toks[i], i + 1
        seqs.append((name, s))
    return seqs


def _analysis(tmp_path, name, newick, seqfile=BROWN, placement=False, n_tips=None):
    from paml_amd import hostlib
    tree = tmp_path / (name + ".trees")
    tree.write_text(newick + "\n" if n_tips is None else "%d 1\n%s\n" % (n_tips, newick))
    ctl = tmp_path / (name + ".ctl")
    ctl.write_text(K80_TEXT % (seqfile, tree))
    return hostlib.Analysis(str(ctl), "baseml", placement=placement)


def test_host_loads_a_tree_that_leaves_a_sequence_out(tmp_path):
    a = _analysis(tmp_path, "place", TREE4, placement=True)
    assert (a.n_tips, a.n_queries, a.query_names()) == (4, 1, ["Gorilla"])
    assert a.seq_names() == ["Human", "Chimpanzee", "Orangutan", "Gibbon"]
    pa = a.problem(np.array(a.default_x()))
    assert pa.weights.sum() == 895 and a.query_codes().shape == (1, a.n_patt) and a.query_codes().max() < 4
    # the same tree and options on a file that holds the four sequences only
    four = tmp_path / "four.nuc"
    seqs = [s for s in _brown_sequences() if s[0] != "Gorilla"]
    four.write_text("4 895\n" + "".join("%s\n%s\n" % s for s in seqs))
    b = _analysis(tmp_path, "four", TREE4, seqfile=str(four))
    assert b.n_tips == 4 and b.n_queries == 0 and b.np == a.np and list(b.default_x()) == list(a.default_x())
    x = np.array(a.default_x())
    la, lb = oracle.evaluate(a.problem(x))["lnL"], oracle.evaluate(b.problem(x))["lnL"]
    print("lnL of the four-sequence tree: placement load %.10f, ordinary load %.10f" % (la, lb))
    assert abs(la - lb) <= 1e-10 * abs(lb)
    # patterns that differ only in the query stay apart: more patterns than the four sequences alone make
    assert a.n_patt > b.n_patt
    # the tree's sequences by number in file order
    c = _analysis(tmp_path, "numbers", "((1: 0.1, 2: 0.2): 0.15, 4: 0.4, 5: 0.5);", placement=True)
    assert c.seq_names() == a.seq_names() and c.query_names() == ["Gorilla"] and np.array_equal(c.query_codes(), a.query_codes())
    with pytest.raises(RuntimeError, match="at least 3"):
        _analysis(tmp_path, "two", "(Human: 0.1, Gibbon: 0.2);", placement=True)


def test_host_placement_equals_the_five_taxon_analyses(tmp_path):
    """The restatement on the placement analysis's problem and query codes, every edge at phi = 0.5 and a pendant of 0.1, against the CPU
    oracle on ordinary five-sequence analyses loaded from the trees pamlh_placement_newick writes."""
    a = _analysis(tmp_path, "place", TREE4, placement=True)
    x = np.array(a.default_x())
    pa = a.problem(x)
    order = a.branch_order()
    got = pr.placement_scores_of(pa, a.query_codes(), 0.5, (0.1,), edges=order)
    assert len(order) == 5
    for b, v in enumerate(order):
        nw = a.placement_newick(0, b, 0.5, 0.1)
        assert nw.count("Gorilla") == 1 and nw.count("(") == 3
        five = _analysis(tmp_path, "five%d" % b, nw, n_tips=5)
        assert five.n_tips == 5 and five.n_queries == 0
        ref = oracle.evaluate(five.problem(np.array(five.default_x())))["lnL"]
        print("branch above node %d: restatement %.9f, five-sequence analysis %.9f\n  %s" % (v, got["lnL"][0, b, 0], ref, nw))
        assert abs(got["lnL"][0, b, 0] - ref) <= 1e-8
    with pytest.raises(RuntimeError, match="branch 5 of 5"):
        a.placement_newick(0, 5, 0.5, 0.1)
    with pytest.raises(RuntimeError, match="query 1 of 1"):
        a.placement_newick(1, 0, 0.5, 0.1)


@pytest.mark.parametrize("ctl,word", [("brown_hky85_clock.ctl", "clock"), ("brown_hky85_adg.ctl", "rho"), ("brown_hky85.ctl", "no queries")])
def test_host_refuses_clocks_rho_models_and_an_analysis_without_queries_by_name(ctl, word):
    """Before anything reaches the engine: pamlh_placement_scores and pamlh_place alike."""
    from paml_amd import hostlib
    a = hostlib.Analysis(os.path.join(CTL, ctl), "baseml", placement=True)
    assert a.n_queries == 0
    x = np.array(a.default_x())
    for call in (lambda: a.placement_scores(x), lambda: a.place(x)):
        with pytest.raises(RuntimeError, match=word):
            call()
