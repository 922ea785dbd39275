"""The yardstick of the edge-score tests (tests/edge_ref.py) and the host-only parts pinned on the CPU, before any GPU run.  The
restatement's lnf of every configuration of every edge at random override lengths against oracle.evaluate of the rearranged problem
with the lengths written into its tree, at 1e-9 (the gradient tests' bound for lnf); on the exactly reversible shapes its d1 and d2
against oracle.eval_branch of the rearranged problem at the row's length (rtol 1e-9, atol 1e-9: the gradient tests' TOL); the list of
edges in Python against paml_amd_edge_list; the arithmetic the GPU batching test relies on."""
import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import edge_ref as er
import gradient_ref as gr
import nni_ref as nr
import oracle
from paml_amd import engine
from paml_amd.problem import balanced_tree
from test_gradient_cpu import _irreversible_cases

TOL = dict(rtol=1e-9, atol=1e-9)


def _restatement_against_the_oracle(pb, scale_every=None, derivatives=True):
    t = pb.tree
    rows, on, ot = er.all_rows(t, seed=11)
    assert len(rows) >= 15
    got = er.edge_scores(pb, ar.matrices_from_oracle(pb), rows, on, ot)
    assert np.max(np.abs(got["lnf0"] - oracle.evaluate(pb)["lnf"])) <= 1e-9
    worst, worst_d = 0.0, 0.0
    for i0 in range(0, len(rows), 5):      # (the five roles of one edge and configuration share their lengths)
        v, s, x, _ = rows[i0]
        q = er.rearranged_problem(pb, v, s, x, on[i0], ot[i0], scale_every)
        ref = oracle.evaluate(q)
        for i in range(i0, i0 + 5):
            worst = max(worst, float(np.max(np.abs(got["lnf"][i] - ref["lnf"]))))
            if derivatives:
                u = int(rows[i][3])
                _, dl, ddl = oracle.eval_branch(q, u, np.array([q.tree.branch[u]]))
                worst_d = max(worst_d, abs(got["d1"][i] - dl[0]), abs(got["d2"][i] - ddl[0]))
                assert np.allclose(got["d1"][i], dl[0], **TOL), (i, rows[i], got["d1"][i], dl[0])
                assert np.allclose(got["d2"][i], ddl[0], **TOL), (i, rows[i], got["d2"][i], ddl[0])
    print("%d rows: largest |lnf - oracle| %.3e; largest |d - oracle| %.3e" % (len(rows), worst, worst_d))
    assert worst <= 1e-9


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracle_on_the_rearranged_tree(name):
    _restatement_against_the_oracle(gr.reversible_problem(name), nr.scale_every_of(name))


@pytest.mark.parametrize("name", [c[0] for c in _irreversible_cases()])
def test_restatement_lnf_equals_the_oracle_on_irreversible_models(name):
    """(the branch-local derivative of the oracle re-roots the tree: no reference for d1 and d2 here)"""
    _restatement_against_the_oracle(dict(_irreversible_cases())[name](), derivatives=False)


def test_u_minus_one_gives_zero_derivatives_and_the_same_lnf():
    pb = gr.reversible_problem("5-K1")
    rows, on, ot = er.all_rows(pb.tree, seed=3)
    P = ar.matrices_from_oracle(pb)
    a = er.edge_scores(pb, P, rows[:5], on[:5], ot[:5])
    r0 = rows[:5].copy()
    r0[:, 3] = -1
    b = er.edge_scores(pb, P, r0, on[:5], ot[:5])
    assert np.array_equal(a["lnf"], b["lnf"]) and not b["d1"].any() and not b["d2"].any()


def _trees():
    out = [gr.reversible_problem(s[0]).tree for s in gr.REVERSIBLE_SHAPES]      # (binary trees and the polytomy tree)
    out += [c[1]().tree for c in _irreversible_cases()]                         # (two of them rooted at a tip)
    out += [balanced_tree(k) for k in (4, 5, 8, 13)]
    out.append(helpers.random_problem(4, 30, 4, seed=9).tree)
    t = balanced_tree(8)
    if len(t.sons[t.root]) == 3:      # a root with two sons: the root's last two sons under a new node
        sons = [list(s) for s in t.sons] + [list(t.sons[t.root][1:])]
        sons[t.root] = [t.sons[t.root][0], t.n_nodes]
        t = type(t)(t.n_tips, t.n_nodes + 1, t.root, sons, np.append(t.branch, 0.1), np.append(t.label, 0))
    out.append(t)
    return out


def test_python_list_equals_the_librarys():
    two_son_root = polytomy = tip_root = 0
    for t in _trees():
        lib_edges, lib_five = engine.edge_list(t)
        edges, five = t.edge_configs()
        assert edges.dtype == np.int32 and edges.shape == lib_edges.shape and np.array_equal(edges, lib_edges)
        assert five.shape == lib_five.shape and np.array_equal(five, lib_five)
        f = t.father()
        swaps = {tuple(int(c) for c in sw) for sw in t.nni_swaps()}
        for e in range(len(edges)):
            v = int(edges[e][0][0])
            assert tuple(edges[e][0]) == (v, -1, -1) and v != t.root and len(t.sons[v]) == 2
            assert tuple(edges[e][1]) in swaps and tuple(edges[e][2]) in swaps and tuple(edges[e][1]) != tuple(edges[e][2])
            allowed = set(t.sons[v]) | {v} | (set(t.sons[f[v]]) - {v}) | ({int(f[v])} if f[v] != t.root else set())
            assert set(int(c) for c in five[e]) == allowed and len(allowed) == 5
        binary = len(t.sons[t.root]) == 3 and all(len(t.sons[v]) in (0, 2) for v in range(t.n_nodes) if v != t.root)
        if binary:
            assert len(edges) == t.n_tips - 3
        two_son_root += len(t.sons[t.root]) == 2
        tip_root += t.root < t.n_tips
        polytomy += len(t.sons[t.root]) > 3 or any(len(t.sons[v]) > 2 for v in range(t.n_nodes) if v != t.root)
        if len(t.sons[t.root]) == 2:      # no edge under a root with two sons
            assert all(f[int(e[0][0])] != t.root for e in edges)
    assert two_son_root >= 1 and polytomy >= 1 and tip_root >= 2


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, one class, all 90 rows.  The bytes a pattern takes in the
    workspace: 2 K n_int (n_s + 1) doubles for the down partials and the outer messages (n_s = 64 on the matrix cores), then 4 K + 3
    doubles (f, f', f'' and their log factor per class; lnf, g1, g2) per row and for the present tree."""
    K, n_int, n_rows, n_patt = 1, 9 - 2, 15 * (9 - 3), 3000
    per_patt = 2 * K * n_int * (64 + 1) * 8 + (n_rows + 1) * (4 * K + 3) * 8
    assert n_patt * per_patt > 1 << 20
    assert 64 * per_patt <= 1 << 20      # (and one tile with all rows fits: the patterns are walked in batches, not the rows in groups)


# ---- the host side: the table arithmetic, the refusals, the numpy coordinate ascent ----------------------------------------------------------

def supports_restated(rep, l3):
    """pamlh_branch_supports_from_replicates in numpy: (delta, support).  The means are added in replicate order, as the C loop adds them."""
    rep, l3 = np.asarray(rep, dtype=np.float64), np.asarray(l3, dtype=np.float64).reshape(-1, 3)
    n_rep, n = rep.shape[0], len(l3)
    delta = 2 * (l3[:, 0] - np.maximum(l3[:, 1], l3[:, 2]))
    mean = np.add.accumulate(rep, axis=0)[-1] / n_rep
    c = np.sort((rep - mean[None, :]).reshape(n_rep, n, 3), axis=2)
    dstar = 2 * (c[:, :, 2] - c[:, :, 1])
    support = (dstar < delta[None, :]).sum(axis=0) / n_rep
    support[~(delta > 0)] = 0
    return delta, support


def test_table_arithmetic_equals_its_restatement_on_random_replicates():
    from paml_amd import hostlib
    rng = np.random.default_rng(5)
    for n_edges, n_rep in [(1, 1), (3, 7), (6, 1000)]:
        rep = rng.normal(-2500.0, 30.0, (n_rep, 3 * n_edges)) + rng.normal(0, 4.0, (1, 3 * n_edges))
        l3 = rng.normal(-2500.0, 3.0, (n_edges, 3))
        l3[0, 0] = l3[0].max() + 1.5      # (a supported edge)
        if n_edges > 1:
            l3[1, 0] = l3[1, 1:].max() - 0.5      # (delta < 0: a better neighbour exists)
        delta, sup = hostlib.branch_supports_from_replicates(rep, l3)
        d_ref, s_ref = supports_restated(rep, l3)
        assert np.array_equal(delta, d_ref) and np.array_equal(sup, s_ref), (sup, s_ref)
        assert ((sup >= 0) & (sup <= 1)).all() and (sup[delta <= 0] == 0).all()
    assert sup.max() > 0


def test_table_arithmetic_counts_with_a_strict_inequality_and_gives_zero_at_delta_zero():
    """Integer replicate sums whose columns add up to 0 (the centring is exact): edge 0 has delta equal to one of its delta*_r, which
    therefore does not count; edge 1 has delta = 0 and edge 2 delta < 0: support 0."""
    from paml_amd import hostlib
    rng = np.random.default_rng(8)
    rep = rng.integers(-9, 10, (7, 9)).astype(np.float64)
    rep = np.vstack([rep, -rep.sum(axis=0)])
    c = np.sort(rep.reshape(8, 3, 3), axis=2)
    dstar = 2 * (c[:, :, 2] - c[:, :, 1])
    tie = float(np.sort(dstar[:, 0])[4])
    l3 = np.array([[tie / 2, 0.0, -1.0], [3.0, 3.0, 1.0], [2.0, 1.0, 4.0]])
    delta, sup = hostlib.branch_supports_from_replicates(rep, l3)
    assert np.array_equal(delta, [tie, 0.0, -4.0])
    assert sup[0] == (dstar[:, 0] < tie).sum() / 8 and sup[0] < (dstar[:, 0] <= tie).sum() / 8
    assert sup[1] == 0 and sup[2] == 0
    assert np.array_equal(sup, supports_restated(rep, l3)[1])


@pytest.mark.parametrize("ctl,word", [("brown_hky85_clock.ctl", "clock"), ("brown_hky85_adg.ctl", "rho")])
def test_host_refuses_clocks_and_rho_models_by_name(ctl, word):
    """Before anything reaches the engine: pamlh_edge_list, pamlh_edge_optimize and pamlh_branch_supports alike."""
    import os
    from paml_amd import hostlib
    a = hostlib.Analysis(os.path.join(helpers.GOLDEN, "ctl", ctl), "baseml")
    x = np.array(a.default_x())
    for call in (lambda: a.edge_list(), lambda: a.edge_optimize(x, np.zeros((1, 3, 3)), np.zeros((1, 5))), lambda: a.branch_supports(x)):
        with pytest.raises(RuntimeError, match=word):
            call()


def test_host_refuses_fixed_branch_lengths_and_a_root_with_two_sons(tmp_path):
    import os
    from paml_amd import hostlib
    text = "seqfile = %s\ntreefile = %s\nmodel = 4\nfix_kappa = 0\nkappa = 5\nfix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\n%s"
    seq = os.path.join(helpers.GOLDEN, "data", "brown.nuc")
    for name, newick, extra, word in [("fixed", "((Human: 0.1, Chimpanzee: 0.1): 0.1, Gorilla: 0.1, (Orangutan: 0.1, Gibbon: 0.1): 0.1);", "fix_blength = 2\n", "fix_blength = 2"),
                                      ("rooted", "((Human, Chimpanzee), (Gorilla, (Orangutan, Gibbon)));", "", "the root has two sons")]:
        tree = tmp_path / (name + ".trees")
        tree.write_text("5 1\n%s\n" % newick)
        ctl = tmp_path / (name + ".ctl")
        ctl.write_text(text % (seq, tree, extra))
        a = hostlib.Analysis(str(ctl), "baseml")
        with pytest.raises(RuntimeError, match=word):
            a.branch_supports(np.array(a.default_x()))


def test_numpy_coordinate_ascent_ends_at_a_stationary_point():
    """The yardstick of the host test on the problem it is used on (brown.nuc, HKY85, at the control file's initial values): every
    configuration's lnL rises from its start, and at the end, along every one of the five branches, either the gain Newton's step would
    still predict, d1^2 / (2 |d2|), is below 1e-8 (ten times the tolerance the sweeps end at) or the derivative points out of a bound."""
    import os
    from paml_amd import hostlib
    a = hostlib.Analysis(os.path.join(helpers.GOLDEN, "ctl", "brown_hky85.ctl"), "baseml")
    pb = a.problem(np.array(a.default_x()))
    P = ar.matrices_from_oracle(pb)
    passes = er.tree_passes(pb, P)
    edges, five = pb.tree.edge_configs()
    assert len(edges) == 2
    for e in range(len(edges)):
        for cfg in edges[e]:
            start = er.edge_scores(pb, P, [list(cfg) + [-1]], [five[e]], [pb.tree.branch[five[e]]], passes=passes)["lnL"][0]
            t5, l = er.coordinate_ascent(pb, P, cfg, five[e], passes=passes)
            assert l >= start
            for u in five[e]:
                r = er.edge_scores(pb, P, [list(cfg) + [int(u)]], [five[e]], [t5], passes=passes)
                tu = t5[list(five[e]).index(u)]
                left = r["d1"][0] ** 2 / (2 * abs(r["d2"][0]))
                assert abs(r["lnL"][0] - l) <= 1e-9 and (left <= 1e-8 or (tu <= 4e-6 and r["d1"][0] < 0) or (tu >= 50 and r["d1"][0] > 0)), (cfg, u, r["d1"][0], left)
