"""The yardstick of the relabel tests (tests/relabel_ref.py) pinned on the CPU, before any GPU run: the restatement's lnf and class values
of every (non-root node, label) row against oracle.evaluate of the relabelled problem at 1e-9 (the NNI tests' bound for lnf; measured:
see the tests' output, about 1e-14), Tree.relabelled's trees, and the arithmetic the GPU batching test relies on; then the host parts that
need no engine: pamlh_mixture_max on the lysozyme classes and on synthetic ones, pamlh_foreground_point as an exact point of model A,
pamlh_set_foreground with pamlh_newick, and the host's refusals by name."""
import copy
import os
import re

import numpy as np
import pytest

import helpers
import oracle
import relabel_ref as rr
from paml_amd import hostlib
from test_ancestral_gpu import _rooted_at_tip0


def _restatement_against_the_oracle(pb):
    rows = rr.all_rows(pb.tree, pb.n_labels)
    assert len(rows) == (pb.tree.n_nodes - 1) * pb.n_labels
    got = rr.relabel_scores_of(pb, rows)
    live = pb.weights > 0
    ref0 = oracle.evaluate(pb, want_fhk=True)
    assert np.max(np.abs(got["lnf0"] - ref0["lnf"])[live]) <= 1e-9
    assert np.max(np.abs(got["lnfk0"] - rr.oracle_class_logs(pb, ref0))[:, live]) <= 1e-9
    worst, worst_k, changed = 0.0, 0.0, 0
    for i, (v, l) in enumerate(rows):
        ref = oracle.evaluate(rr.relabelled_problem(pb, v, l), want_fhk=True)
        worst = max(worst, float(np.max(np.abs(got["lnf"][i] - ref["lnf"])[live])))
        rk = rr.oracle_class_logs(pb, ref)
        fin = np.isfinite(rk) & live[None, :]
        worst_k = max(worst_k, float(np.max(np.abs(got["lnfk"][i] - rk)[fin])))
        changed += bool(np.max(np.abs(ref["lnf"] - ref0["lnf"])[live]) > 1e-6)
    print("%d rows (%d move lnf): largest |lnf - oracle| %.3e, |log fhK - oracle| %.3e" % (len(rows), changed, worst, worst_k))
    assert worst <= 1e-9 and worst_k <= 1e-9
    assert changed >= len(rows) // 3      # (the labels do select different models: the rows are no copies of the present tree)


@pytest.mark.parametrize("n,K,genes", rr.LABEL_SHAPES)
def test_restatement_equals_the_oracle_on_the_relabelled_tree(n, K, genes):
    _restatement_against_the_oracle(rr.label_problem(n, K, genes))


@pytest.mark.parametrize("name", rr.REVERSIBLE_NAMES)
def test_restatement_with_ambiguity_codes_a_polytomy_and_scaling_marks(name):
    _restatement_against_the_oracle(rr.labelled_reversible_problem(name))


def test_restatement_on_a_tree_rooted_at_a_tip():
    _restatement_against_the_oracle(_rooted_at_tip0(rr.label_problem(4, 2, 1, seed=57)))


def test_relabelled_changes_one_label_and_shares_the_rest():
    t = rr.label_problem(4, 2, 1).tree
    for v in range(t.n_nodes):
        if v == t.root:
            continue
        q = t.relabelled(v, 2)
        assert q.label[v] == 2 and np.array_equal(np.delete(q.label, v), np.delete(t.label, v))
        assert q.label is not t.label and q.sons is t.sons and q.branch is t.branch and q.root == t.root
    for bad in (t.root, -1, t.n_nodes):
        with pytest.raises(ValueError):
            t.relabelled(bad, 0)


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, two classes, all 15 x 3 rows.  The bytes a pattern takes
    in the workspace, as DESIGN 4 AD documents them: 2 K n_int (n_s + 1) doubles for the down partials and the outer messages (n_s = 64
    on the matrix cores), then 3 K + 1 doubles (f_hk, its log factor and lnfk per class, lnf) per row and for the present tree."""
    K, n_int, n_rows, n_patt = 2, 9 - 2, (2 * 9 - 3) * 3, 3000      # (an unrooted binary tree of 9 tips: 7 internal nodes, 15 branches)
    fixed, per_row = 2 * K * n_int * (64 + 1) * 8, (3 * K + 1) * 8
    assert n_patt * (fixed + per_row * (n_rows + 1)) > 1 << 20      # several batches
    assert 64 * (fixed + per_row * (n_rows + 1)) > 1 << 20          # and one tile with all rows does not fit either: groups of rows
    assert 64 * (fixed + per_row * 2) <= 1 << 20                    # (one tile with one row and the present tree does)


# ---- the host: the mixture over the site-class proportions, the parameter vector of a row, the relabelled tree ------------------------------------

CTL = os.path.join(helpers.GOLDEN, "ctl")


def _lyso():
    g = helpers.load_golden("lyso_bsa")
    a = hostlib.Analysis(os.path.join(CTL, "lyso_bsa.ctl"), "codeml")
    return g, a, np.array(g["x"])


def _class_logs_at_effective_lengths(pb, tau, node):
    """[4][n_patt]: the logs of model A's class likelihoods f0, f1, f2a, f2b with `node` the only foreground branch, at the lengths tau
    and every Qfactor 1: one oracle evaluation."""
    q = copy.copy(pb)
    lab = np.zeros(pb.tree.n_nodes, dtype=np.int32)
    lab[node] = 1
    q.tree = type(pb.tree)(pb.tree.n_tips, pb.tree.n_nodes, pb.tree.root, pb.tree.sons, np.ascontiguousarray(tau), lab)
    q.qfactor = np.ones_like(pb.qfactor)
    return rr.oracle_class_logs(q, oracle.evaluate(q, want_fhk=True))


def _mixture(w, f4, p0, p1):
    s, r = p0 + p1, p0 / (p0 + p1)
    pr = np.array([s * r, s * (1 - r), (1 - s) * r, (1 - s) * (1 - r)])
    mx = f4.max(axis=0)
    return float(np.dot(w, mx + np.log((pr[:, None] * np.exp(f4 - mx)).sum(axis=0))))


@pytest.fixture(scope="module")
def lyso_classes():
    """The golden's foreground branch, its point, and the class values at the golden's effective lengths (computed once)."""
    g, a, x = _lyso()
    pb = a.problem(x)
    fg = np.flatnonzero(pb.tree.label == 1)
    assert list(fg) == [21]
    tau = pb.tree.branch * pb.qfactor[0][pb.tree.label]
    return dict(g=g, a=a, x=x, pb=pb, node=21, f4=_class_logs_at_effective_lengths(pb, tau, 21))


def test_mixture_max_on_the_lysozyme_classes(lyso_classes):
    c = lyso_classes
    w, f4, pb = c["pb"].weights, c["f4"], c["pb"]
    gp0, gp1 = float(pb.freqK[0]), float(pb.freqK[1])
    at_golden = _mixture(w, f4, gp0, gp1)
    assert abs(at_golden - oracle.evaluate(pb)["lnL"]) <= 1e-9 * w.sum()      # (the fixed-f mixture is the model's lnL at the golden's point)
    starts = [(0.55, 0.55), (0.9, 0.3), (gp0 + gp1, gp0 / (gp0 + gp1))]
    got = [hostlib.mixture_max(w, f4, s0, r0) for s0, r0 in starts]
    mid = (np.arange(40) + 0.5) / 40
    grid = max(_mixture(w, f4, s * r, s * (1 - r)) for s in mid for r in mid)
    print("lnL from three starts: %r; spread %.3e; above the 40 x 40 grid by %.3e; above the golden's proportions by %.3e"
          % ([r["lnL"] for r in got], max(r["lnL"] for r in got) - min(r["lnL"] for r in got), min(r["lnL"] for r in got) - grid, min(r["lnL"] for r in got) - at_golden))
    assert max(r["lnL"] for r in got) - min(r["lnL"] for r in got) <= 1e-9
    for r in got:
        assert r["lnL"] >= grid and r["lnL"] >= at_golden
        assert abs(r["lnL"] - _mixture(w, f4, r["p0"], r["p1"])) <= 1e-9 * w.sum()      # (the value is the mixture at the proportions returned)


def test_mixture_max_with_an_impossible_class_and_at_the_edge_of_the_box():
    rng = np.random.default_rng(4)
    n = 50
    w = rng.integers(1, 5, n).astype(np.float64)
    w[7] = 0
    f4 = np.log(rng.random((4, n))) - 30
    f4[2, 3] = -np.inf
    f4[:, 7] = -np.inf      # (weight 0: never looked at)
    r = hostlib.mixture_max(w, f4, 0.5, 0.5)
    mid = (np.arange(40) + 0.5) / 40
    with np.errstate(divide="ignore"):
        live = w > 0
        grid = max(_mixture(w[live], f4[:, live], s * q, s * (1 - q)) for s in mid for q in mid)
        assert np.isfinite(r["lnL"]) and r["lnL"] >= grid
        assert abs(r["lnL"] - _mixture(w[live], f4[:, live], r["p0"], r["p1"])) <= 1e-9 * w.sum()
    # the foreground classes are worse at every pattern: the maximum is at s = 1 - 1e-6
    f4 = np.log(rng.random((4, n)))
    f4[2:] = f4[:2] - 1.0
    for s0, r0 in ((0.3, 0.5), (0.999, 0.2)):
        r = hostlib.mixture_max(w, f4, s0, r0)
        assert abs(r["p0"] + r["p1"] - (1 - 1e-6)) <= 1e-12, r
    with pytest.raises(RuntimeError):
        bad = f4.copy()
        bad[:, 0] = -np.inf
        hostlib.mixture_max(w, bad)


def test_foreground_point_is_an_exact_point_of_model_a(lyso_classes):
    """The golden's node and w2 with other proportions: the model's own lnL at the vector equals the mixture of the class values taken
    at the effective lengths tau = t Qfactor_bg(r_x) of every branch."""
    c = lyso_classes
    a, x, pb, node = c["a"], c["x"], c["pb"], c["node"]
    w2 = float(x[-1])
    f4 = _class_logs_at_effective_lengths(pb, pb.tree.branch * pb.qfactor[0][0], node)
    xa = a.foreground_point(x, node, w2, 0.48, 0.32)
    a.set_foreground(node)
    qa = a.problem(xa)
    assert list(np.flatnonzero(qa.tree.label == 1)) == [node]
    got, want = oracle.evaluate(qa)["lnL"], _mixture(pb.weights, f4, 0.48, 0.32)
    print("lnL at the point %.10f, the fixed-f mixture %.10f, difference %.3e" % (got, want, got - want))
    assert abs(got - want) <= 1e-9 * pb.weights.sum()
    assert abs(qa.freqK[0] - 0.48) < 1e-15 and abs(qa.freqK[1] - 0.32) < 1e-15


def test_set_foreground_and_newick_read_back_with_the_one_label():
    g, a, x = _lyso()
    a.set_x(x)
    for node in (3, 25):
        a.set_foreground(node)
        nw = a.newick()
        assert len(re.findall(r"#1", nw)) == 1 and "#" not in nw.replace("#1", "")
        assert list(np.flatnonzero(a.problem(x).tree.label == 1)) == [node]
    a.set_foreground(21)
    assert list(np.flatnonzero(a.problem(x).tree.label)) == [21]
    with pytest.raises(RuntimeError, match="root"):
        a.set_foreground(a.root)


@pytest.mark.parametrize("ctl,word", [("lyso_bsa_null.ctl", "fix_omega"), ("lysos_m0_clock.ctl", "clock"), ("hiv_ns0.ctl", "branch-site model A")])
def test_host_refuses_other_analyses_by_name(ctl, word):
    """Before anything reaches the engine: pamlh_foreground_scan, pamlh_foreground_point and pamlh_set_foreground alike."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), "codeml")
    x = np.array(a.default_x())
    for call in (lambda: a.foreground_scan(x), lambda: a.foreground_point(x, 1, 2.0, 0.5, 0.3), lambda: a.set_foreground(1)):
        with pytest.raises(RuntimeError, match=word):
            call()
