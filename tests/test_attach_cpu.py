"""The yardstick of the attachment tests (tests/attach_ref.py) pinned on the CPU, before any GPU run.  The restatement's lnf of every
non-root branch with every query role at random lengths against oracle.evaluate of the enlarged problem with the three lengths written
into its tree, at 1e-9 (the edge tests' bound for lnf); on the exactly reversible shapes its d1 and d2 against oracle.eval_branch of the
enlarged problem at the role's node (rtol 1e-9, atol 1e-9: the edge tests' TOL); on the irreversible shapes, where the oracle's
branch-local form re-roots the tree and is no reference, against central differences of the restatement's own lnL and d1."""
import numpy as np
import pytest

import ancestral_ref as ar
import attach_ref as at
import edge_ref as er
import gradient_ref as gr
import nni_ref as nr
import oracle
import placement_ref as pr
from test_gradient_cpu import _irreversible_cases

TOL = dict(rtol=1e-9, atol=1e-9)


def _restatement_against_the_oracle(pb, scale_every=None, derivatives=True):
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=12)
    assert len(rows) == 4 * (pb.tree.n_nodes - 1)
    got = at.attach_scores(pb, queries, rows, t3)
    assert np.max(np.abs(got["lnf0"] - oracle.evaluate(pb)["lnf"])) <= 1e-9
    worst, worst_d = 0.0, 0.0
    for i in range(len(rows)):
        q, v, role = (int(c) for c in rows[i])
        big, nodes = at.attached_problem(pb, v, t3[i], queries[q], 0, scale_every)
        worst = max(worst, float(np.max(np.abs(got["lnf"][i] - oracle.evaluate(big)["lnf"]))))
        if role < 0:
            assert got["d1"][i] == 0 and got["d2"][i] == 0
        elif derivatives:
            _, dl, ddl = oracle.eval_branch(big, nodes[role], np.array([t3[i][role]]))
            worst_d = max(worst_d, abs(got["d1"][i] - dl[0]), abs(got["d2"][i] - ddl[0]))
            assert np.allclose(got["d1"][i], dl[0], **TOL), (i, rows[i], got["d1"][i], dl[0])
            assert np.allclose(got["d2"][i], ddl[0], **TOL), (i, rows[i], got["d2"][i], ddl[0])
    print("%d rows: largest |lnf - oracle| %.3e; largest |d - oracle| %.3e" % (len(rows), worst, worst_d))
    assert worst <= 1e-9
    return queries, rows, t3, got


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracle_on_the_enlarged_tree(name):
    _restatement_against_the_oracle(gr.reversible_problem(name), nr.scale_every_of(name))


@pytest.mark.parametrize("name", [c[0] for c in _irreversible_cases()])
def test_restatement_on_irreversible_models(name):
    """lnf against the oracle on the enlarged tree; d1 against the central difference of the restatement's own lnL and d2 against that
    of its own d1, both along the role's length with step h = 1e-6, relative to max(1, |d|).  Every length differenced is >= 1e-3 (a
    thousand steps).  What the difference itself is off by: truncation h^2 / 6 x the third derivative above the one differenced, which
    for lengths t >= 1e-3 is at most ~ |d| / t^2 <= 1e6 |d|, so <= 2e-7 |d|; rounding 1e-16 x |lnL| (<= 1e5) / h = 1e-5 absolute at the
    very worst for d1 and 1e-16 x |d1| (<= 1e5) / h for d2.  Allowance 1e-4; a formula that took the wrong factor for a role is off by
    the order of d itself."""
    pb = dict(_irreversible_cases())[name]()
    queries, rows, t3, got = _restatement_against_the_oracle(pb, derivatives=False)
    keep = rows[:, 2] >= 0
    rows, t3 = rows[keep], t3[keep]
    d1, d2 = got["d1"][keep], got["d2"][keep]
    h = 1e-6
    P = ar.matrices_from_oracle(pb)
    passes = er.tree_passes(pb, P)
    side = []
    for sgn in (1, -1):
        tt = t3.copy()
        tt[np.arange(len(rows)), rows[:, 2]] += sgn * h
        assert tt[np.arange(len(rows)), rows[:, 2]].min() >= 1e-3 - h
        side.append(at.attach_scores(pb, queries, rows, tt, P=P, passes=passes))
    fd1 = (side[0]["lnL"] - side[1]["lnL"]) / (2 * h)
    fd2 = (side[0]["d1"] - side[1]["d1"]) / (2 * h)
    dev1 = float(np.max(np.abs(d1 - fd1) / np.maximum(1.0, np.abs(d1))))
    dev2 = float(np.max(np.abs(d2 - fd2) / np.maximum(1.0, np.abs(d2))))
    print("%s: %d rows: largest deviation from central differences: d1 %.3e, d2 %.3e" % (name, len(rows), dev1, dev2))
    assert d1.any() and d2.any() and dev1 <= 1e-4 and dev2 <= 1e-4


def test_role_minus_one_gives_zero_derivatives_and_the_same_lnf():
    pb = gr.reversible_problem("5-K1")
    queries = pr.queries_of(pb)
    rows, t3 = at.all_rows(pb, len(queries), seed=3)
    rows[:4, 0] = 1      # (the four roles of the first branch, one query)
    a = at.attach_scores(pb, queries, rows[:4], t3[:4])
    assert np.array_equal(a["lnf"][0], a["lnf"][1]) and np.array_equal(a["lnf"][0], a["lnf"][3])
    assert a["d1"][0] == 0 and a["d2"][0] == 0 and a["d1"][1:].all()


def test_split_lengths_give_the_placement_restatement():
    """t3 = ((1 - phi) t_v, phi t_v, tau) is the grid call's tree: the two restatements agree to rounding."""
    pb = gr.reversible_problem("5-K1")
    queries = pr.queries_of(pb)
    phi, tau = 0.3, 0.07
    ref = pr.placement_scores_of(pb, queries, phi, [tau])
    rows = [[q, int(v), -1] for q in range(len(queries)) for v in ref["edges"]]
    t3 = [[(1 - phi) * pb.tree.branch[v], phi * pb.tree.branch[v], tau] for _, v, _ in rows]
    got = at.attach_scores(pb, queries, rows, t3)
    assert np.max(np.abs(got["lnf"].reshape(len(queries), len(ref["edges"]), -1) - ref["lnf"][:, :, 0])) <= 1e-12


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, one class, all 60 rows.  The bytes a pattern takes in the
    workspace: 2 K n_int (n_s + 1) doubles for the down partials and the outer messages (n_s = 64 on the matrix cores), then 4 K + 3
    doubles (f, f', f'' and their log factor per class; lnf, g1, g2) per row and for the present tree."""
    K, n_int, n_rows, n_patt = 1, 9 - 2, 4 * (2 * 9 - 3), 3000
    per_patt = 2 * K * n_int * (64 + 1) * 8 + (n_rows + 1) * (4 * K + 3) * 8
    assert n_patt * per_patt > 1 << 20
    assert 64 * per_patt <= 1 << 20      # (and one tile with all rows fits: the patterns are walked in batches, not the rows in groups)
