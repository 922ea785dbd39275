"""Maximum-likelihood placement in the C host (pamlh_attach_scores, pamlh_place_optimize, pamlh_place_ml, pamlh_placement_newick3) and
the driver (pamlh_lnl --place --place-ml), on the placement analysis of tests/test_placement_host_gpu.py: brown.nuc under K80 with kappa
fixed, Gorilla the query on the four-sequence tree.  The yardstick of the optimiser is a coordinate ascent on the CPU: Newton steps from
oracle.eval_branch on the enlarged problem (attach_ref.attached_problem; K80 is reversible, so the branch-local form is a reference), run
to 1e-9; the optimiser's lnL within 1e-4 of it (the bound tests/test_edge_host_gpu.py holds pamlh_edge_optimize to against
edge_ref.coordinate_ascent)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import attach_ref as at
import oracle
from paml_amd import hostlib
from test_nni_host_gpu import _bipartitions
from test_placement_cpu import TREE4, _analysis

pytestmark = pytest.mark.gpu
PENDANT, PHI = (0.05, 0.1, 0.2, 0.4), 0.5
NAMES = ["Human", "Chimpanzee", "Gorilla", "Orangutan", "Gibbon"]


def _cpu_ascent(pb, v, qrow, t3, tol=1e-9, lo=4e-6, hi=50.0, max_sweeps=500):
    """(t3, lnL): the three lengths at the new node maximised with everything else held, started at t3: the branches up, dn, pendant in
    turn, each by a safeguarded Newton iteration of its own on oracle.eval_branch (Newton's step where ddl < 0, otherwise the length
    doubled or halved along the gradient; clipped to [lo, hi]; halved until the lnL does not fall), until a sweep gains less than tol."""
    t = np.clip(np.array(t3, dtype=np.float64), lo, hi)
    big, nodes = at.attached_problem(pb, v, t, qrow)

    def val(j, tj):
        l, dl, ddl = oracle.eval_branch(big, nodes[j], np.array([tj]))
        return float(l[0]), float(dl[0]), float(ddl[0])
    l = val(0, t[0])[0]
    for _ in range(max_sweeps):
        l_sweep = l
        for j in range(3):
            for _ in range(60):
                l, d1, d2 = val(j, t[j])
                step = -d1 / d2 if d2 < 0 else (t[j] if d1 > 0 else -0.5 * t[j] if d1 < 0 else 0.0)
                tn = min(max(t[j] + step, lo), hi)
                gained = 0.0
                while abs(tn - t[j]) >= 1e-13:
                    l2 = val(j, tn)[0]
                    if l2 >= l:
                        gained, l = l2 - l, l2
                        t[j] = tn
                        break
                    tn = 0.5 * (tn + t[j])
                big.tree.branch[nodes[j]] = t[j]
                if gained <= 1e-13:
                    break
        if l - l_sweep < tol:
            break
    return t, l


def test_every_row_is_maximised_over_its_three_lengths(tmp_path):
    a = _analysis(tmp_path, "place", TREE4, placement=True)
    x = np.array(a.default_x())
    pb = a.problem(x)
    order = a.branch_order()
    nb = len(order)
    grid = a.placement_scores(x, PENDANT, PHI)
    base = a.eval_gpu(x, want_lnf=False)[0]
    ml = a.place_ml(x, 0, PENDANT, PHI)
    assert len(ml["q"]) == nb and not ml["q"].any() and sorted(ml["edge"]) == list(range(nb))
    le = grid["lnL"][0].max(axis=1)
    assert list(ml["edge"]) == sorted(range(nb), key=lambda e: (-le[e], e))      # (best of the grid first)
    start = np.array([[(1 - PHI) * pb.tree.branch[order[e]], PHI * pb.tree.branch[order[e]], PENDANT[int(np.argmax(grid["lnL"][0, e]))]] for e in ml["edge"]])
    s0 = a.attach_scores(x, ml["q"], ml["edge"], np.full(nb, -1), start)
    assert abs(s0["lnL0"] - base) <= 1e-10 * abs(base)
    assert np.all(np.abs(s0["lnL"] - le[ml["edge"]]) <= 1e-10 * np.abs(s0["lnL"]))      # (the start is the grid's best point)
    assert np.all(ml["lnL"] >= s0["lnL"]) and np.all(ml["lnL"] >= le[ml["edge"]])
    assert (ml["lnL"] > s0["lnL"] + 1e-3).any()
    again = a.attach_scores(x, ml["q"], ml["edge"], np.full(nb, 2), ml["t3"])
    assert np.all(np.abs(again["lnL"] - ml["lnL"]) <= 1e-8 * np.abs(ml["lnL"]))
    # likelihood weight ratios over the kept, maximised rows
    w = np.exp(ml["lnL"] - ml["lnL"].max())
    assert abs(ml["lwr"].sum() - 1) <= 1e-12 and np.allclose(ml["lwr"], w / w.sum(), rtol=1e-12, atol=0)
    # place_optimize by itself from the same starts: the same maxima, and its counts
    opt = a.place_optimize(x, ml["q"], ml["edge"], start)
    assert opt["lnL"].tobytes() == ml["lnL"].tobytes() and opt["t3"].tobytes() == ml["t3"].tobytes()
    assert 1 <= opt["sweeps"] <= 30 and opt["calls"] >= 1 + 3 * opt["sweeps"] and 0 <= opt["at_bound"] <= nb
    print("place_optimize: %d rows, %d sweeps, %d engine calls, %d rows at a bound" % (nb, opt["sweeps"], opt["calls"], opt["at_bound"]))
    # the best two branches against the coordinate ascent on the CPU
    for i in range(2):
        v = int(order[ml["edge"][i]])
        t_ref, l_ref = _cpu_ascent(pb, v, a.query_codes()[0], start[i])
        print("branch above node %d: host %.9f at %s; CPU ascent %.9f at %s" % (v, ml["lnL"][i], ml["t3"][i], l_ref, t_ref))
        assert abs(ml["lnL"][i] - l_ref) <= 1e-4
    # the analysis itself is as it was
    assert a.eval_gpu(x, want_lnf=False)[0] == base


def test_keep_and_the_tree_with_three_lengths(tmp_path):
    a = _analysis(tmp_path, "keep", TREE4, placement=True)
    x = np.array(a.default_x())
    order = a.branch_order()
    full, ml = a.place_ml(x, 0, PENDANT, PHI), a.place_ml(x, 2, PENDANT, PHI)
    assert len(ml["q"]) == 2 and list(ml["edge"]) == list(full["edge"][:2])
    assert ml["lnL"].tobytes() == full["lnL"][:2].tobytes() and ml["t3"].tobytes() == full["t3"][:2].tobytes()      # (a row is maximised by itself)
    assert abs(ml["lwr"].sum() - 1) <= 1e-12
    t_up, t_dn, t_pend = (float(t) for t in ml["t3"][0])
    nw = a.placement_newick3(0, int(ml["edge"][0]), t_up, t_dn, t_pend)
    want = a.placement_newick(0, int(ml["edge"][0]), PHI, 0.1)
    assert _bipartitions(nw, NAMES) == _bipartitions(want, NAMES) and len(_bipartitions(nw, NAMES)) == 2
    five = _analysis(tmp_path, "back", nw, n_tips=5)      # the host reads the tree back: the three lengths as they were written
    t5 = five.problem(np.array(five.default_x())).tree
    f = t5.father()
    g = NAMES.index("Gorilla")
    u = int(f[g])
    sib = [int(c) for c in t5.sons[u] if c != g]
    assert len(sib) == 1 and t5.branch[g] == t_pend and t5.branch[u] == t_up and t5.branch[sib[0]] == t_dn
    names4 = a.seq_names()
    v = int(order[ml["edge"][0]])
    assert v >= a.n_tips or NAMES[sib[0]] == names4[v]
    l5 = oracle.evaluate(five.problem(np.array(five.default_x())))["lnL"]
    assert abs(l5 - ml["lnL"][0]) <= 1e-8 * abs(l5)


def test_driver_prints_the_table_and_a_tree_that_reads_back(tmp_path):
    a = _analysis(tmp_path, "drv", TREE4, placement=True)
    x = np.array(a.default_x())
    ml = a.place_ml(x, 3, PENDANT, PHI)
    l0 = a.placement_scores(x, PENDANT, PHI)["lnL0"]
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--place", "--place-ml", "--keep", "3"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert any(ln.startswith("query 1 (Gorilla)") for ln in lines)
    rows = [ln.split() for ln in lines if re.fullmatch(r"\s*\d+\.\.\d+(\s+[0-9.]+){3}\s+-?[0-9.]+\s+-?[0-9.]+\s+[0-9.]+(\s+\*)?\s*", ln)]
    assert len(rows) == 3
    f = a.problem(x).tree.father()
    order = a.branch_order()
    for i, row in enumerate(rows):
        v = int(order[ml["edge"][i]])
        assert row[0] == "%d..%d" % (f[v] + 1, v + 1)
        assert np.allclose([float(c) for c in row[1:4]], ml["t3"][i], rtol=0, atol=6e-7)
        assert abs(float(row[4]) - ml["lnL"][i]) <= 6e-7 and abs(float(row[5]) - (ml["lnL"][i] - l0)) <= 1.2e-6 and abs(float(row[6]) - ml["lwr"][i]) <= 6e-7
        assert (row[-1] == "*") == (i == int(np.argmax(ml["lnL"])))
    nw = next(ln for ln in lines if ln.startswith("(") and ln.rstrip().endswith(";"))
    best = int(np.argmax(ml["lnL"]))
    assert nw == a.placement_newick3(0, int(ml["edge"][best]), *(float(t) for t in ml["t3"][best]))
    five = _analysis(tmp_path, "back", nw, n_tips=5)
    l5 = oracle.evaluate(five.problem(np.array(five.default_x())))["lnL"]
    assert abs(l5 - ml["lnL"][best]) <= 1e-8 * abs(l5)
    # --place alone: the grid's table as before, from pamlh_place's values
    ref, pl = a.placement_scores(x, PENDANT, PHI), a.place(x, PENDANT, PHI)
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--place"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "placement of 1 query on 5 branches (one engine call): lnL of the tree = %.6f, split %.4f" % (ref["lnL0"], PHI)
    assert lines[2:4] == ["query 1 (Gorilla)", "%10s %10s %16s %14s %9s" % ("branch", "pendant", "lnL", "difference", "LWR")]
    for b in range(5):
        v, lb = int(ref["edges"][b]), ref["lnL"][0, b]
        assert lines[4 + b] == "%10s %10.6f %16.6f %14.6f %9.6f%s" % ("%d..%d" % (f[v] + 1, v + 1), PENDANT[int(np.argmax(lb))], lb.max(), lb.max() - ref["lnL0"],
                                                                       pl["lwr"][0, b], " *" if b == pl["best_edge"][0] else "")
    assert lines[9] == a.placement_newick(0, int(pl["best_edge"][0]), PHI, float(pl["best_pendant"][0])) and len(lines) == 10
    assert subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--place-ml"], cwd=tmp_path, capture_output=True, text=True, timeout=300).returncode == 1


@pytest.mark.parametrize("ctl,word", [("brown_hky85_clock.ctl", "clock"), ("brown_hky85_adg.ctl", "rho")])
def test_host_refuses_clocks_and_rho_models_by_name(ctl, word):
    a = hostlib.Analysis(os.path.join(helpers.GOLDEN, "ctl", ctl), "baseml")
    x = np.array(a.default_x())
    for call in (lambda: a.attach_scores(x, [0], [0], [-1], np.full((1, 3), 0.1)), lambda: a.place_optimize(x, [0], [0], np.full((1, 3), 0.1)), lambda: a.place_ml(x)):
        with pytest.raises(RuntimeError, match=word):
            call()


def test_host_refuses_fixed_branch_lengths_and_bad_rows(tmp_path):
    from test_placement_cpu import BROWN, K80_TEXT
    tree = tmp_path / "fixed.trees"
    tree.write_text(TREE4 + "\n")
    ctl = tmp_path / "fixed.ctl"
    ctl.write_text(K80_TEXT % (BROWN, tree) + "fix_blength = 2\n")
    a = hostlib.Analysis(str(ctl), "baseml", placement=True)
    with pytest.raises(RuntimeError, match="fix_blength = 2"):
        a.place_ml(np.array(a.default_x()))
    b = _analysis(tmp_path, "rows", TREE4, placement=True)
    x = np.array(b.default_x())
    for q, e, t, word in [([1], [0], 0.1, "row 0: query 1 of 1"), ([0], [5], 0.1, "row 0: branch 5 of 5"), ([0], [0], -0.1, "row 0: length 0 is negative")]:
        with pytest.raises(RuntimeError, match=word):
            b.place_optimize(x, q, e, np.full((1, 3), t))
