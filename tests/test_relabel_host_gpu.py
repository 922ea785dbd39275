"""pamlh_foreground_scan on the lysozyme data of branch-site model A (lyso_bsa.ctl): every branch as the foreground in turn from one
engine call.  x_base is the golden's point with the foreground branch written at the background's time scale (t qfactor_fg /
qfactor_bg, both from a.problem(x).qfactor), so that the effective lengths of the scan, tau = t Qfactor_bg, are the golden's on every
branch; the grid holds the golden's w2.  Bounds: 1e-9 sum_h w_h, the family's bound for a sum of per-pattern logs."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from paml_amd import hostlib

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
GRID = (1, 1.5, 2, 3, 4.809805, 8, 20)
FG = 21      # the golden's foreground branch (0-based node)


def _start():
    g = helpers.load_golden("lyso_bsa")
    a = hostlib.Analysis(os.path.join(CTL, "lyso_bsa.ctl"), "codeml")
    x = np.array(g["x"])
    pb = a.problem(x)
    assert list(np.flatnonzero(pb.tree.label == 1)) == [FG]
    xb = x.copy()
    i = list(a.branch_order()).index(FG)
    xb[i] = x[i] * pb.qfactor[0][1] / pb.qfactor[0][0]
    return a, x, xb, float(pb.weights.sum())


@pytest.fixture(scope="module")
def scan():
    a, x, xb, wsum = _start()
    before = a.eval_gpu(x)
    labels = a.problem(x).tree.label.copy()
    sc = a.foreground_scan(xb, GRID)
    return dict(a=a, x=x, xb=xb, wsum=wsum, before=before, labels=labels, sc=sc)


def test_the_scan_finds_the_golden_point_and_ranks_its_branch_first(scan):
    sc, wsum = scan["sc"], scan["wsum"]
    assert len(sc["node"]) == 33 == scan["a"].n_nodes - 1 and sc["lnL"].shape == (33, len(GRID))      # (34 nodes: 33 branches)
    i = int(np.flatnonzero(sc["node"] == FG)[0])
    row = sc["lnL"][i][GRID.index(4.809805)]
    print("row (node %d, w2 4.809805): lnL %.8f; eval at the golden's x %.8f; delta of the branch %.4f, next %.4f"
          % (FG, row, scan["before"][0], sc["delta"][i], np.sort(sc["delta"])[-2]))
    assert row >= scan["before"][0] - 1e-9 * wsum
    assert int(np.argmax(sc["delta"])) == i and sc["delta"][i] > np.sort(sc["delta"])[-2]
    # s = 1 - 1e-6 and r = r_x lie in the box, and there the mixture is at least (1 - 1e-6) times the one without a foreground class
    assert (sc["lnL"] >= sc["lnL_base"] + wsum * np.log1p(-1e-6) - 1e-9 * wsum).all()
    assert (sc["best"] >= 1).all() and np.allclose(sc["delta"], 2 * (sc["lnL"][np.arange(33), sc["best"]] - sc["lnL"][:, 0]))


def test_the_scan_leaves_the_labels_and_the_evaluation_as_they_were(scan):
    a, x = scan["a"], scan["x"]
    assert np.array_equal(a.problem(x).tree.label, scan["labels"])
    after = a.eval_gpu(x)
    assert np.float64(after[0]).tobytes() == np.float64(scan["before"][0]).tobytes() and after[1].tobytes() == scan["before"][1].tobytes()


def test_rows_are_exact_points_of_the_model():
    """foreground_point, set_foreground, then the analysis's own evaluation: the row's lnL."""
    a, x, xb, wsum = _start()
    sc = a.foreground_scan(xb, GRID)
    i_fg = int(np.flatnonzero(sc["node"] == FG)[0])
    for i, g in ((i_fg, GRID.index(4.809805)), (2, 3), (i_fg - 1, 0)):      # the golden's row, a tip's row, a row at w2 = 1
        node = int(sc["node"][i])
        xa = a.foreground_point(xb, node, GRID[g], sc["p0"][i][g], sc["p1"][i][g])
        a.set_foreground(node)
        lnl = a.eval_gpu(xa, want_lnf=False)[0]
        print("node %d, w2 %g: the row %.9f, the model at its point %.9f, difference %.3e" % (node, GRID[g], sc["lnL"][i][g], lnl, lnl - sc["lnL"][i][g]))
        assert abs(lnl - sc["lnL"][i][g]) <= 1e-9 * wsum
    assert int(sc["node"][2]) < a.n_tips


def test_the_driver_prints_the_table_and_maximises_the_best_branch():
    a, x, xb, wsum = _start()
    args = [hostlib.DRIVER_PATH, "codeml", os.path.join(CTL, "lyso_bsa.ctl"), "--foreground-scan", "--omega-grid", ",".join("%r" % v for v in GRID), "--top", "1"]
    out = subprocess.run(args + ["%.17g" % v for v in xb], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    rows = [ln.split() for ln in lines if re.fullmatch(r"\s*\d+\.\.\d+\s+[0-9.]+\s+[0-9.]+\s+[0-9.]+\s+-?[0-9.]+\s+-?[0-9.]+\s*", ln)]
    assert len(rows) == 33 == a.n_nodes - 1
    top = max(rows, key=lambda r: float(r[5]))
    assert int(top[0].split("..")[1]) - 1 == FG
    head = next(ln for ln in lines if ln.startswith("foreground "))
    m = re.fullmatch(r"foreground (\d+)\.\.(\d+) maximised from the scan's point \(lnL (-?[0-9.]+)\): lnL = (-?[0-9.]+)", head)
    assert m and int(m.group(2)) - 1 == FG and float(m.group(4)) >= float(m.group(3)) - 1e-6
    nw = next(ln for ln in lines if ln.startswith("(") and ln.rstrip().endswith(";"))
    assert len(re.findall("#1", nw)) == 1
    # the labelled branch is the golden's: the same tip set below it as below node FG of the analysis's tree
    t = a.problem(x).tree
    below, stack = set(), [FG]
    while stack:
        u = stack.pop()
        if u < t.n_tips:
            below.add(a.seq_names()[u])
        stack += list(t.sons[u])
    end = nw.index(" #1")      # (the labelled node is internal: the text before the label ends with its closing bracket)
    assert nw[end - 1] == ")"
    depth, start = 0, end - 1
    while True:
        depth += (nw[start] == ")") - (nw[start] == "(")
        if depth == 0:
            break
        start -= 1
    assert set(n for n in a.seq_names() if re.search(r"[(,\s]%s[\s:#]" % re.escape(n), nw[start:end])) == below
