#!/usr/bin/env python3
"""Generate the golden vector of the SPR search's tests: runs the UNMODIFIED reference baseml (oracle/_ref/baseml, built by
oracle/Makefile) with runmode = 0 (the tree of the tree file, branch lengths and kappa estimated), model = 4 (HKY85), cleandata = 1 on
data/brown.nuc, once for each of the 15 unrooted topologies of its five sequences, and records the lnL it printed for each.

What is committed is data: the trees as Newick strings, their tip bipartitions, the printed numbers.

usage: python tests/golden/make_golden_spr.py
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(REPO, "oracle", "_ref", "baseml")
sys.path.insert(0, HERE)
from make_golden_nni import bipartitions  # noqa: E402


def topologies(names):
    """The 15 unrooted binary trees of five tips: a middle tip and the other four in two pairs."""
    out = []
    for m in names:
        a, b, c, d = [n for n in names if n != m]
        for (p, q), (r, s) in (((a, b), (c, d)), ((a, c), (b, d)), ((a, d), (b, c))):
            out.append("((%s,%s),%s,(%s,%s));" % (p, q, m, r, s))
    return out


def run(newick):
    d = tempfile.mkdtemp(prefix="golden_spr_")
    try:
        shutil.copy(os.path.join(HERE, "data", "brown.nuc"), os.path.join(d, "seq.txt"))
        with open(os.path.join(d, "tree.txt"), "w") as f:
            f.write("5 1\n%s\n" % newick)
        with open(os.path.join(d, "baseml.ctl"), "w") as f:
            f.write("seqfile = seq.txt\ntreefile = tree.txt\noutfile = mlb\nnoisy = 0\nverbose = 0\nrunmode = 0\nmodel = 4\nfix_kappa = 0\nkappa = 5\n"
                    "fix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\ngetSE = 0\nclock = 0\nMgene = 0\nnhomo = 0\nfix_rho = 1\nrho = 0\nRateAncestor = 0\n"
                    "Small_Diff = 1e-6\nmethod = 0\n")
        subprocess.run([REF, "baseml.ctl"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT, timeout=3600, input=b"\n" * 50, check=True)
        out = open(os.path.join(d, "mlb")).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return float(re.search(r"lnL\(ntime:\s*\d+\s+np:\s*\d+\):\s*(-?[0-9.]+)", out).group(1))


if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/baseml is not built (make -C oracle)")
    names = json.load(open(os.path.join(HERE, "brown_nni_search.json")))["names"]
    trees = []
    for nw in topologies(names):
        lnl = run(nw)
        trees.append(dict(newick=nw, bipartitions=bipartitions(nw, names), lnL=lnl))
        print("%s %.6f" % (nw, lnl))
    assert len(set(json.dumps(t["bipartitions"]) for t in trees)) == 15
    doc = dict(case="brown_spr_all15", program="baseml", seqfile="data/brown.nuc", runmode=0, model=4, cleandata=1, names=names, trees=trees)
    with open(os.path.join(HERE, "brown_spr_all15.json"), "w") as f:
        json.dump(doc, f, indent=1)
