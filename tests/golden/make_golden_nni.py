#!/usr/bin/env python3
"""Generate the NNI tree-search golden vector: runs the UNMODIFIED reference baseml (oracle/_ref/baseml, built by oracle/Makefile) with
runmode = 5 (Perturbation treesub.c:4642: the NNI search from the tree of the tree file), model = 4 (HKY85), cleandata = 1 on
data/brown.nuc from each starting tree below, and records what it printed: the lnL of the starting tree, of every better tree and of the
best tree (four decimals), and the best tree as the set of its tip bipartitions.

What is committed is data: the starting trees, the bipartitions, the printed numbers.

usage: python tests/golden/make_golden_nni.py
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
STARTS = ("((Human,Gorilla),Chimpanzee,(Orangutan,Gibbon));", "((Human,Orangutan),Gorilla,(Chimpanzee,Gibbon));")


def bipartitions(newick, names):
    """The non-trivial splits of the unrooted tree, each as the sorted names of the side without names[0]."""
    s = re.sub(r":\s*[0-9.eE+-]+", "", newick).replace(" ", "").rstrip(";")
    stack, splits = [], set()
    for tok in re.findall(r"[(),]|[^(),]+", s):
        if tok == "(":
            stack.append(set())
        elif tok == ")":
            clade = stack.pop()
            if stack:
                stack[-1] |= clade
                side = clade if names[0] not in clade else set(names) - clade
                if 1 < len(side) < len(names) - 1:
                    splits.add(tuple(sorted(side)))
        elif tok != ",":
            stack[-1].add(tok)
    return sorted(splits)


def run(start):
    d = tempfile.mkdtemp(prefix="golden_nni_")
    try:
        shutil.copy(os.path.join(HERE, "data", "brown.nuc"), os.path.join(d, "seq.txt"))
        names = [ln.strip() for ln in open(os.path.join(d, "seq.txt")) if re.fullmatch(r"[A-Za-z]+", ln.strip()) and not re.fullmatch(r"[ACGTacgt]+", ln.strip())]
        with open(os.path.join(d, "tree.txt"), "w") as f:
            f.write("%d 1\n%s\n" % (len(names), start))
        with open(os.path.join(d, "baseml.ctl"), "w") as f:
            f.write("seqfile = seq.txt\ntreefile = tree.txt\noutfile = mlb\nnoisy = 0\nverbose = 0\nrunmode = 5\nmodel = 4\nfix_kappa = 0\nkappa = 5\n"
                    "fix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\ngetSE = 0\nclock = 0\nMgene = 0\nnhomo = 0\nfix_rho = 1\nrho = 0\nRateAncestor = 0\n"
                    "Small_Diff = 1e-6\nmethod = 0\n")
        subprocess.run([REF, "baseml.ctl"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT, timeout=3600, input=b"\n" * 50, check=True)
        out = open(os.path.join(d, "mlb")).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    body = out.split("Heuristic tree search by NNI perturbation")[1]
    head, best = body.split("Best tree found:")
    trace = [-abs(float(v)) for v in re.findall(r"lnL =\s*(-?[0-9.]+)", head)]      # (the start's is printed negated, the better trees' are not)
    best_lnl = -abs(float(re.search(r"lnL =\s*(-?[0-9.]+)", best).group(1)))
    best_tree = [ln.strip() for ln in best.split("\n") if ln.strip().startswith("(") and re.search(r"[A-Za-z]", ln)][0]
    return names, dict(start=start, lnL_trace=trace, best_lnL=best_lnl, best_tree=best_tree, best_bipartitions=bipartitions(best_tree, names))


if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/baseml is not built (make -C oracle)")
    runs = []
    for s in STARTS:
        names, r = run(s)
        runs.append(r)
        print("%s: %s -> %s" % (s, " -> ".join("%.4f" % v for v in r["lnL_trace"]), r["best_tree"]))
    doc = dict(case="brown_nni_search", program="baseml", seqfile="data/brown.nuc", runmode=5, model=4, cleandata=1, names=names, runs=runs)
    with open(os.path.join(HERE, "brown_nni_search.json"), "w") as f:
        json.dump(doc, f, indent=1)
