#!/usr/bin/env python3
"""Generate the pairwise (runmode = -2) golden vectors: runs the UNMODIFIED reference codeml (oracle/_ref/codeml, built by
oracle/Makefile) on the committed control files tests/golden/ctl/pairwise_*.ctl with getSE = 0, noisy = 0 and records, per pair, what it
printed: from the main result file lnL (6 decimals) and x (5 decimals), from `rst` N, S, dN, dS, omega, and the three 2ML.* files verbatim.

What is committed is data.  `data/bigmhc40.phy` (the first 40 sequences of data/bigmhc.phy as a plain sequential PHYLIP file) is written
here as well.

usage: python tests/golden/make_golden_pairwise.py [case ...]
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(REPO, "oracle", "_ref", "codeml")
CASES = ("pairwise_hiv_f3x4", "pairwise_hiv_f61_fixk", "pairwise_mhc40_f1x4")


def write_mhc40():
    """The first 40 sequences of bigmhc.phy (192 x 810, options GC, sequential): header, then name line + sequence lines."""
    src = open(os.path.join(HERE, "data", "bigmhc.phy")).read().split("\n")
    ns, ls = int(src[0].split()[0]), int(src[0].split()[1])
    seqs, i = [], 1
    while len(seqs) < 40:
        while not src[i].strip():
            i += 1
        tok = src[i].split()      # (a few sequences start on the line of their name)
        name, i, s = tok[0], i + 1, "".join(tok[1:])
        while len(s) < ls:
            s += "".join(src[i].split())
            i += 1
        assert len(s) == ls, (name, len(s))
        seqs.append((name, s))
    assert ns == 192
    with open(os.path.join(HERE, "data", "bigmhc40.phy"), "w") as f:
        f.write("%6d %6d\n" % (len(seqs), ls))
        for name, s in seqs:
            f.write("%s\n" % name)
            for k in range(0, ls, 60):
                f.write(s[k:k + 60] + "\n")


def read_ctl(path):
    opts = {}
    for line in open(path):
        line = line.split("*")[0]
        if "=" in line:
            k, v = line.split("=", 1)
            opts[k.strip()] = v.strip()
    return opts


def run_case(name):
    ctl = read_ctl(os.path.join(HERE, "ctl", name + ".ctl"))
    d = tempfile.mkdtemp(prefix="golden_pw_")
    try:
        seq = os.path.normpath(os.path.join(HERE, "ctl", ctl["seqfile"]))
        shutil.copy(seq, os.path.join(d, "seq.txt"))
        ctl.update(seqfile="seq.txt", outfile="mlc", noisy="0", verbose="0", getSE="0")
        ctl.pop("treefile", None)
        with open(os.path.join(d, "codeml.ctl"), "w") as f:
            for k, v in ctl.items():
                f.write("%s = %s\n" % (k, v))
        t0 = time.time()
        subprocess.run([REF, "codeml.ctl"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT, timeout=7200, input=b"\n" * 50, check=True)
        secs = time.time() - t0
        mlc = open(os.path.join(d, "mlc")).read()
        rst = open(os.path.join(d, "rst")).read()
        files = {k: open(os.path.join(d, k)).read() for k in ("2ML.t", "2ML.dN", "2ML.dS")}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    pairs = []
    # main result file: "\n\n2 (name) ... 1 (name)\nlnL = -123.456789\n  x0 x1 x2\n"
    for m in re.finditer(r"\n(\d+) \((\S+)\) \.\.\. (\d+) \((\S+)\)\nlnL =\s*(-?[0-9.]+)\n([^\n]*)\n", mlc):
        pairs.append(dict(i=int(m.group(1)), j=int(m.group(3)), lnL=float(m.group(5)), x=[float(v) for v in m.group(6).split()]))
    # rst: "seq seq N S dN dS dN/dS Paras." then "%3d %3d %8.1f %8.1f %8.4f %8.4f %8.4f x... lnL"
    tab = rst.split("Paras.")[1]
    rows = [ln.split() for ln in tab.strip().split("\n") if len(ln.split()) >= 8]
    assert len(rows) == len(pairs), (len(rows), len(pairs))
    for p, r in zip(pairs, rows):
        assert (int(r[0]), int(r[1])) == (p["i"], p["j"])
        p.update(N=float(r[2]), S=float(r[3]), dN=float(r[4]), dS=float(r[5]), omega=float(r[6]))
    names = [ln.split()[0] for ln in files["2ML.t"].split("\n")[1:] if ln.strip()]
    out = dict(case=name, program="codeml", ctl="ctl/%s.ctl" % name, n_seq=len(names), names=names, n_pairs=len(pairs),
               CodonFreq=int(ctl["CodonFreq"]), fix_kappa=int(ctl.get("fix_kappa", 0)), kappa=float(ctl.get("kappa", 2)),
               fix_omega=int(ctl.get("fix_omega", 0)), reference_seconds=round(secs, 1), pairs=pairs, files=files)
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    n_bound = sum(1 for p in pairs if p["omega"] >= 98.99 or p["omega"] <= 0.00101 or p["x"][0] >= 49.99)
    print("%s: %d sequences, %d pairs, %d on a bound (%.1f %%), reference %.1f s" % (name, len(names), len(pairs), n_bound, 100.0 * n_bound / len(pairs), secs))


if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/codeml is not built (make -C oracle)")
    write_mhc40()
    for c in (sys.argv[1:] or CASES):
        run_case(c)
