"""A numpy restatement of the reference's pairwise likelihood (lfun2dSdN codeml.c:4219-4264 with the set-up of PairwiseCodon
codeml.c:4407-4453, GetCodonFreqs2 4169-4216 and the GY94 rate matrix of eigenQcodon 3229-3316), shared by the pairwise tests.
Universal genetic code."""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("pairwise_hiv_f3x4", "pairwise_hiv_f61_fixk", "pairwise_mhc40_f1x4")
AA = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"      # codons in T C A G order
SENSE = [c for c in range(64) if AA[c] != "*"]
N = len(SENSE)


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def counts(z, w, a, b):
    """fp[max][min] += w (codeml.c:4407-4413) and the number of sites."""
    fp = np.zeros((N, N))
    np.add.at(fp, (np.maximum(z[a], z[b]), np.minimum(z[a], z[b])), w)
    return fp, float(w.sum())


def codon_freqs(fp, ls, codonfreq):
    pi = (fp.sum(axis=1) + fp.sum(axis=0)) / (2.0 * ls)
    if codonfreq == 0:
        return np.full(N, 1.0 / N)
    if codonfreq == 3:
        return pi
    b = np.array([[c // 16, (c // 4) % 4, c % 4] for c in SENSE])
    f3 = np.zeros((3, 4))
    for j in range(3):
        np.add.at(f3[j], b[:, j], pi)
    f4 = f3.sum(axis=0) / 3.0
    out = f3[0][b[:, 0]] * f3[1][b[:, 1]] * f3[2][b[:, 2]] if codonfreq == 2 else f4[b[:, 0]] * f4[b[:, 1]] * f4[b[:, 2]]
    return out / out.sum()


def pattern():
    """(row, col, flags) of the elements a codon matrix can have at and below its diagonal, row-major; flags bit 0 = transition,
    bit 1 = nonsynonymous."""
    row, col, fl = [], [], []
    for i in range(N):
        for j in range(i + 1):
            c1, c2 = SENSE[i], SENSE[j]
            d = [(c1 // 16, c2 // 16), ((c1 // 4) % 4, (c2 // 4) % 4), (c1 % 4, c2 % 4)]
            diff = [x for x in d if x[0] != x[1]]
            if len(diff) > 1:
                continue
            f = 0
            if diff:
                f |= 1 if sum(diff[0]) in (1, 5) else 0      # T<->C (0 + 1), A<->G (2 + 3)
                f |= 2 if AA[c1] != AA[c2] else 0
            row.append(i); col.append(j); fl.append(f)
    return np.array(row, dtype=np.int32), np.array(col, dtype=np.int32), np.array(fl, dtype=np.uint8)


_PAT = pattern()


def lnl(fp, pi, t, kappa, omega):
    row, col, fl = _PAT
    off = row != col
    s = np.where(fl[off] & 1, kappa, 1.0) * np.where(fl[off] & 2, omega, 1.0)
    S = np.zeros((N, N))
    S[row[off], col[off]] = s
    S = S + S.T
    Q = S * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(axis=1))
    mr = -(pi * np.diag(Q)).sum()
    live = pi > 1e-100
    sp = np.sqrt(pi[live])
    A = (sp[:, None] * Q[np.ix_(live, live)]) / sp[None, :]
    w, R = np.linalg.eigh((A + A.T) / 2)
    P = np.zeros((N, N))
    P[np.ix_(live, live)] = ((R * np.exp(w * t / mr)[None, :]) @ R.T) * sp[None, :] / sp[:, None]
    j, k = np.nonzero(np.tril(fp) > 0)
    f = pi[j] * P[j, k]
    f = np.where(f <= 0, 1e-70, f)
    return float((fp[j, k] * np.log(f)).sum())


def params(g, p):
    """(t, kappa, omega) of a golden pair from its printed x."""
    x = p["x"]
    if g["fix_kappa"]:
        return x[0], g["kappa"], x[1]
    return x[0], x[1], x[2]


def parse_2ml(text):
    """{(i, j): value} (1-based, j < i) and the names of a 2ML.* file."""
    lines = [ln for ln in text.split("\n") if ln.strip()]
    ns, vals, names = int(lines[0]), {}, []
    for i, ln in enumerate(lines[1:1 + ns]):
        tok = ln.split()
        names.append(tok[0])
        assert len(tok) == 1 + i
        for j, v in enumerate(tok[1:]):
            vals[(i + 1, j + 1)] = float(v)
    return vals, names
