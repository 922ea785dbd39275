"""Pairwise ML dN / dS (codeml runmode = -2) without a GPU: the numpy restatement of lfun2dSdN against the reference's printed results,
and the host's logic — which control files the loader takes and refuses, complete deletion, the pairs' codon frequencies, the layout of
2ML.t / 2ML.dN / 2ML.dS."""
import os
import re

import numpy as np
import pytest

import pairwise_ref as ref
from paml_amd import hostlib

CTL = os.path.join(ref.GOLDEN, "ctl")
DATA = os.path.join(ref.GOLDEN, "data") + "/"


def _tips(name):
    a = hostlib.Analysis(os.path.join(CTL, name + ".ctl"), "codeml")
    L, h = a._L, a._h
    z = hostlib._arr(L.pamlh_tips(h), np.uint8, a.n_tips * a.n_patt).reshape(a.n_tips, a.n_patt).astype(np.int64)
    w = hostlib._arr(L.pamlh_weights(h), np.float64, a.n_patt)
    return a, z, w


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_reproduces_the_reference_lnl(name):
    """At the reference's printed x (5 decimals) the restated lnL equals its printed lnL (6 decimals) within 1e-6 for every pair: the
    print rounding of lnL (5e-7) doubled; x sits at a maximum, where its own rounding moves lnL by second order only."""
    g = ref.load(name)
    a, z, w = _tips(name)
    assert a.n_tips == g["n_seq"] and g["n_pairs"] == a.n_tips * (a.n_tips - 1) // 2
    worst = 0.0
    for p in g["pairs"]:
        fp, ls = ref.counts(z, w, p["i"] - 1, p["j"] - 1)
        pi = ref.codon_freqs(fp, ls, g["CodonFreq"])
        worst = max(worst, abs(ref.lnl(fp, pi, *ref.params(g, p)) - p["lnL"]))
    print("%s: max |lnL - printed| = %.2e over %d pairs" % (name, worst, g["n_pairs"]))
    assert worst <= 1e-6


def _load(tmp_path, base, prog="codeml", seq=None, **over):
    txt = open(os.path.join(CTL, base)).read().replace("../data/", DATA)
    if seq is not None:
        txt = re.sub(r"^\s*seqfile\s*=.*$", " seqfile = %s" % seq, txt, flags=re.M)
    for k, v in over.items():
        txt = re.sub(r"^\s*%s\s*=.*$" % k, "", txt, flags=re.M) + "\n %s = %s\n" % (k, v)
    f = tmp_path / "x.ctl"
    f.write_text(txt)
    return hostlib.Analysis(str(f), prog)


def test_loader_accepts_pairwise_control_files(tmp_path):
    """runmode = -2 for codeml with codon sequences loads without a tree file (the parent commit answers "runmode = -2 is not
    supported"); the free parameters are t and whichever of kappa, omega are not fixed."""
    a = _load(tmp_path, "pairwise_hiv_f3x4.ctl")
    assert a.is_pairwise() and a.n_pairs() == 78 and a.np == 3 and a.n == 61 and a.cleandata == 1
    assert a.seq_names()[0] == "U68496"
    assert _load(tmp_path, "pairwise_hiv_f61_fixk.ctl").np == 2
    assert _load(tmp_path, "pairwise_hiv_f3x4.ctl", fix_omega=1, omega=0.5).np == 2
    assert _load(tmp_path, "pairwise_hiv_f3x4.ctl", CodonFreq=0).is_pairwise()
    assert _load(tmp_path, "pairwise_hiv_f3x4.ctl", treefile=DATA + "HIVenvSweden.trees").is_pairwise()      # a tree file is allowed and ignored
    assert not hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml").is_pairwise()


@pytest.mark.parametrize("over, msg", [
    (dict(NSsites=2), "NSsites"), (dict(fix_alpha=0, alpha=0.5), "alpha"), (dict(fix_alpha=1, alpha=0.5), "alpha"), (dict(aaDist=1), "aaDist"),
    (dict(hkyREV=1), "hkyREV"), (dict(CodonFreq=4), "CodonFreq"), (dict(CodonFreq=5), "CodonFreq"), (dict(CodonFreq=6), "CodonFreq"),
    (dict(CodonFreq=7), "CodonFreq"), (dict(runmode=-3), "runmode"), (dict(seqtype=2), "seqtype"), (dict(seqtype=3), "seqtype"),
    (dict(model=2), "model")])
def test_loader_refuses_what_pairwise_does_not_cover(tmp_path, over, msg):
    with pytest.raises(RuntimeError, match=msg):
        _load(tmp_path, "pairwise_hiv_f3x4.ctl", **over)


def test_loader_refuses_several_genes_and_baseml(tmp_path):
    with pytest.raises(RuntimeError, match="Mgene|genes"):
        _load(tmp_path, "pairwise_hiv_f3x4.ctl", seq=DATA + "lysinYangSwanson2002.nuc", Mgene=0)      # option G: two partitions
    with pytest.raises(RuntimeError, match="runmode"):
        _load(tmp_path, "brown_hky85.ctl", prog="baseml", runmode=-2)


def test_complete_deletion_is_forced(tmp_path):
    """Like the reference (codeml.c:1849-1852) runmode = -2 drops every codon with a gap or an ambiguity in any sequence, whatever
    cleandata says."""
    src = open(DATA + "HIVenvSweden.txt").read().split("\n")
    k = next(i for i, ln in enumerate(src) if ln.startswith("U68497"))
    name, body = src[k].split(None, 1)
    body = body.replace(" ", "")
    src[k] = name + "   " + "---" + body[3:6] + "NNN" + body[9:]      # codons 1 and 3 of the second sequence
    f = tmp_path / "gaps.txt"
    f.write_text("\n".join(src))
    base = _load(tmp_path, "pairwise_hiv_f3x4.ctl")
    a = _load(tmp_path, "pairwise_hiv_f3x4.ctl", seq=str(f), cleandata=0)
    assert base.ls == 91 and a.ls == 89 and a.cleandata == 1 and a.n_codes == 61


@pytest.mark.parametrize("codonfreq", [0, 1, 2, 3])
def test_pair_frequencies_follow_getcodonfreqs2(tmp_path, codonfreq):
    a, z, w = _tips("pairwise_hiv_f3x4")
    b = _load(tmp_path, "pairwise_hiv_f3x4.ctl", CodonFreq=codonfreq)
    for i, j in ((1, 0), (7, 3), (12, 11)):
        fp, ls = ref.counts(z, w, i, j)
        np.testing.assert_allclose(b.pairwise_freqs(fp, ls), ref.codon_freqs(fp, ls, codonfreq), rtol=1e-13, atol=1e-300)


def test_codon_pattern_has_the_universal_code_counts():
    row, col, fl = ref.pattern()
    assert len(row) == 263 + 61 and int((row != col).sum()) == 263 and not fl[row == col].any()
    assert int(((fl & 2) != 0).sum()) == 196 and int(((fl & 2) == 0)[row != col].sum()) == 67      # nonsynonymous / synonymous one-step pairs


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_2ml_files_have_the_reference_layout(tmp_path, name):
    """Given the recorded numbers the writer reproduces the reference's 2ML.t, 2ML.dN and 2ML.dS byte for byte."""
    g = ref.load(name)
    a = hostlib.Analysis(os.path.join(CTL, name + ".ctl"), "codeml")
    rec = {k: ref.parse_2ml(g["files"][k])[0] for k in ("2ML.t", "2ML.dN", "2ML.dS")}
    tab = np.zeros((g["n_pairs"], 9))
    for q, p in enumerate(g["pairs"]):
        key = (p["i"], p["j"])
        assert q == (p["i"] - 1) * (p["i"] - 2) // 2 + p["j"] - 1
        t, k, w = ref.params(g, p)
        tab[q] = [rec["2ML.t"][key], k, w, p["lnL"], p["S"], p["N"], rec["2ML.dN"][key], rec["2ML.dS"][key], 0]
    a.pairwise_write(tab, str(tmp_path))
    for k in ("2ML.t", "2ML.dN", "2ML.dS"):
        assert (tmp_path / k).read_text() == g["files"][k], k
    rst = (tmp_path / "rst").read_text().split("Paras.\n")[1].split("\n")
    p = g["pairs"][5]
    assert rst[5].split()[:7] == ["%d" % p["i"], "%d" % p["j"], "%.1f" % p["N"], "%.1f" % p["S"], "%.4f" % p["dN"], "%.4f" % p["dS"], "%.4f" % p["omega"]]
