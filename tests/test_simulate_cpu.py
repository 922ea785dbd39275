"""Simulation under the loaded model, the parts that need no GPU: the numpy restatement of the draw (tests/simulate_ref.py) against
exact pattern probabilities, the counter layout, and pamlh_write_alignment's round trip through the sequence reader."""
import os

import numpy as np
import pytest

import helpers
import oracle
import simulate_ref as ref
from paml_amd import hostlib

CTL = os.path.join(helpers.GOLDEN, "ctl")


def test_restatement_against_exact_probabilities():
    """10^6 sites of the star case: Pearson's X^2 over the 64 patterns against the oracle's probabilities stays below the
    Wilson-Hilferty value of chi-square(63) at z = 6 (about 156); a wrong orientation of P, class rate or root table gives thousands."""
    pb, P = ref.star_case()
    prob = np.exp(oracle.evaluate(pb)["lnf"])
    assert abs(prob.sum() - 1) < 1e-12
    n_sites = 10 ** 6
    expected = prob * n_sites
    assert expected.min() > 20, expected.min()
    sim = ref.simulate(pb.pi[0], pb.freqK, P, pb.tree.sons, pb.tree.root, 3, n_sites, seed=1)
    counts = ref.pattern_counts(sim["z"])
    x2 = float(((counts - expected) ** 2 / expected).sum())
    bound = ref.chi2_bound(63, 6.0)
    print("X2 = %.2f, bound = %.2f, smallest expected count = %.1f" % (x2, bound, expected.min()))
    assert 155 < bound < 157
    assert x2 < bound
    # the classes are drawn from freqK: a binomial count within six standard deviations
    n1 = int(sim["cls"].sum())
    assert abs(n1 - 0.7 * n_sites) < 6 * np.sqrt(n_sites * 0.3 * 0.7), n1


def test_counter_layout():
    """Site j of a 5-site request with first_site = 7 is site j + 7 of a 12-site request."""
    pb, P = ref.star_case()
    args = (pb.pi[0], pb.freqK, P, pb.tree.sons, pb.tree.root, 3)
    whole = ref.simulate(*args, 12, seed=3, replicate=2)
    part = ref.simulate(*args, 5, seed=3, replicate=2, first_site=7)
    for key in ("z", "cls", "anc"):
        assert np.array_equal(part[key], whole[key][..., 7:12]), key
    assert not np.array_equal(ref.simulate(*args, 12, seed=3, replicate=3)["z"], whole["z"])


@pytest.mark.parametrize("ctl,program", [("brown_hky85.ctl", "baseml"), ("stewart_lg_g4.ctl", "codeml"), ("hiv_ns0_icode4.ctl", "codeml")])
def test_write_alignment_round_trip(ctl, program, tmp_path):
    """Random states written by pamlh_write_alignment and read back by the sequence reader: the encoded tips, expanded by pose, are z."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), program)
    rng = np.random.default_rng(257)
    z = rng.integers(0, a.n, size=(a.n_tips, 257)).astype(np.uint8)
    path = str(tmp_path / "sim.phy")
    a.write_alignment(z, path)
    b = hostlib.Analysis(os.path.join(CTL, ctl), program, overrides="seqfile = " + path)
    assert (b.n, b.n_tips) == (a.n, a.n_tips) and b.seq_names() == a.seq_names()
    pose = b.pose()
    assert len(pose) == 257
    tips = hostlib._arr(b._L.pamlh_tips(b._h), np.uint8, b.n_tips * b.n_patt).reshape(b.n_tips, b.n_patt)
    assert np.array_equal(tips[:, pose], z)
