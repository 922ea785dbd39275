"""Tree comparison without a GPU: the table arithmetic from a given replicate matrix (pamlh_tree_comparison_from_replicates) against
a numpy restatement of the formulas, the restated generator's own indices, and the host path's results unchanged."""
import numpy as np

import helpers
import rell_ref as ref
from paml_amd import hostlib


def _check(lnf, w, rep):
    got = hostlib.tree_comparison_from_replicates(lnf, w, rep)
    want = ref.table_from_replicates(lnf, w, rep)
    assert got["best"] == want["best"]
    # li, Dli, SE: sums of n_patt <= 100 products, the two sides in different orders: n * eps * sum |terms| <= 1e-14 * 3000 here
    for k in ("li", "dli", "se"):
        assert np.all(np.abs(got[k] - want[k]) <= 1e-10), (k, got[k], want[k])
    # pKH: the host's normal distribution function is the reference's series (Hill 1973), good to about 1e-9; math.erfc is exact to eps
    assert np.all(np.abs(got["pKH"] - want["pKH"]) <= 1e-8), (got["pKH"], want["pKH"])
    # pSH, pRELL: counts over n_rep, accumulated as k additions of 1 / n_rep (or a half, a third of it): k * eps
    for k in ("pSH", "pRELL"):
        assert np.all(np.abs(got[k] - want[k]) <= 1e-12), (k, got[k], want[k])
    assert abs(got["pRELL"].sum() - 1) < 1e-9
    return got


def test_table_from_replicates_matches_the_formulas():
    rng = np.random.default_rng(1)
    n_patt = 60
    w = rng.integers(0, 9, n_patt).astype(float)
    for n_trees, n_rep in ((2, 200), (3, 1000), (7, 333)):
        lnf = rng.uniform(-8, -1, (n_trees, n_patt))
        lnf[1:] -= rng.uniform(0, 0.05, (n_trees - 1, 1))      # tree 0 a little better: P values away from 0 and 1
        rep, _ = ref.replicates(lnf, w, [0, 20, n_patt], n_rep, seed=3)
        got = _check(lnf, w, rep)
        assert 0 < got["pRELL"].max() < 1 or n_trees == 2


def test_ties_share_a_replicate_and_a_tree_without_variance_has_no_p_value():
    """Tree 1 = tree 0 exactly (SE = 0 < 1e-6: pKH = pSH = -1; equal in every replicate: each gets half of what the pair wins), tree 2 =
    tree 0 + 2e-9 at one pattern (best by a hair, within 1e-5 of trees 0 and 1 in every replicate: a three-way tie), tree 3 about one SE behind."""
    rng = np.random.default_rng(2)
    n_patt = 50
    w = rng.integers(1, 6, n_patt).astype(float)
    a = rng.uniform(-8, -1, n_patt)
    d = rng.uniform(-0.3, 0.3, n_patt)
    worse = a + d - (w @ d / w.sum() + 0.01)      # 0.01 a site behind: Dli = -0.01 ls = -1.5 against an SE of about 0.17 sqrt(ls) = 2
    lnf = np.stack([a, a, a, worse])
    lnf[2, 7] += 2e-9
    rep, _ = ref.replicates(lnf, w, None, 500, seed=8)
    got = _check(lnf, w, rep)
    assert got["best"] == 2 and got["se"][0] < 1e-6 and got["se"][1] < 1e-6
    assert got["pKH"][0] == -1 and got["pSH"][0] == -1 and got["pKH"][1] == -1 and got["pKH"][2] == -1
    assert got["pRELL"][0] == got["pRELL"][1] and abs(got["pRELL"][:3].sum() + got["pRELL"][3] - 1) < 1e-9
    assert 0 < got["pKH"][3] < 0.5 and 0 < got["pSH"][3] < 1 and 0 < got["pRELL"][3] < 0.5
    # two trees alone, equal: every replicate is shared
    rep2, _ = ref.replicates(lnf[:2], w, None, 40, seed=8)
    assert np.allclose(_check(lnf[:2], w, rep2)["pRELL"], 0.5, atol=1e-12)


def test_restated_generator_indices():
    for lg in (1, 2, 7, 100, 4097):
        for g in (0, 3):
            d = ref.draws(5, 2, g, lg)
            assert d.shape == (lg,) and d.min() >= 0 and d.max() < lg
    assert not np.array_equal(ref.draws(5, 2, 0, 100), ref.draws(5, 3, 0, 100))
    assert not np.array_equal(ref.draws(5, 2, 0, 100), ref.draws(5, 2, 1, 100))
    assert not np.array_equal(ref.draws(5, 2, 0, 100), ref.draws(6, 2, 0, 100))
    # 10^6 draws into ten equal cells: each count is binomial(10^6, 0.1), sigma = 300; all within 5 sigma of 10^5
    n = 1_000_000
    cells = np.bincount(ref.draws(12345, 0, 0, n) * 10 // n, minlength=10)
    assert cells.sum() == n and np.all(np.abs(cells - n / 10) < 5 * np.sqrt(n * 0.1 * 0.9)), cells
    # the pattern map: weights -> site list without the empty patterns; genes keep their draws inside
    assert ref.site_list([2, 0, 3]).tolist() == [0, 0, 2, 2, 2]
    c = ref.counts([1, 2, 3, 0, 90], [0, 1, 1, 5], seed=4, n_rep=20)
    assert np.all(c[:, 0] == 1) and np.all(c[:, 3] == 0) and np.all(c.sum(axis=1) == 96)


def test_host_path_is_unchanged():
    """hostlib.tree_comparison(device=False) on golden stewart_two_trees, seed 7: the arrays the host path returned before the table
    arithmetic was split from the resampling (recorded from that commit), bit for bit — also with genes and another replicate count."""
    g = helpers.load_golden("stewart_two_trees")
    lnf, w = np.array(g["logf"]), np.array(g["counts"])
    fh = float.fromhex
    r = hostlib.tree_comparison(lnf, w, seed=7)
    want = dict(li=["-0x1.039682a0ebb3bp+10", "-0x1.010857db0d23cp+10"], dli=["-0x1.471562ef47f80p+3", "0x0.0p+0"],
                se=["0x1.cc7cc9056e4cbp+2", "0x0.0p+0"], pKH=["0x1.3e54278de6748p-4", "-0x1.0000000000000p+0"],
                pSH=["0x1.48e8a71de6a09p-4", "-0x1.0000000000000p+0"], pRELL=["0x1.2a9930be0df1fp-4", "0x1.daacd9e83e121p-1"])
    assert r["best"] == 1
    for k, v in want.items():
        assert r[k].tolist() == [fh(x) for x in v], (k, [x.hex() for x in r[k]])
    r = hostlib.tree_comparison(lnf, w, gene_off=[0, 40, len(w)], n_rep=333, seed=7)
    want.update(pSH=["0x1.3381ec0313384p-4", "-0x1.0000000000000p+0"], pRELL=["0x1.7d4f2ee517d52p-4", "0x1.d0561a235d07ep-1"])
    for k, v in want.items():
        assert r[k].tolist() == [fh(x) for x in v], (k, [x.hex() for x in r[k]])
