"""Bootstrap replicates of the tree comparison on the GPU (paml_amd_rell_replicates, pamlh_tree_comparison_gpu, pamlh_lnl --rell-gpu):
exact draw counts against the numpy restatement of the generator (tests/rell_ref.py), tree padding and tree blocks, determinism and
independence of n_rep / batches, a size over many chunks and workgroups, the reference's table, ABI errors, the driver."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import rell_ref as ref
from paml_amd import engine, hostlib

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
CHUNK = engine.rell_info()["chunk"]
TREE_BLOCK = engine.rell_info()["tree_block"]


def _spread(ls):
    """Five patterns with ls sites in all."""
    return [ls - 10, 1, 2, 3, 4]


# (weights, gene_off): the smallest shapes that can go wrong
COUNT_CASES = {
    "one_pattern": ([7], None),
    "five_patterns": ([1, 2, 3, 4, 90], None),
    "zero_weights": ([3, 1, 4, 0, 5, 9, 0], None),
    "chunk_minus_1": (_spread(CHUNK - 1), None),
    "chunk": (_spread(CHUNK), None),
    "chunk_plus_1": (_spread(CHUNK + 1), None),
    "three_chunks_17": (_spread(3 * CHUNK + 17), None),
    "gene_of_one_site": ([1, 2, 3, 4, 90], [0, 1, 5]),
    "empty_gene": ([3, 1, 4, 0, 5, 9, 0], [0, 2, 2, 7]),
    "gene_of_zero_weights": ([3, 1, 4, 0, 5, 9, 0], [0, 3, 4, 7]),
    "genes_across_chunks": (_spread(CHUNK + 1) + [5, 0, CHUNK], [0, 2, 6, 8]),
}


@functools.lru_cache(maxsize=None)
def _want_counts(name, n_rep, seed=11):
    w, go = COUNT_CASES[name]
    return ref.counts(w, go, seed, n_rep)


@pytest.mark.parametrize("n_rep", [1, 3, 1000])
@pytest.mark.parametrize("name", sorted(COUNT_CASES))
def test_exact_counts(name, n_rep):
    """lnf = the identity makes rep[r][t] the number of times pattern t was drawn: integers, exact in any summation order."""
    w, go = COUNT_CASES[name]
    n = len(w)
    got = engine.rell_replicates(np.eye(n), w, gene_off=go, n_rep=n_rep, seed=11)
    want = _want_counts(name, n_rep)
    assert got.shape == (n_rep, n)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[:2], want[:2])
    assert np.all(got.sum(axis=1) == sum(w))
    off = go or [0, n]
    for g in range(len(off) - 1):      # sites are drawn inside their gene
        assert np.all(got[:, off[g]:off[g + 1]].sum(axis=1) == sum(w[off[g]:off[g + 1]])), g
    assert np.all(got[:, np.array(w) == 0] == 0)


@pytest.mark.parametrize("n_trees", [1, 2, 3, 7, 9, TREE_BLOCK + 1, 2 * TREE_BLOCK + 1])
def test_tree_padding_and_blocks(n_trees):
    """Every T_pad (2, 4, 8, 16 = two tree blocks, 32) against the restatement: |got - want| <= 1e-11 * sum |lnf of the draws| per entry —
    twenty times the worst-case bound n * eps of 5 000 FP64 additions (5000 * 1.1e-16 = 5.5e-13), which covers both summation orders."""
    rng = np.random.default_rng(100 + n_trees)
    n_patt = 37
    w = rng.integers(0, 270, n_patt)      # about 5 000 sites
    lnf = rng.uniform(-30, -1, (n_trees, n_patt))
    got = engine.rell_replicates(lnf, w, n_rep=64, seed=5)
    want, mag = ref.replicates(lnf, w, None, 64, 5)
    err = np.abs(got - want)
    print("n_trees %d ls %d: max err / sum|lnf| = %.3e" % (n_trees, w.sum(), (err / mag).max()))
    assert got.shape == want.shape and np.all(err <= 1e-11 * mag)


def _det_case():
    rng = np.random.default_rng(3)
    w = rng.integers(0, 40, 900)      # ~ 17 000 sites: five chunks
    return rng.uniform(-30, -1, (3, 900)), w, [0, 300, 300, 900]


def test_determinism_and_independence_of_n_rep():
    lnf, w, go = _det_case()
    a = engine.rell_replicates(lnf, w, gene_off=go, n_rep=1000, seed=9)
    b = engine.rell_replicates(lnf, w, gene_off=go, n_rep=1000, seed=9)
    assert np.array_equal(a, b)                                  # two calls: equal bits
    c = engine.rell_replicates(lnf, w, gene_off=go, n_rep=10, seed=9)
    assert np.array_equal(a[:10], c)                             # replicate r does not depend on n_rep
    d = engine.rell_replicates(lnf, w, gene_off=go, n_rep=1000, seed=10)
    assert np.all(np.any(a != d, axis=1))                        # another seed changes every row
    assert len({row.tobytes() for row in a}) == 1000             # and the replicates of one call differ from each other


def test_batches_give_the_same_bits():
    lnf, w, go = _det_case()
    a = engine.rell_replicates(lnf, w, gene_off=go, n_rep=50, seed=9)
    assert engine.rell_info()["last_batches"] == 1
    n_chunks = -(-int(w.sum()) // CHUNK)
    per_rep = n_chunks * 4 * 8                                   # chunk sums of one replicate at T_pad = 4
    b = engine.rell_replicates(lnf, w, gene_off=go, n_rep=50, seed=9, arena_mb=7.5 * per_rep / 2 ** 20)      # room for 7 replicates
    assert engine.rell_info()["last_batches"] == 8
    assert np.array_equal(a, b)
    c = engine.rell_replicates(lnf, w, gene_off=go, n_rep=50, seed=9, arena_mb=1e-9)      # less than one replicate: one at a time
    assert engine.rell_info()["last_batches"] == 50 and np.array_equal(a, c)


def test_many_chunks_and_workgroups():
    """100 000 patterns, ~3e5 sites (74 chunks a replicate, two-level scan over 49 tiles): the same relative bound with n = ls —
    1e-11 against n * eps = 3e5 * 1.1e-16 = 3.3e-11 in the worst case of one running sum; the device adds at most 64 + 6 + 74 terms into
    any one accumulator and the restatement sums through counts (1e5 terms), so 1e5 * 1.1e-16 = 1.1e-11 bounds both; asserted at 1e-11
    as the issue sets it."""
    rng = np.random.default_rng(4)
    n_patt = 100_000
    w = 1 + np.arange(n_patt) % 5
    lnf = rng.uniform(-30, -1, (3, n_patt))
    got = engine.rell_replicates(lnf, w, n_rep=64, seed=21)
    want, mag = ref.replicates(lnf, w, None, 64, 21)
    err = np.abs(got - want)
    print("ls %d: max err / sum|lnf| = %.3e" % (w.sum(), (err / mag).max()))
    assert np.all(err <= 1e-11 * mag)


def test_the_reference_table_with_device_replicates():
    """Golden stewart_two_trees: li, Dli, SE, pKH to the printed digits, pSH and pRELL of 10 000 device replicates within 0.012 (3 sigma of
    10 000 draws at p = 0.08) — the bounds of the host path's test."""
    g = helpers.load_golden("stewart_two_trees")
    lnf, w = np.array(g["logf"]), np.array(g["counts"])
    r = hostlib.tree_comparison(lnf, w, device=True, seed=7)
    assert r["best"] == 1
    for t, row in enumerate(g["table"]):
        assert abs(r["li"][t] - row["li"]) < 6e-4 and abs(r["dli"][t] - row["dli"]) < 6e-4 and abs(r["se"][t] - row["se"]) < 6e-4
        assert abs(r["pKH"][t] - row["pKH"]) < 6e-4
        assert abs(r["pSH"][t] - row["pSH"]) < 0.012 and abs(r["pRELL"][t] - row["pRELL"]) < 0.012, (t, r["pSH"], r["pRELL"])
    assert abs(r["pRELL"].sum() - 1) < 1e-9
    # n_rep = 0 is 10 000 on this path: the columns are those of the table arithmetic on the device's 10 000 replicates
    rep = engine.rell_replicates(lnf, w, n_rep=10000, seed=7)
    r1 = hostlib.tree_comparison_from_replicates(lnf, w, rep)
    assert np.array_equal(r1["pRELL"], r["pRELL"]) and np.array_equal(r1["pSH"], r["pSH"])
    r3 = hostlib.tree_comparison(lnf, w, gene_off=[0, 40, len(w)], device=True, seed=7)
    assert np.array_equal(r3["se"], r["se"])      # stratified resampling leaves the deterministic columns alone


@pytest.mark.parametrize("kw, msg", [
    (dict(lnf=np.zeros((0, 3))), "n_trees = 0 < 1"),
    (dict(lnf=np.zeros((2, 0)), w=[]), "n_patt = 0 < 1"),
    (dict(n_rep=0), "n_rep = 0 < 1"),
    (dict(w=[1, -2, 1]), "weight of pattern 1 is negative"),
    (dict(w=[1, 1, 2.5]), "weight of pattern 2 is not an integer"),
    (dict(w=[2.0 ** 31, 1, 1]), "weight of pattern 0 is 2^31 or more"),
    (dict(w=[0, 0, 0]), "no sites"),
    (dict(gene_off=[1, 2, 3]), "gene_off does not run from 0 to n_patt"),
    (dict(gene_off=[0, 2, 4]), "gene_off does not run from 0 to n_patt"),
    (dict(gene_off=[0, 2, 1, 3]), "gene_off decreases at gene 1"),
])
def test_errors(kw, msg):
    a = dict(lnf=np.zeros((2, 3)), w=[1, 1, 1], n_rep=4)
    a.update(kw)
    with pytest.raises(engine.EngineError) as e:
        engine.rell_replicates(**a)
    assert msg in str(e.value) and "code -1" in str(e.value)
    assert engine.rell_replicates(np.zeros((2, 3)), [1, 1, 1], n_rep=4).shape == (4, 2)      # and the next call is not affected


ROW = r"^\s*(\d+)(\*?)\s+(-?[0-9.]+)\s+(-?[0-9.]+)\s+(-?[0-9.]+)\s+(-?[0-9.]+)\s+(-?[0-9.]+)\s+(-?[0-9.]+)\s*$"


def test_driver_rell_gpu(tmp_path):
    """`pamlh_lnl codeml <ctl> --all-trees --rell-gpu`: the table of the stewart two-tree case with its bootstrap columns from 10 000
    device replicates, their number printed under it; without the flag the output is the host path's table and nothing more."""
    g = helpers.load_golden("stewart_two_trees")
    data = os.path.join(helpers.GOLDEN, "data")
    (tmp_path / "two.trees").write_text(open(os.path.join(data, "stewart.trees")).read().replace("6  1", "6  2", 1))
    ctl = open(os.path.join(CTL, "stewart_lg_g4.ctl")).read().replace("../data/stewart.aa", os.path.join(data, "stewart.aa"))
    ctl = ctl.replace("../data/lg.dat", os.path.join(data, "lg.dat")).replace("../data/stewart.trees", str(tmp_path / "two.trees"))
    (tmp_path / "two.ctl").write_text(ctl)
    cmd = ["timeout", "-k", "10", "300", hostlib.DRIVER_PATH, "codeml", str(tmp_path / "two.ctl"), "--all-trees"]
    out = subprocess.run(cmd + ["--rell-gpu"], cwd=tmp_path, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = re.findall(ROW, out.stdout, re.M)
    assert len(rows) == 2 and rows[1][1] == "*", out.stdout
    assert re.findall(r"from (\d+) bootstrap replicates drawn on the GPU", out.stdout) == ["10000"]
    for r, want in zip(rows, g["table"]):
        assert abs(float(r[2]) - want["li"]) < 2e-3 and abs(float(r[3]) - want["dli"]) < 2e-3 and abs(float(r[4]) - want["se"]) < 2e-3
        assert abs(float(r[5]) - want["pKH"]) < 2e-3
        assert abs(float(r[6]) - want["pSH"]) < 0.012 and abs(float(r[7]) - want["pRELL"]) < 0.012
    few = subprocess.run(cmd + ["--rell-gpu", "--replicates", "300"], cwd=tmp_path, capture_output=True, text=True)
    assert few.returncode == 0 and re.findall(r"from (\d+) bootstrap replicates", few.stdout) == ["300"]
    # without the flag: the same lines up to the bootstrap columns, no replicate line
    plain = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert "replicates" not in plain.stdout
    prow = re.findall(ROW, plain.stdout, re.M)
    assert [r[:6] for r in prow] == [r[:6] for r in rows]
    assert len(plain.stdout.splitlines()) == len(out.stdout.splitlines()) - 2      # the blank line and the replicate line
    for r, want in zip(prow, g["table"]):
        assert abs(float(r[7]) - want["pRELL"]) < 0.012
