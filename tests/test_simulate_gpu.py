"""Simulation under the loaded model on the GPU (paml_amd_simulate, pamlh_simulate, pamlh_lnl --simulate): equal bytes against the numpy
restatement of the draw (tests/simulate_ref.py) fed with the matrices paml_amd_get_pmat returns, at 4 / 20 / 61 states and every
eigen-system kind; the shapes of the walk; independence of batches, first_site and company; the closed loop through the engine's own
likelihood; the engine's state left alone; ABI errors; the host path and the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle
import simulate_ref as ref
from paml_amd import engine, hostlib
from paml_amd.problem import EIGEN_K80, Tree

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")


class Borrowed(engine.Engine):
    """The engine behind a hostlib.Analysis, seen through the Python binding; it stays the analysis's to destroy."""

    def __init__(self, a, K):
        a._L.pamlh_engine_handle.restype = C.c_void_p
        a._L.pamlh_engine_handle.argtypes = [C.c_void_p]
        self._L = engine.lib()
        self._h = C.c_void_p(a._L.pamlh_engine_handle(a._h))
        assert self._h.value
        self.n, self.n_tips, self.n_patt, self.n_genes, self.K, self.n_nodes = a.n, a.n_tips, a.n_patt, 1, K, a.n_nodes

    def close(self):
        self._h = None


def analysis_engine(ctl, program, x=None):
    """(analysis, engine, problem at x) with the model at x on the device as pamlh_eval_gpu sends it."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), program)
    x = np.array(a.default_x() if x is None else x)
    pb = a.problem(x)
    a.eval_gpu(x, want_lnf=False)
    return a, Borrowed(a, pb.K), pb, x


def pmats(eng, K, n_nodes, root):
    P = np.zeros((K, n_nodes, eng.n, eng.n))
    for k in range(K):
        for v in range(n_nodes):
            if v != root:
                P[k, v] = eng.get_pmat(0, k, v)
    return P


def check_bytes(eng, pb, branch, n_sites, seed=5, replicate=1):
    """The device's z, cls and anc against the restatement fed with get_pmat of every (class, node)."""
    t = pb.tree
    got = eng.simulate(branch, n_sites, seed=seed, replicate=replicate, want_classes=True, want_ancestors=True)
    P = pmats(eng, pb.K, t.n_nodes, t.root)
    want = ref.simulate(np.asarray(pb.pi).reshape(-1)[:pb.n], pb.freqK, P, t.sons, t.root, t.n_tips, n_sites, seed=seed, replicate=replicate)
    for key in ("cls", "z", "anc"):
        assert got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), (key, np.argwhere(got[key] != want[key])[:5])
    return got


@pytest.mark.parametrize("n_sites", [4097, 1])
def test_equal_bytes_61_states(n_sites):
    """HIV M2a: 13 taxa, K = 3, eigen systems decomposed on the device; 4097 = a multiple of 64 plus one."""
    a, eng, pb, x = analysis_engine("hiv_ns2.ctl", "codeml", helpers.load_golden("hiv_m2a")["x"])
    assert (pb.n, pb.tree.n_tips, pb.K) == (61, 13, 3)
    n_dec = C.c_long()
    eng._L.paml_amd_eigen_counters(eng._h, C.byref(n_dec), None, 0)
    assert n_dec.value > 0      # the device decomposed
    got = check_bytes(eng, pb, pb.tree.branch, n_sites)
    if n_sites > 1:
        assert len(np.unique(got["cls"])) == 3 and got["z"].max() > 40


def _k80_problem():
    pb = helpers.random_problem(4, 7, 10, K=4, seed=3)
    pb.eigen = [dict(kind=EIGEN_K80, kappa=2.5)]
    pb.pi = np.full((1, 4), 0.25)
    return pb


@pytest.mark.parametrize("case", ["hky85_cijk_g4", "k80", "unrest", "lg_g4"])
def test_equal_bytes_4_and_20_states(case):
    if case == "k80":
        pb = _k80_problem()
        eng = engine.engine_for(pb)
    else:
        ctl, prog = {"hky85_cijk_g4": ("brown_hky85_g4.ctl", "baseml"), "unrest": ("brown_unrest.ctl", "baseml"),
                     "lg_g4": ("stewart_lg_g4.ctl", "codeml")}[case]
        a, eng, pb, x = analysis_engine(ctl, prog)
    check_bytes(eng, pb, pb.tree.branch, 1000)


def _shape_problem(shape):
    if shape == "tip_root":      # a rooted tree whose root is tip 0: 0 -> 4 -> (1, 5 -> (2, 3))
        pb = helpers.random_problem(4, 4, 5, K=2, seed=11)
        pb.tree = Tree(4, 6, 0, [[4], [], [], [], [1, 5], [2, 3]], np.array([0.0, 0.2, 0.3, 0.1, 0.25, 0.15]), np.zeros(6, dtype=np.int32))
    elif shape == "polytomy5":   # 7 -> (0, 1, 2, 3, 8 -> (4, 5, 6))
        pb = helpers.random_problem(20, 7, 5, K=2, seed=12)
        pb.tree = Tree(7, 9, 7, [[], [], [], [], [], [], [], [0, 1, 2, 3, 8], [4, 5, 6]], np.array([0.1, 0.2, 0.3, 0.15, 0.25, 0.05, 0.4, 0.0, 0.2]),
                       np.zeros(9, dtype=np.int32))
    elif shape == "taxa40":      # 78 nodes: past the tile of node states kept in LDS
        pb = helpers.random_problem(4, 40, 8, K=2, seed=13)
    elif shape == "taxa40_20states":
        pb = helpers.random_problem(20, 40, 8, K=1, seed=14)
    else:                        # 61 states, 11 classes: the tables of a node do not fit LDS
        pb = helpers.random_problem(61, 6, 5, K=11, seed=15)
    return pb


@pytest.mark.parametrize("shape", ["tip_root", "polytomy5", "taxa40", "taxa40_20states", "codon_k11"])
def test_shapes_of_the_walk(shape):
    pb = _shape_problem(shape)
    eng = engine.Engine(pb.n, pb.tree.n_tips, pb.n_patt, max_classes=pb.K)
    eng.set_tree(pb.tree)      # no tips: the simulation needs none
    eng.set_pi(pb.pi)
    for i, e in enumerate(pb.eigen):
        eng.set_eigen(i, e)
    eng.set_classes(pb.mode, pb.freqK, pb.rate, pb.eigen_of, pb.qfactor)
    got = check_bytes(eng, pb, pb.tree.branch, 300)
    if shape == "tip_root":
        assert len(np.unique(got["z"][0])) > 1      # the root's drawn states are that tip's sequence


def test_independence_of_company(monkeypatch):
    a, eng, pb, x = analysis_engine("hiv_ns0.ctl", "codeml", helpers.load_golden("hiv_m0")["x"])
    br = pb.tree.branch
    whole = eng.simulate(br, 20000, seed=9, want_classes=True, want_ancestors=True)
    assert engine.simulate_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_SIM_ARENA_MB", "0.2")
    parts = eng.simulate(br, 20000, seed=9, want_classes=True, want_ancestors=True)
    info = engine.simulate_info()
    assert info["last_batches"] >= 3 and info["last_kernel_ms"] > 0, info
    monkeypatch.delenv("PAML_AMD_SIM_ARENA_MB")
    for key in ("z", "cls", "anc"):
        assert np.array_equal(parts[key], whole[key]), key
    window = eng.simulate(br, 100, seed=9, first_site=5000, want_classes=True, want_ancestors=True)
    for key in ("z", "cls", "anc"):
        assert np.array_equal(window[key], whole[key][..., 5000:5100]), key
    other = eng.simulate(br, 20000, seed=9, replicate=1)
    assert not np.array_equal(other["z"], whole["z"])
    assert np.array_equal(eng.simulate(br, 20000, seed=9, replicate=1)["z"], other["z"])
    assert np.array_equal(eng.simulate(br, 20000, seed=9)["z"], whole["z"])


def test_closed_loop_on_the_device():
    """The configuration of the CPU test through the engine: the pattern counts of 10^6 sites equal the restatement's (fed with the engine's
    matrices), so Pearson's X^2 against the oracle's probabilities stays below the same bound; and the engine's own likelihood of the
    64-pattern alignment reproduces those probabilities to 1e-12."""
    pb, _ = ref.star_case()
    prob = np.exp(oracle.evaluate(pb)["lnf"])
    eng = engine.engine_for(pb)
    out = eng.eval(pb.tree.branch, want_lnf=True)
    assert np.max(np.abs(np.exp(out["lnf"]) - prob)) <= 1e-12
    n_sites = 10 ** 6
    got = eng.simulate(pb.tree.branch, n_sites, seed=1)
    want = ref.simulate(pb.pi[0], pb.freqK, pmats(eng, 2, 4, 3), pb.tree.sons, 3, 3, n_sites, seed=1)
    counts = ref.pattern_counts(got["z"])
    assert np.array_equal(counts, ref.pattern_counts(want["z"]))
    expected = prob * n_sites
    x2 = float(((counts - expected) ** 2 / expected).sum())
    print("X2 = %.2f, bound = %.2f" % (x2, ref.chi2_bound(63, 6.0)))
    assert x2 < ref.chi2_bound(63, 6.0)


def test_state_untouched():
    a, eng, pb, x = analysis_engine("hiv_ns2.ctl", "codeml", helpers.load_golden("hiv_m2a")["x"])
    l1 = a.eval_gpu(x, want_lnf=False)[0]
    p1 = eng.get_pmat(0, 1, 5)
    eng.simulate(pb.tree.branch * 1.3, 500, seed=2)
    ps = eng.get_pmat(0, 1, 5)
    assert not np.array_equal(ps, p1)      # the simulation's own matrices
    l2 = a.eval_gpu(x, want_lnf=False)[0]
    assert l2 == l1
    assert np.array_equal(eng.get_pmat(0, 1, 5), p1)


def _code(exc):
    return int(str(exc.value).rsplit("(code ", 1)[1].rstrip(")"))


def test_errors():
    pb = _k80_problem()
    eng = engine.engine_for(pb)
    br = pb.tree.branch
    with pytest.raises(engine.EngineError) as ex:
        eng.simulate(br, 0)
    assert _code(ex) == -1
    L = engine.lib()
    L.paml_amd_simulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.paml_amd_simulate(eng._h, br.ctypes.data_as(C.c_void_p), None, 10, 0, 1, 0, None, None, None) == -1      # a null z
    with pytest.raises(engine.EngineError) as ex:
        eng.simulate(br, 10, first_site=-1)
    assert _code(ex) == -1
    two = engine.Engine(4, pb.tree.n_tips, pb.n_patt, max_classes=4, n_genes=2)
    with pytest.raises(engine.EngineError) as ex:
        two.simulate(br, 10)
    assert _code(ex) == -4 and "one gene" in str(ex.value)
    bare = engine.Engine(4, pb.tree.n_tips, pb.n_patt, max_classes=4)
    bare.set_tree(pb.tree)
    bare.set_pi(pb.pi)
    bare.set_eigen(0, pb.eigen[0])
    with pytest.raises(engine.EngineError) as ex:
        bare.simulate(br, 10)      # no set_classes yet
    assert _code(ex) == -1
    z = np.zeros((1, 1), dtype=np.uint8)
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85_adg.ctl"), "baseml")
    with pytest.raises(RuntimeError, match="rho"):
        a.simulate(a.default_x(), 10)
    b = hostlib.Analysis(os.path.join(CTL, "pairwise_hiv_f3x4.ctl"), "codeml")
    with pytest.raises(RuntimeError, match="runmode = -2"):
        b.simulate(None, 10)
    del z


def test_host_path_and_driver(tmp_path):
    g = helpers.load_golden("hiv_m0")
    a, eng, pb, x = analysis_engine("hiv_ns0.ctl", "codeml", g["x"])
    host = a.simulate(x, 300, seed=4, replicate=2)
    dev = eng.simulate(pb.tree.branch, 300, seed=4, replicate=2, want_classes=True)
    assert np.array_equal(host["z"], dev["z"]) and np.array_equal(host["cls"], dev["cls"])
    assert a.simulate(x, None, seed=4)["z"].shape == (a.n_tips, len(a.pose()))
    out = str(tmp_path / "sim.phy")
    r = subprocess.run([hostlib.DRIVER_PATH, "codeml", os.path.join(CTL, "hiv_ns0.ctl"), "--simulate", out, "--sites", "200", "--seed", "4"] +
                       ["%.6f" % v for v in x], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    b = hostlib.Analysis(os.path.join(CTL, "hiv_ns0.ctl"), "codeml", overrides="seqfile = " + out)
    assert len(b.pose()) == 200
    lnl = b.eval_gpu(x, want_lnf=False)[0]
    assert np.isfinite(lnl) and lnl < 0
    r = subprocess.run([hostlib.DRIVER_PATH, "codeml", os.path.join(CTL, "hiv_ns0.ctl"), "--simulate", out, "--sites", "50", "--replicates", "2"] +
                       ["%.6f" % v for v in x], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and os.path.exists(out + ".0000") and os.path.exists(out + ".0001"), r.stderr.decode()[-2000:]
