"""Ancestral reconstruction at every internal node in one call (paml_amd_ancestral_marginal / paml_amd_ancestral_joint, their host-layer
and driver forms): the marginal against the oracle's node_posterior at rtol 1e-9 / atol 1e-13 (test_node_posterior_matches_oracle's
tolerances), the joint against the numpy restatement (tests/ancestral_ref.py) fed with the matrices paml_amd_get_pmat returns, at 1e-9
absolute (the project's tolerance for ln f_h), and both against the reference's own reconstruction of brown.nuc."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle
import ancestral_ref as ar
from paml_amd import engine, hostlib
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT, Tree

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")


def _check_marginal(pb, eng=None, ref_pb=None):
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.ancestral_marginal(t.branch, pb.gene_rate)
    post, best, prob = got["post"], got["best"], got["prob"]
    for qi, node in enumerate(range(t.n_tips, t.n_nodes)):
        ref = oracle.node_posterior(ref_pb or pb, node)
        err = float(np.max(np.abs(post[qi] - ref)))
        print("node %d: max abs error %.3e" % (node, err))
        assert np.allclose(post[qi], ref, rtol=1e-9, atol=1e-13), (node, err)
    assert np.allclose(post.sum(axis=2), 1)
    assert np.array_equal(best, np.argmax(post, axis=2))
    assert np.array_equal(prob.view(np.uint64), np.take_along_axis(post, best[:, :, None].astype(np.int64), axis=2)[:, :, 0].view(np.uint64))
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    return eng, got


@pytest.mark.parametrize("n,K,amb,every,extra", [
    (4, 1, False, None, {}), (4, 3, True, 3, {}), (5, 2, False, None, {}), (20, 2, False, None, {}), (61, 2, True, None, {}),
    (61, 1, False, 4, {}), (4, 2, False, None, dict(n_genes=2)), (20, 1, False, None, dict(polytomy=True))])
def test_marginal_matches_the_oracle_at_every_node(n, K, amb, every, extra):
    _check_marginal(helpers.random_problem(n, 9, 140, K=K, seed=51 + n, ambiguity=amb, scale_every=every, **extra))


def test_marginal_deep_tree_with_rescaling():
    """40 tips x 70 patterns at 20 states, a scaling node every 8: the deepest outer chain and its rescaling."""
    _check_marginal(helpers.random_problem(20, 40, 70, K=1, seed=77, scale_every=8))


def test_marginal_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernel's split)."""
    pb = helpers.random_problem(20, 9, 140, K=2, seed=71)
    _check_marginal(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


def test_marginal_subset_and_no_post():
    pb = helpers.random_problem(61, 9, 140, K=2, seed=112, ambiguity=True)
    t = pb.tree
    eng = engine_for(pb)
    full = eng.ancestral_marginal(t.branch, pb.gene_rate)
    sub = eng.ancestral_marginal(t.branch, pb.gene_rate, nodes=[t.n_nodes - 1, t.root])
    for qi, node in enumerate([t.n_nodes - 1, t.root]):
        for key in ("best", "prob", "post"):
            assert np.array_equal(sub[key][qi], full[key][node - t.n_tips]), (node, key)
    nop = eng.ancestral_marginal(t.branch, pb.gene_rate, want_post=False)
    assert nop["post"] is None and np.array_equal(nop["best"], full["best"]) and np.array_equal(nop["prob"], full["prob"])


def _rooted_at_tip0(pb):
    """pb with its tree re-rooted at tip 0 (the same unrooted tree and branch lengths)."""
    t = pb.tree
    father = [-1] * t.n_nodes
    for v in range(t.n_nodes):
        for s in t.sons[v]:
            father[s] = v
    nbr = [list(t.sons[v]) + ([father[v]] if father[v] >= 0 else []) for v in range(t.n_nodes)]
    length = lambda a, b: t.branch[a] if father[a] == b else t.branch[b]
    sons, branch = [[] for _ in range(t.n_nodes)], np.zeros(t.n_nodes)
    stack = [(0, -1)]
    while stack:
        v, par = stack.pop()
        for w in nbr[v]:
            if w != par:
                sons[v].append(w)
                branch[w] = length(v, w)
                stack.append((w, v))
    q = copy.copy(pb)
    q.tree = Tree(t.n_tips, t.n_nodes, 0, sons, branch, t.label.copy())
    return q


def test_marginal_on_a_tree_rooted_at_a_tip():
    """The tree re-rooted at tip 0 (clean data: a root that is a tip is a clean sequence everywhere in the project).  The oracle's
    node_posterior is taken on the SAME tree in its original rooting: the model is reversible, so the posteriors at a node do not depend on
    where the root sits, and orc_node_posterior itself does not take a root that is a tip (on this case it differs from its own values
    for the original rooting by up to 0.78, while its lnL of the two rootings is the same to the last bit)."""
    pb0 = helpers.random_problem(4, 9, 140, K=2, seed=55)
    _check_marginal(_rooted_at_tip0(pb0), ref_pb=pb0)


def test_marginal_on_a_tree_rooted_at_a_tip_on_the_matrix_cores():
    """... at 61 states, two classes: the father that is a tip in the matrix-core kernel (the same reference as above)."""
    pb0 = helpers.random_problem(61, 9, 140, K=2, seed=56)
    _check_marginal(_rooted_at_tip0(pb0), ref_pb=pb0)


def test_marginal_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_ANC_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips (test_ancestral_cpu.py): several batches, equal bytes."""
    pb = helpers.random_problem(61, 9, 3000, K=1, seed=13)
    t = pb.tree
    eng = engine_for(pb)
    one = eng.ancestral_marginal(t.branch, pb.gene_rate)
    assert engine.ancestral_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_ANC_ARENA_MB", "1")
    many = eng.ancestral_marginal(t.branch, pb.gene_rate)
    assert engine.ancestral_info()["last_batches"] > 1
    for key in ("best", "prob", "post"):
        assert one[key].tobytes() == many[key].tobytes(), key
    ref = oracle.node_posterior(pb, t.root)
    assert np.allclose(one["post"][t.root - t.n_tips], ref, rtol=1e-9, atol=1e-13)


def _check_joint(pb):
    t = pb.tree
    eng = engine_for(pb)
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.ancestral_joint(t.branch, pb.gene_rate)
    P, tips = ar.matrices_from_engine(eng, pb), ar.tips_of(pb)      # (get_pmat works after the joint call)
    states, ln_best = ar.joint(P, pb.pi, tips, t)
    err = float(np.max(np.abs(got["ln_best"] - ln_best)))
    score = ar.joint_score(P, pb.pi, tips, t, got["states"])
    print("ln_best: max abs error %.3e; score of the returned states against the optimum: %.3e" % (err, float(np.max(np.abs(score - ln_best)))))
    assert err <= 1e-9
    assert np.max(np.abs(score - ln_best)) <= 1e-9      # every pattern: no exclusion rule for near-ties
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    return eng, got, (P, tips, states, ln_best)


@pytest.mark.parametrize("n", [4, 20, 61])
@pytest.mark.parametrize("amb", [False, True])
def test_joint_matches_the_restatement(n, amb):
    _check_joint(helpers.random_problem(n, 9, 140, seed=90 + n, ambiguity=amb))


def test_joint_two_genes():
    _check_joint(helpers.random_problem(4, 9, 140, seed=94, n_genes=2))


def test_joint_polytomous_root():
    _check_joint(helpers.random_problem(20, 9, 140, seed=95, polytomy=True))


def test_joint_tip_root():
    _check_joint(_rooted_at_tip0(helpers.random_problem(4, 9, 140, seed=96)))


def test_joint_tip_root_at_61_states():
    _check_joint(_rooted_at_tip0(helpers.random_problem(61, 9, 140, seed=98)))


def test_joint_large_tree_where_the_product_form_underflows():
    """120 tips x 40 patterns at 20 states, scaling every 10: probabilities around e^-400 and below per pattern."""
    eng, got, _ = _check_joint(helpers.random_problem(20, 120, 40, seed=97, scale_every=10))
    assert np.all(np.isfinite(got["ln_best"]))


def test_joint_batches_have_the_same_bytes(monkeypatch):
    pb = helpers.random_problem(61, 9, 3000, seed=14)
    eng = engine_for(pb)
    one = eng.ancestral_joint(pb.tree.branch)
    monkeypatch.setenv("PAML_AMD_ANC_ARENA_MB", "1")
    many = eng.ancestral_joint(pb.tree.branch)
    assert engine.ancestral_info()["last_batches"] > 1
    assert one["states"].tobytes() == many["states"].tobytes() and one["ln_best"].tobytes() == many["ln_best"].tobytes()


def _raw(eng):
    L = eng._L
    L.paml_amd_ancestral_marginal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.paml_amd_ancestral_joint.argtypes = [C.c_void_p] * 5
    return L


def test_argument_errors_and_state():
    pb = helpers.random_problem(4, 9, 140, seed=3)
    t = pb.tree
    eng = engine_for(pb)
    L = _raw(eng)
    ni = t.n_nodes - t.n_tips
    br = np.ascontiguousarray(t.branch)
    best, prob = np.zeros((ni, 140), dtype=np.uint8), np.zeros((ni, 140))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1

    def bad(rc, code):
        assert rc == code, rc
        assert L.paml_amd_last_error(eng._h).decode().startswith("ancestral_")
    bad(L.paml_amd_ancestral_marginal(eng._h, None, None, 0, None, p(best), p(prob), None), EINVAL)
    bad(L.paml_amd_ancestral_marginal(eng._h, p(br), None, 0, None, None, p(prob), None), EINVAL)
    bad(L.paml_amd_ancestral_marginal(eng._h, p(br), None, 0, None, p(best), None, None), EINVAL)
    bad(L.paml_amd_ancestral_joint(eng._h, None, None, p(best), p(prob)), EINVAL)
    bad(L.paml_amd_ancestral_joint(eng._h, p(br), None, None, p(prob)), EINVAL)
    bad(L.paml_amd_ancestral_joint(eng._h, p(br), None, p(best), None), EINVAL)
    for nodes in ([], [0], [t.n_nodes], [-1], [t.root, t.root]):
        nd = np.array(nodes + [0], dtype=np.int32)
        bad(L.paml_amd_ancestral_marginal(eng._h, p(br), None, len(nodes), p(nd), p(best), p(prob), None), EINVAL)
    # a model that is not set yet
    fresh = engine.Engine(4, 9, 140)
    bad(_raw(fresh).paml_amd_ancestral_marginal(fresh._h, p(br), None, 0, None, p(best), p(prob), None), EINVAL)
    bad(_raw(fresh).paml_amd_ancestral_joint(fresh._h, p(br), None, p(best), p(prob)), EINVAL)
    # the state either call leaves: get_pmat after the joint call, refused after the marginal one; eval_branch recomputes and agrees
    b = t.n_tips + 1
    ts = np.array([t.branch[b], 0.2])
    before = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
    eng.ancestral_joint(t.branch)
    assert np.allclose(eng.get_pmat(0, 0, 1), oracle.pmat_branch(pb, 0, 0, 1), atol=1e-13)
    after = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    eng.ancestral_marginal(t.branch)
    with pytest.raises(engine.EngineError):
        eng.get_pmat(0, 0, 1)
    after = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    eng.eval(t.branch)
    eng.get_pmat(0, 0, 1)


def test_joint_refuses_classes_and_marginal_refuses_rate_matrices():
    pb = helpers.random_problem(4, 9, 140, K=2, seed=4)
    eng = engine_for(pb)
    with pytest.raises(engine.EngineError, match="one class"):
        eng.ancestral_joint(pb.tree.branch)
    pq = helpers.random_problem(4, 9, 140, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    eng = engine_for(pq)
    with pytest.raises(engine.EngineError, match="reversible"):
        eng.ancestral_marginal(pq.tree.branch)


# ---- the reference's own reconstruction of brown.nuc, the host layer and the driver --------------------------------------------------

def test_marginal_reproduces_the_reference_reconstruction():
    from test_oracle_golden import _brown_anc
    g, pb, raw = _brown_anc()
    got = engine_for(pb).ancestral_marginal(pb.tree.branch)
    for k, node in enumerate(g["nodes_1based"]):
        qi = node - 1 - pb.tree.n_tips
        for h, patt in enumerate(raw):
            row = g["patterns"][patt]
            assert "TCAG"[got["best"][qi, h]] == row["best"][k] and abs(got["prob"][qi, h] - row["prob"][k]) < 6e-4


def test_host_layer_joint_matches_the_reference_rst_and_the_host_routine():
    g = helpers.load_golden("brown_hky85_joint")
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
    x = np.array(g["x"])
    st_host, pr_host = a.joint_reconstruction(x)
    got = a.ancestral_joint(x)
    pb = a.problem(x)
    lnf = oracle.evaluate(pb)["lnf"]
    pr = np.exp(got["ln_best"] - lnf)
    swaps = 0
    for h in range(a.n_patt):
        row = g["patterns"]["".join("TCAG"[c] for c in pb.z[:, h])]
        mine = "".join("TCAG"[c] for c in got["states"][:, h])
        assert abs(pr[h] - row["prob"]) < 6e-4, (h, pr[h], row)
        swaps += mine != row["best"]
        assert mine == row["best"] or row["prob"] < 0.51
    assert swaps <= 1
    assert np.allclose(pr, pr_host, rtol=1e-9)
    P, tips = np.stack([[np.stack([oracle.pmat_branch(pb, 0, 0, v) if v != pb.tree.root else np.eye(4) for v in range(pb.tree.n_nodes)])]]), ar.tips_of(pb)
    clear = ar.second_best_gap(P, pb.pi, tips, pb.tree) > 1e-6
    assert clear.mean() >= 0.95
    assert np.array_equal(got["states"].T[clear], st_host[clear])
    m = a.ancestral_marginal(x)
    for qi, node in enumerate(range(a.n_tips, a.n_nodes)):
        assert np.allclose(m["post"][qi], a.node_posterior(x, node), rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("ctl,prog,n", [("brown_hky85.ctl", "baseml", 4), ("mtcdnapri_jtt.ctl", "codeml", 20), ("hiv_ns0.ctl", "codeml", 61)])
def test_device_joint_agrees_with_the_host_joint_reconstruction(ctl, prog, n):
    """The device joint against the host's existing pamlh_joint_reconstruction at 4, 20 and 61 states.  The host routine takes an analysis
    read from a control file, so the cases are the committed clean-data, one-class analyses of brown.nuc (5 taxa), mtCDNApri.aa (7) and
    HIVenvSweden (13) at the control file's initial values, in place of random 9-tip problems: exp(ln_best - ln f_h) and the states
    agree wherever the restatement's best and second-best assignments differ by more than 1e-6 in log; at most 5 % of the patterns may
    be excluded that way (on the CPU, with the oracle's matrices, none is at these three)."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = a.default_x()
    pb = a.problem(x)
    assert a.n == n and pb.K == 1 and pb.cleandata
    st_host, pr_host = a.joint_reconstruction(x)
    got = a.ancestral_joint(x)
    pr = np.exp(got["ln_best"] - oracle.evaluate(pb)["lnf"])
    clear = ar.second_best_gap(ar.matrices_from_oracle(pb), pb.pi, ar.tips_of(pb), pb.tree) > 1e-6
    print("%s: excluded %d of %d patterns; max relative difference of the probabilities %.3e"
          % (ctl, int((~clear).sum()), a.n_patt, float(np.max(np.abs(pr / pr_host - 1)[clear]))))
    assert (~clear).mean() <= 0.05
    assert np.allclose(pr[clear], pr_host[clear], rtol=1e-9)
    assert np.array_equal(got["states"].T[clear], st_host[clear])


def test_driver_ancestral_all_prints_the_table_of_ancestral(tmp_path):
    ctl = tmp_path / "brown_hky85.ctl"
    ctl.write_text(open(os.path.join(CTL, "brown_hky85.ctl")).read().replace("../data/", os.path.join(helpers.GOLDEN, "data") + "/"))

    def table(flag):
        out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(ctl), flag], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i = next(k for k, ln in enumerate(lines) if ln.startswith("Marginal reconstruction"))
        j = next((k for k in range(i, len(lines)) if lines[k].startswith("Joint reconstruction")), len(lines))
        return [ln for ln in lines[i:j] if ln.strip()], lines[j:]
    one, _ = table("--ancestral")
    allnodes, joint = table("--ancestral-all")
    assert len(one) > 10 and one == allnodes
    assert joint and joint[0].startswith("Joint reconstruction") and len([ln for ln in joint[1:] if ln.strip()]) == len(one) - 1
