"""Who frees device memory.  Every device buffer of the library is a DevBuf (paml_amd/csrc/dev_buf.h) that frees itself with its owner,
and paml_amd_debug_device_bytes() is the sum of what they hold over the process.  Three properties, each an EXACT equality on that
counter (never on the device's free memory, which moves under other processes' work):

  per-call scratch   a whole-tree call, walked in several batches, holds after its second run what it held after its first (the first
                     lets the engine's own buffers reach their size);
  refusals           a call refused by anc_pmat — the class table names an eigen set that was never set, which is found only after the
                     packed tree is on the device — returns non-zero and leaves the counter where it was;
  engine lifetime    an engine that has evaluated, rotated its P sets, run eval_branch, a batched device decomposition and a gradient
                     gives everything back when it is destroyed.

Shapes: 6 tips, two genes of 150 patterns (300 in all: every gene ends in a ragged tile), K = 2, at 4, 20 and 61 states; the joint
reconstruction takes one class and the simulation one gene, so these two have engines of their own with that one difference."""
import ctypes as C
import gc

import numpy as np
import pytest

import helpers
import edge_ref as er
from paml_amd import engine
from paml_amd.engine import KEEP_PARTIALS, engine_for

pytestmark = pytest.mark.gpu

N_TIPS, N_PATT = 6, 300
STATES = [4, 20, 61]
TINY = "0.001"      # MiB: no call's workspace holds more than its smallest batch


def device_bytes():
    L = engine.lib()
    L.paml_amd_debug_device_bytes.restype = C.c_longlong
    L.paml_amd_debug_device_bytes.argtypes = []
    return L.paml_amd_debug_device_bytes()


def _problem(n, K=2, n_genes=2):
    return helpers.random_problem(n, N_TIPS, N_PATT, K=K, seed=40 + n, n_genes=n_genes)


def _calls(pb, eng):
    """name -> (the arena variable, the call, its info entry): every whole-tree call this engine can serve."""
    t, gr = pb.tree.branch, pb.gene_rate
    n = pb.n
    labels = np.ones((2, n, n))
    labels[1] = np.eye(n)
    rows, on, ot = er.all_rows(pb.tree, seed=7)
    queries = np.ascontiguousarray(pb.z[:2])
    calls = {
        "gradient": ("PAML_AMD_GRAD_ARENA_MB", lambda: eng.gradient(t, gr, want_lnf=True, want_scores=True), engine.gradient_info),
        "curvature": ("PAML_AMD_CURV_ARENA_MB", lambda: eng.curvature(t, gr, want_lnf=True), engine.curvature_info),
        "hessian": ("PAML_AMD_HESS_ARENA_MB", lambda: eng.hessian(t, gr, want_lnf=True), engine.hessian_info),
        "model_gradient": ("PAML_AMD_MODELGRAD_ARENA_MB", lambda: eng.model_gradient(t, gr, want_pairs=True), engine.model_gradient_info),
        "subst_counts": ("PAML_AMD_COUNTS_ARENA_MB", lambda: eng.subst_counts(t, gr, labels=labels, want_sites=True, want_lnf=True), engine.subst_counts_info),
        "ancestral_marginal": ("PAML_AMD_ANC_ARENA_MB", lambda: eng.ancestral_marginal(t, gr), engine.ancestral_info),
        "nni_scores": ("PAML_AMD_NNI_ARENA_MB", lambda: eng.nni_scores(t, gr, want_lnf=True), engine.nni_info),
        "placement_scores": ("PAML_AMD_PLACE_ARENA_MB", lambda: eng.placement_scores(t, gr, queries=queries, pendant=(0.1, 0.3), want_lnf=True), engine.placement_info),
        "spr_scores": ("PAML_AMD_SPR_ARENA_MB", lambda: eng.spr_scores(t, gr, want_lnf=True), engine.spr_info),
        "edge_scores": ("PAML_AMD_EDGE_ARENA_MB", lambda: eng.edge_scores(t, gr, rows, on, ot, want_lnf=True), engine.edge_info),
    }
    if pb.K == 1:
        calls = {"ancestral_joint": ("PAML_AMD_ANC_ARENA_MB", lambda: eng.ancestral_joint(t, gr), engine.ancestral_info)}
    if pb.n_genes == 1:
        calls = {"simulate": ("PAML_AMD_SIM_ARENA_MB", lambda: eng.simulate(t, 5000, seed=3, want_classes=True, want_ancestors=True), engine.simulate_info)}
    return calls


def _engines(n):
    """The engines of one state count, opened one at a time: the two-gene two-class one, then the one-class and the one-gene one."""
    for pb in (_problem(n), _problem(n, K=1), _problem(n, n_genes=1)):
        eng = engine_for(pb)
        try:
            yield pb, eng
        finally:
            eng.close()


# 1 ---- per-call scratch -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", STATES)
def test_a_call_in_several_batches_leaves_nothing_behind(n, monkeypatch):
    seen = []
    for pb, eng in _engines(n):
        for name, (env, call, info) in _calls(pb, eng).items():
            monkeypatch.setenv(env, TINY)
            call()
            assert info()["last_batches"] >= 2, (name, info())
            held = device_bytes()
            call()
            assert info()["last_batches"] >= 2, (name, info())
            assert device_bytes() == held, (name, device_bytes() - held)
            monkeypatch.delenv(env)
            seen.append(name)
    assert sorted(seen) == sorted(["gradient", "curvature", "hessian", "model_gradient", "subst_counts", "ancestral_marginal", "ancestral_joint",
                                   "nni_scores", "placement_scores", "spr_scores", "edge_scores", "simulate"])


def test_the_stand_alone_entries_leave_nothing_behind():
    """paml_amd_rell_replicates (in several batches) and the device compression: no engine, so everything they take is scratch."""
    rng = np.random.default_rng(5)
    lnf = -rng.gamma(4.0, 1.0, size=(3, N_PATT))
    w = rng.integers(0, 4, N_PATT).astype(np.float64)
    chars = rng.integers(0, 4, size=(N_TIPS, 2000)).astype(np.uint8)
    for _ in range(2):
        held = device_bytes()
        engine.rell_replicates(lnf, w, gene_off=[0, 150, N_PATT], n_rep=200, seed=2, arena_mb=0.001)
        assert engine.rell_info()["last_batches"] >= 2
        assert device_bytes() == held
        engine.compress_patterns(chars, gene=np.repeat([0, 1], 1000))
        assert device_bytes() == held


# 2 ---- a refusal after allocation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", STATES)
def test_a_call_refused_after_its_first_upload_leaves_nothing_behind(n):
    """set_classes takes a table whose eigen set does not exist yet (the sets may follow); eigen_refs_ok refuses it inside anc_pmat, after
    anc_tree_pack has put the packed tree on the device."""
    refused = []
    for pb in (_problem(n), _problem(n, K=1)):
        eng = engine_for(pb)
        hole = len(pb.eigen)
        eng.set_eigen(hole + 1, pb.eigen[0])      # (the table now has a slot `hole` that was never set)
        eng.set_classes(pb.mode, pb.freqK, pb.rate, np.full_like(np.asarray(pb.eigen_of, dtype=np.int32), hole), pb.qfactor)
        for name, (_, call, _) in _calls(pb, eng).items():
            held = device_bytes()
            with pytest.raises(engine.EngineError, match="eigen set %d was never set" % hole):
                call()
            assert device_bytes() == held, (name, device_bytes() - held)
            refused.append(name)
        eng.close()
    assert len(refused) == 11 and "ancestral_joint" in refused


# 3 ---- engine lifetime --------------------------------------------------------------------------------------------------------------------

def _reversible(n, m, seed):
    rng = np.random.default_rng(seed)
    Qs, pis = [], []
    for _ in range(m):
        pi = rng.dirichlet(np.ones(n) * 3)
        S = np.tril(rng.uniform(0.05, 2.0, size=(n, n)), -1)
        Q = (S + S.T) * pi[None, :]
        Q[np.diag_indices(n)] = -Q.sum(axis=1)
        Qs.append(Q); pis.append(pi)
    return np.array(Qs), np.array(pis)


@pytest.mark.parametrize("n,flags", [(61, KEEP_PARTIALS), (4, 0)])
def test_a_destroyed_engine_has_given_everything_back(n, flags):
    import torch
    pb = _problem(n)
    t, gr = pb.tree.branch, pb.gene_rate
    out = torch.zeros(3, dtype=torch.float64, device="cuda")      # (torch's memory: not the library's, not counted)
    gc.collect()      # (no engine of an earlier test waits for the collector)
    first = device_bytes()
    for _ in range(2):
        eng = engine_for(pb, flags=flags)
        eng.eval(t, gr)
        for i in range(3):      # a run: the P sets rotate
            eng.eval_device(t * (1 + 0.01 * i), out.data_ptr() + 8 * i, gr)
        eng.flush()
        node = pb.tree.sons[pb.tree.root][0]
        eng.eval_branch(node, [0.1, 0.2], t, gr)
        Qs, pis = _reversible(n, 3, seed=n)
        eng.set_eigen_qrev_batch(len(pb.eigen) + np.arange(3), Qs, pis)
        eng.eigen_status()
        eng.gradient(t, gr)
        assert device_bytes() > first
        eng.close()
        assert device_bytes() == first, device_bytes() - first
