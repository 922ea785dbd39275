"""One engine across changes of every input.  Every real user of the ABI keeps one engine alive and changes its inputs hundreds of
times; the engine keeps state derived from them (the tree program, the resolved P(t) table, the resident partials, eval_branch's
branch cache with its eigen-basis coefficients and operand fragments, per-tree kernels keyed by strings, subtree / cherry / gather
tables keyed by generations, the pipelined eval_device path).  A case here is (engine kind) x (mutation): the engine is created once
for the sizes of problem A and loaded with it, PRIMED with the calls that leave state behind, MUTATED to B through the ABI calls of
that mutation alone, CHECKED on B call by call, mutated on along the row and at last BACK TO A and checked again (a cache whose key
happens to match again).

References are never the engine under test: oracle.evaluate / eval_branch / node_posterior at the bounds of test_engine_gpu.py, and
the `_check` helpers of the whole-tree calls' own test files with the references and bounds they have there.  One exception, where no
oracle is defined: eval_branch under a pi that is not the stationary vector of the eigen systems (rows pi_alone and pi_shape) — the
re-rooted contraction is then not a reversible model's, and which end of the branch carries pi is the implementation's choice; the
reference is a FRESH engine of the same flags loaded with B, at the bound the project uses between its two forms of the call
(test_eval_branch_eigen_basis_walk_cache_and_many_trial_lengths: l rtol 1e-12, dl 1e-9 / 1e-9, ddl 1e-9 / 1e-8).  In those two rows the
gradient's branch-local reference is left out for the same reason (test_gradient_gpu.py does so for every model that is not reversible).

Not vacuous: every step of every row asserts that the references of the two problems differ by more than 1e-6 |lnL| — a million
times the bound on lnL, so an answer from state of the problem before cannot pass.

Shapes: 9 tips x 150 patterns (150 is no multiple of 64 or 128: a ragged last tile), K = 2; the rows with branch labels take
test_engine_gpu._branch_model_problem's own 10 x 160 (160 = 128 + 32), its eigen systems replaced by reversible ones of the problem's
pi so that every reference applies.  A case collects the failures of all its calls and asserts at the end that there are none.

What the file found when it was written: paml_amd_set_pi left eval_branch's state alone, and the row pi_alone failed at eval_branch on
every engine that takes the eigen-basis form of that call (20 states with default flags, 61 states with default flags, KEEP_PARTIALS
and JIT) — the branch whose coefficients were held answered with the lnL of the frequencies before, 3.1 (20 states) and 15.6 (61
states) away from the value, 4e-4 and 1.5e-3 of |lnL|, in both directions of the row.  No other row failed."""
import copy

import numpy as np
import pytest

import helpers
import oracle
from paml_amd import models
from paml_amd.engine import JIT, KEEP_PARTIALS, Engine, EngineError, engine_for
from paml_amd.problem import EIGEN_JC69LIKE, EIGEN_K80, EIGEN_UVROOT, MODE_LFUN, set_node_scale
from test_engine_gpu import _branch_model_problem

pytestmark = pytest.mark.gpu

N_TIPS, N_PATT = 9, 150
KINDS = {"4": (4, 0), "20": (20, 0), "20keep": (20, KEEP_PARTIALS), "61": (61, 0), "61keep": (61, KEEP_PARTIALS), "61jit": (61, JIT)}
REFUSAL = "eval_dirty needs PAML_AMD_KEEP_PARTIALS and a previous full evaluation"


# ---- problems ----------------------------------------------------------------------------------------------------------------------------

def _with(pb, **kw):
    q = copy.deepcopy(pb)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _base(n, seed, **kw):
    return helpers.random_problem(n, N_TIPS, N_PATT, K=2, seed=seed, **kw)


def _system(pi, seed):
    """Another reversible rate matrix with the stationary vector pi, as a (U, V, Root) set."""
    rng = np.random.default_rng(seed)
    n = len(pi)
    S = np.triu(rng.gamma(1.0, 1.0, size=(n, n)), 1)
    S = S + S.T
    Q = S * pi[None, :]
    Q[np.diag_indices(n)] = -Q.sum(axis=1)
    Q /= -np.dot(pi, np.diag(Q))
    U, V, root = models.eigen_rev(Q, pi)
    return dict(kind=EIGEN_UVROOT, U=U, V=V, Root=root)


def _label_model(n, seed):
    """Two branch labels, a set of its own for every (class, label), a rate factor each — all sets reversible with the problem's pi."""
    pb = _branch_model_problem(n, 2, seed, n_labels=2)
    pb.eigen = [pb.eigen[0]] + [_system(pb.pi[0], seed + 100 + i) for i in range(4)]
    pb.eigen_of = np.ascontiguousarray(1 + np.arange(4, dtype=np.int32).reshape(1, 2, 2))
    return pb


def _reversed_pi(pi):
    r = np.ascontiguousarray(np.atleast_2d(pi)[:, ::-1])
    return r / r.sum(axis=1, keepdims=True)


def _two_genes(n, seed):
    return helpers.give_genes_their_own_models(_base(n, seed, n_genes=2), seed=seed + 1)


# ---- the ABI calls of one mutation ---------------------------------------------------------------------------------------------------------

def _set_tips(eng, pb):
    eng.set_tips(pb.z, pb.weights, pb.cleandata, None if pb.cleandata else pb.n_chara, None if pb.cleandata else pb.chara_map,
                 pb.gene_off if pb.n_genes > 1 else None)


def _set_tree(eng, pb):
    eng.set_tree(pb.tree, pb.scale_node)


def _set_classes(eng, pb):
    eng.set_classes(pb.mode, pb.freqK, pb.rate, pb.eigen_of, pb.qfactor)


def _set_gene_class_rates(eng, pb):
    import ctypes as C
    eng._L.paml_amd_set_gene_class_rates.argtypes = [C.c_void_p, C.c_void_p]
    r = np.ascontiguousarray(pb.rate, dtype=np.float64).reshape(pb.n_genes * pb.K) if pb.rate_per_gene else None
    eng._chk(eng._L.paml_amd_set_gene_class_rates(eng._h, None if r is None else r.ctypes.data_as(C.c_void_p)))


def _labels_then_tree(eng, pb):
    """n_labels 1 -> 2: the classes first (set_classes refuses a tree whose labels it does not cover), then the tree; 2 -> 1 the tree first."""
    if pb.n_labels > 1:
        _set_classes(eng, pb)
        _set_tree(eng, pb)
    else:
        _set_tree(eng, pb)
        _set_classes(eng, pb)


# ---- the rows: (problems A, B, ... in turn — the case ends back at A —, the ABI calls that take the engine to a problem, options per problem) --

class Row:
    def __init__(self, states, move, n_genes=1, only=None):
        self.states, self.move, self.n_genes, self.only = states, move, n_genes, only


def S(pb, reversible=True, scale_every=None):
    return dict(pb=pb, reversible=reversible, scale_every=scale_every)


def _row_pi_alone(n):
    A = _base(n, 11)
    return [S(A), S(_with(A, pi=_reversed_pi(A.pi)), reversible=False)]


def _row_pi_shape(n):
    A = _base(n, 12, n_genes=2)
    return [S(A), S(_with(A, pi=np.ascontiguousarray(np.stack([A.pi[0], _reversed_pi(A.pi)[0]]))), reversible=False)]


def _row_eigen_one_label(n):
    A = _label_model(n, 13)
    B = _with(A)
    B.eigen[int(A.eigen_of[0, 0, 1])] = _system(A.pi[0], 990)
    return [S(A), S(B)]


def _move_eigen_one_label(eng, pb):
    s = int(pb.eigen_of[0, 0, 1])
    eng.set_eigen(s, pb.eigen[s])


def _row_eigen_kind(n):
    A = _base(n, 14)
    uni = np.full((1, n), 1.0 / n)
    k80 = _with(A, pi=uni, eigen=[dict(kind=EIGEN_K80, kappa=2.5)])
    return [S(k80), S(_with(k80, eigen=[_system(uni[0], 991)])), S(_with(k80, eigen=[dict(kind=EIGEN_JC69LIKE)]))]


def _row_classes_values(n):
    A = _base(n, 15)
    rng = np.random.default_rng(150)
    return [S(A), S(_with(A, freqK=rng.dirichlet(np.full(2, 5.0)), rate=rng.gamma(2.0, 0.5, size=2)))]


def _row_classes_K(n):
    A = _base(n, 16)
    rng = np.random.default_rng(160)
    B = _with(A, freqK=rng.dirichlet(np.full(3, 5.0)), rate=rng.gamma(2.0, 0.5, size=3), eigen_of=np.zeros((1, 3, 1), dtype=np.int32), qfactor=np.ones((3, 1)))
    C = _with(A, mode=MODE_LFUN, freqK=np.ones(1), rate=np.ones(1), eigen_of=np.zeros((1, 1, 1), dtype=np.int32), qfactor=np.ones((1, 1)))
    return [S(A), S(B), S(C)]


def _row_classes_eigen_of(n):
    A = _label_model(n, 17)
    rng = np.random.default_rng(170)
    return [S(A), S(_with(A, eigen_of=np.ascontiguousarray(A.eigen_of[:, ::-1, ::-1]), qfactor=0.5 + rng.random((2, 2))))]


def _row_classes_labels(n):
    B = _label_model(n, 18)
    A = _with(B, eigen_of=np.ascontiguousarray(B.eigen_of[:, :, :1]), qfactor=np.ascontiguousarray(B.qfactor[:, :1]))
    A.tree.label = np.zeros_like(B.tree.label)
    return [S(A), S(B)]


def _row_gene_class_rates(n):
    A = _two_genes(n, 19)
    rng = np.random.default_rng(190)
    return [S(A), S(_with(A, rate=rng.gamma(2.0, 0.5, size=(2, 2)), rate_per_gene=True)), S(_with(A, rate=rng.gamma(2.0, 0.5, size=(2, 2)), rate_per_gene=True))]


def _row_tips_codes(n):
    A = _base(n, 20)
    return [S(A), S(_with(A, z=_base(n, 200).z))]


def _row_tips_weights(n):
    A = _base(n, 21)
    rng = np.random.default_rng(210)
    w = rng.integers(1, 9, size=N_PATT).astype(float)
    w[rng.random(N_PATT) < 0.2] = 0
    w[[0, N_PATT - 1]] = 0      # (the first pattern and the last of the ragged tile among them)
    return [S(A), S(_with(A, weights=w))]


def _row_tips_ambiguity(n):
    A = _base(n, 22)
    amb = _base(n, 22, ambiguity=True)      # (the table of n + 3 codes and tips that use it: at 61 states 64 codes, a full ring block)
    assert amb.n_codes == n + 3
    return [S(A), S(_with(A, z=amb.z, cleandata=0, n_chara=amb.n_chara, chara_map=amb.chara_map))]


def _row_tips_68_codes(n):
    A = _base(n, 23, ambiguity=True)
    more = _base(n, 23, ambiguity=True, n_amb=4)      # (64 -> 68 codes crosses the per-tree kernel's ring block: the engine renumbers the codes)
    assert (A.n_codes, more.n_codes) == (64, 68)
    return [S(A), S(_with(A, z=more.z, n_chara=more.n_chara, chara_map=more.chara_map))]


def _row_tree_topology(n):
    A = _base(n, 24)
    return [S(A), S(_with(A, tree=_base(n, 240).tree))]


def _row_tree_four_son_root(n):
    A = _base(n, 25)
    B = _with(A, tree=_base(n, 250, polytomy=True).tree)
    assert B.tree.n_nodes == A.tree.n_nodes - 1 and len(B.tree.sons[B.tree.root]) == 4
    return [S(A), S(B)]


def _row_tree_scaling(n):
    """Scaling nodes change no value, only the exponent range: B also has other branch lengths (an argument of every call, no state), so
    that its references differ from A's."""
    A = _base(n, 26)
    B = _with(A, scale_node=set_node_scale(A.tree, 2))
    assert B.scale_node.sum() >= 2
    B.tree.branch = A.tree.branch * np.random.default_rng(260).uniform(0.6, 1.5, A.tree.n_nodes)
    B.tree.branch[B.tree.root] = 0
    return [S(A), S(B, scale_every=2)]


def _row_tree_labels(n):
    A = _label_model(n, 27)
    B = _with(A)
    B.tree.label = (1 - A.tree.label).astype(np.int32)
    B.tree.label[5:8] = A.tree.label[5:8]
    assert not np.array_equal(A.tree.label, B.tree.label) and set(B.tree.label) == {0, 1}
    return [S(A), S(B)]


def _row_gene_rate_argument(n):
    A = _two_genes(n, 28)
    return [S(A), S(_with(A, gene_rate=np.array([1.4, 0.6])))]


def _row_reload(n):
    return [S(_base(n, 29)), S(_base(n, 290))]


ROWS = {
    "pi_alone": Row(_row_pi_alone, lambda eng, pb: eng.set_pi(pb.pi)),
    "pi_shape": Row(_row_pi_shape, lambda eng, pb: eng.set_pi(pb.pi), n_genes=2),
    "eigen_one_label": Row(_row_eigen_one_label, _move_eigen_one_label),
    "eigen_kind": Row(_row_eigen_kind, lambda eng, pb: eng.set_eigen(0, pb.eigen[0]), only=("4",)),
    "classes_values": Row(_row_classes_values, _set_classes),
    "classes_K": Row(_row_classes_K, _set_classes),
    "classes_eigen_of": Row(_row_classes_eigen_of, _set_classes),
    "classes_labels": Row(_row_classes_labels, _labels_then_tree),
    "gene_class_rates": Row(_row_gene_class_rates, _set_gene_class_rates, n_genes=2),
    "tips_codes": Row(_row_tips_codes, _set_tips),
    "tips_weights": Row(_row_tips_weights, _set_tips),
    "tips_ambiguity": Row(_row_tips_ambiguity, _set_tips),
    "tips_68_codes": Row(_row_tips_68_codes, _set_tips, only=("61", "61keep", "61jit")),
    "tree_topology": Row(_row_tree_topology, _set_tree),
    "tree_four_son_root": Row(_row_tree_four_son_root, _set_tree),
    "tree_scaling": Row(_row_tree_scaling, _set_tree),
    "tree_labels": Row(_row_tree_labels, _set_tree),
    "gene_rate_argument": Row(_row_gene_rate_argument, lambda eng, pb: None, n_genes=2),
    "reload": Row(_row_reload, lambda eng, pb: eng.load(pb)),
}
CASES = [(kind, row) for row in ROWS for kind in KINDS if ROWS[row].only is None or kind in ROWS[row].only]


# ---- what is called, and against what --------------------------------------------------------------------------------------------------------

def _branches(t):
    """(the branch primed twice, its neighbour primed last — the one whose coefficients eval_branch holds —, a tip's branch elsewhere)"""
    b0 = t.n_tips + 1
    assert b0 != t.root and t.sons[b0]
    return b0, int(t.sons[b0][0]), next(v for v in range(t.n_tips) if v not in t.sons[b0])


def _dirty(pb):
    """One tip's branch made longer, the nodes off its path to the root clean (com.oldconP), and the oracle's lnL of that tree."""
    t = pb.tree
    father = t.father()
    br = t.branch.copy()
    br[3] *= 1.7
    clean = np.ones(t.n_nodes, dtype=np.uint8)
    node = 3
    while node != -1:
        clean[node] = 0
        node = father[node]
    q = _with(pb)
    q.tree.branch = br
    return br, clean, oracle.evaluate(q)["lnL"]


def _prime_branch(eng, pb):
    """eval_branch's state as a walk leaves it: partials oriented towards b1, its coefficients and the labels' operand fragments current."""
    t, gr = pb.tree, pb.gene_rate
    b0, b1, _ = _branches(t)
    ts = np.array([t.branch[b0], 0.05])
    eng.eval_branch(b0, ts, t.branch, gr)
    eng.eval_branch(b0, ts, t.branch, gr)      # (served from the coefficients where the eigen-basis form applies)
    eng.eval_branch(b1, np.array([t.branch[b1], 0.05]), t.branch, gr)


def _prime(eng, pb, keep):
    """The calls that leave state behind.  The whole-tree calls and node_posterior build their own P(t) and start eval_branch's state
    over, an ordinary evaluation does not: eval_branch goes last, so that its state is alive when the input changes."""
    t, gr = pb.tree, pb.gene_rate
    for _ in range(3):      # (a per-tree kernel compiled on the second request is in use by the third)
        eng.eval(t.branch, gr)
    eng.node_posterior(t.root, t.branch, gr)
    eng.gradient(t.branch, gr)
    eng.nni_scores(t.branch, gr)
    eng.eval(t.branch, gr)
    if keep:
        br, clean, _ = _dirty(pb)
        eng.eval_dirty(br, clean, gr)
    _prime_branch(eng, pb)


def _eval(eng, pb):
    """test_engine_gpu.check's comparison, on the engine handed in."""
    ref = oracle.evaluate(pb, want_fhk=True)
    out = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True, want_fhk=True)
    print("eval: lnL %.12f oracle %.12f; lnf max abs error %.3e" % (out["lnL"], ref["lnL"], float(np.max(np.abs(out["lnf"] - ref["lnf"])))))
    assert np.isfinite(out["lnL"])
    assert abs(out["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"]) + 1e-9, (out["lnL"], ref["lnL"])
    assert np.max(np.abs(out["lnf"] - ref["lnf"])) < 1e-9
    m = pb.weights > 0
    fk, rk = out["fhK"][:, m], ref["fhK"][:, m]
    tol = 1e-9 * np.abs(rk) + 1e-12 * np.abs(rk).max(axis=0, keepdims=True)
    assert (np.abs(fk - rk) <= tol).all(), float(np.max(np.abs(fk - rk) / np.abs(rk).max(axis=0, keepdims=True)))


def _eval_dirty(eng, pb, may_refuse=False):
    br, clean, want = _dirty(pb)
    try:
        got = eng.eval_dirty(br, clean, pb.gene_rate)
    except EngineError as ex:
        if may_refuse and REFUSAL in str(ex):      # (the mutation dropped the resident partials: refused by name until a full evaluation)
            return
        raise
    print("eval_dirty: lnL %.12f oracle %.12f" % (got, want))
    assert abs(got - want) <= 1e-10 * abs(want) + 1e-9, (got, want)


def _eval_branch(eng, pb, fresh):
    t = pb.tree
    b0, b1, tip = _branches(t)
    for b in (b1, b0, tip):
        ts = np.array([t.branch[b], 0.02, 0.7])
        l, dl, ddl = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
        if fresh is None:
            rl, rdl, rddl = oracle.eval_branch(pb, b, ts)
            l_rtol = 1e-11
        else:
            rl, rdl, rddl = fresh.eval_branch(b, ts, t.branch, pb.gene_rate)
            l_rtol = 1e-12
        print("eval_branch %d: l rel %.3e, dl abs %.3e, ddl abs %.3e" % (b, float(np.max(np.abs(l - rl) / np.abs(rl))), float(np.max(np.abs(dl - rdl))), float(np.max(np.abs(ddl - rddl)))))
        assert np.allclose(l, rl, rtol=l_rtol, atol=0), (b, l, rl)
        assert np.allclose(dl, rdl, rtol=1e-9, atol=1e-9), (b, dl, rdl)
        assert np.allclose(ddl, rddl, rtol=1e-9, atol=1e-8), (b, ddl, rddl)


def _node_posterior(eng, pb):
    t = pb.tree
    for node in (t.root, t.n_tips + 1, t.n_nodes - 1):
        got = eng.node_posterior(node, t.branch, pb.gene_rate)
        ref = oracle.node_posterior(pb, node)
        print("node_posterior %d: max abs error %.3e" % (node, float(np.max(np.abs(got - ref)))))
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-13), (node, float(np.max(np.abs(got - ref))))


def _check_all(eng, st, kind, fresh=None):
    """Every call on the engine as it stands against the references of st's problem; the list of what failed."""
    import test_ancestral_gpu
    import test_counts_gpu
    import test_curvature_gpu
    import test_edge_gpu
    import test_gradient_gpu
    import test_hessian_gpu
    import test_modelgrad_gpu
    import test_nni_gpu
    import test_placement_gpu
    import test_simulate_gpu
    import test_spr_gpu
    pb, rev, every = st["pb"], st["reversible"], st["scale_every"]
    keep = bool(KINDS[kind][1] & KEEP_PARTIALS)
    failed = []

    def run(name, fn, *a, **kw):
        try:
            fn(*a, **kw)
        except AssertionError as ex:
            failed.append("%s: %s" % (name, str(ex).strip().split("\n")[0][:400]))

    steps = []
    # The evaluations first: they leave eval_branch's state as the problem before left it, so the call after them is the first to use
    # it; the calls after that build their own P(t) and start that state over.
    if keep and st.get("dirty_first", True):
        steps.append(("eval_dirty before a full evaluation", _eval_dirty, eng, pb, True))
    steps.append(("eval", _eval, eng, pb))
    if keep:
        steps.append(("eval_dirty", _eval_dirty, eng, pb))
    steps.append(("eval_branch", _eval_branch, eng, pb, None if rev else fresh))
    steps.append(("node_posterior", _node_posterior, eng, pb))
    steps.append(("gradient", lambda: test_gradient_gpu._check(pb, eng, branch_oracle=rev)))
    steps.append(("model_gradient", lambda: test_modelgrad_gpu._check(pb, eng)))
    steps.append(("nni_scores", lambda: test_nni_gpu._check(pb, eng, scale_every=every)))
    steps.append(("placement_scores", lambda: test_placement_gpu._check(pb, eng, scale_every=every)))
    if kind == "61":
        steps.append(("curvature", lambda: test_curvature_gpu._check(pb, eng, branch_oracle=rev)))
        steps.append(("hessian", lambda: test_hessian_gpu._check(pb, eng)))
        steps.append(("subst_counts", lambda: test_counts_gpu._check(pb, eng)))
        steps.append(("spr_scores", lambda: test_spr_gpu._check(pb, eng, scale_every=every)))
        steps.append(("edge_scores", lambda: test_edge_gpu._check(pb, eng, scale_every=every, derivatives="oracle" if rev else "restatement", one_role=True)))
    steps.append(("ancestral_marginal", lambda: test_ancestral_gpu._check_marginal(pb, eng)))
    if pb.n_genes == 1:      # (simulate_ref restates the draw of one gene)
        steps.append(("simulate", lambda: test_simulate_gpu.check_bytes(eng, pb, pb.tree.branch, 257)))
    steps.append(("eval_branch after the calls that start its state over", _eval_branch, eng, pb, None if rev else fresh))
    for name, fn, *a in steps:
        run(name, fn, *a)
    _prime_branch(eng, pb)      # (the next change of an input meets the state of a walk on this problem)
    return failed


@pytest.mark.parametrize("kind,row", CASES, ids=["%s-%s" % (r, k) for k, r in CASES])
def test_one_engine_across_a_change_of_its_inputs(kind, row):
    n, flags = KINDS[kind]
    R = ROWS[row]
    states = R.states(n)
    A = states[0]["pb"]
    assert A.n_genes == R.n_genes
    refs = [oracle.evaluate(s["pb"])["lnL"] for s in states]
    eng = Engine(n, A.tree.n_tips, A.n_patt, max_classes=3, n_genes=R.n_genes, flags=flags)
    eng.load(A)
    _prime(eng, A, bool(flags & KEEP_PARTIALS))
    failed = []
    path = list(range(1, len(states))) + [0]
    prev = 0
    for step, i in enumerate(path):
        st = states[i]
        assert abs(refs[i] - refs[prev]) > 1e-6 * abs(refs[prev]), (row, prev, i, refs[prev], refs[i])
        fresh = None
        if not st["reversible"]:
            # no oracle for eval_branch here (module docstring): a fresh engine, which must itself tell this problem from the one before
            fresh = engine_for(st["pb"], flags=flags)
            before = engine_for(states[prev]["pb"], flags=flags)
            b0 = _branches(st["pb"].tree)[0]
            ts = np.array([0.02])
            l1 = fresh.eval_branch(b0, ts, st["pb"].tree.branch, st["pb"].gene_rate)[0][0]
            l0 = before.eval_branch(b0, ts, states[prev]["pb"].tree.branch, states[prev]["pb"].gene_rate)[0][0]
            assert abs(l1 - l0) > 1e-6 * abs(l0), (l0, l1)
            before.close()
        R.move(eng, st["pb"])
        if row == "gene_rate_argument":
            st = dict(st, dirty_first=False)      # (the resident partials were formed with other gene rates: the caller may not call them clean)
        got = _check_all(eng, st, kind, fresh=fresh)
        failed += ["step %d (problem %d): %s" % (step, i, f) for f in got]
        if fresh is not None:
            fresh.close()
        prev = i
    eng.close()
    assert not failed, "\n".join(failed)


def test_queued_eval_device_calls_keep_the_inputs_they_were_queued_with():
    """61 states, 6 tips, 50 001 patterns, K = 2: n_patt K >= 100 000, so consecutive eval_device calls take the pipelined path (P(t) of
    the next evaluation beside the pruning of the one before, alternating buffers).  Four calls with different branch lengths are queued
    without a synchronisation, then set_classes (another freqK) and set_pi, then two more: each of the six values is the oracle's for the
    inputs in force when it was queued, within 1e-10 |lnL|."""
    import torch
    pb = helpers.random_problem(61, 6, 50001, K=2, seed=41)
    rng = np.random.default_rng(410)
    brs = [pb.tree.branch * rng.uniform(0.6, 1.5, pb.tree.n_nodes) for _ in range(6)]
    pb2 = _with(pb, freqK=np.array([0.8, 0.2]) if pb.freqK[0] < 0.5 else np.array([0.2, 0.8]), pi=_reversed_pi(pb.pi))
    want = []
    for i, b in enumerate(brs):
        q = _with(pb if i < 4 else pb2)
        q.tree.branch = b
        want.append(oracle.evaluate(q, want_lnf=False, nthreads=16)["lnL"])
    q = _with(pb2)
    q.tree.branch = brs[3]
    other = oracle.evaluate(q, want_lnf=False, nthreads=16)["lnL"]
    assert abs(other - want[3]) > 1e-6 * abs(want[3])      # (the two sets of inputs are told apart at equal branch lengths)
    eng = Engine(61, 6, 50001, max_classes=3, n_genes=1).load(pb)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    out = torch.zeros(6, dtype=torch.float64, device="cuda")
    for i in range(4):
        eng.eval_device(brs[i], out.data_ptr() + 8 * i, pb.gene_rate)
    eng.set_classes(pb2.mode, pb2.freqK, pb2.rate, pb2.eigen_of, pb2.qfactor)
    eng.set_pi(pb2.pi)
    for i in range(4, 6):
        eng.eval_device(brs[i], out.data_ptr() + 8 * i, pb.gene_rate)
    eng.flush()
    st.synchronize()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    eng.close()
    err = np.abs(got - np.array(want)) / np.abs(want)
    print("six queued evaluations: relative errors", err)
    assert (err <= 1e-10).all(), (got, want)
