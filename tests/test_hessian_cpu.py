"""The yardstick of the Hessian tests (tests/hessian_ref.py) pinned on the CPU, before any GPU run, in four ways: against the multilinear
identity (lnL's mixed derivative is f with P_u := dP_u and P_v := dP_v through a plain down pass) on every ordered pair; between the two
routes of every unrelated pair; on the diagonal against curvature_ref; and against Richardson-extrapolated central differences of
gradient_ref's own gradient.  Then the plan of hessian_plan.h (through tools/hessian_host_check.cpp's plan mode) on random trees, and the
per-lane bodies under the host sanitizers."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import curvature_ref as cr
import gradient_ref as gr
import hessian_ref as hr
import oracle
from ancestral_ref import _father, _indicator, _postorder
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    ("4-7tips-K2-amb", lambda: helpers.random_problem(4, 7, 40, K=2, seed=11, ambiguity=True)),
    ("5-9tips-polytomy", lambda: helpers.random_problem(5, 9, 40, seed=12, polytomy=True)),
    ("20-6tips-2genes", lambda: helpers.random_problem(20, 6, 30, seed=13, n_genes=2)),
    ("star-3tips", lambda: hr.star_problem(4, 30, seed=3, K=2)),
    ("rooted-2tips", lambda: hr.two_tip_problem(5, 30, seed=4)),
    ("caterpillar-7tips", lambda: hr.caterpillar_problem(4, 7, 30, seed=5, K=2)),
    ("rooted-at-a-tip", lambda: _rooted_at_tip0(helpers.random_problem(4, 7, 30, K=2, seed=55))),
    ("pi-per-label", lambda: _branch_model_problem(4, 2, 306)),
]
_cache = {}


def _case(name):
    """(problem, P, restatement) of a shape: computed once, shared by the tests and left unchanged."""
    if name not in _cache:
        pb = dict(SHAPES)[name]()
        P = ar.matrices_from_oracle(pb)
        _cache[name] = (pb, P, hr.hessian_of(pb, P))
    return _cache[name]


def _f_plain(pb, P, tips):
    """f[h] = sum_k freqK_k sum_x pi_x L_root(x) through a plain down pass with the matrices P (any of them may be a derivative)."""
    z, sets, gene_off = tips
    t, n = pb.tree, pb.n
    post = _postorder(t)
    f = np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        pi_g = pb.pi[g if pb.pi.shape[0] > 1 else 0]
        for k in range(len(pb.freqK)):
            L = {}
            for v in post:
                L[v] = _indicator(z[v, lo:hi], sets, n) if v < t.n_tips else np.ones((hi - lo, n))
                for s in t.sons[v]:
                    L[v] = L[v] * (L[s] @ P[g, k, s].T)
            f[lo:hi] += pb.freqK[k] * (L[t.root] * pi_g[None, :]).sum(axis=1)
    return f


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_restatement_equals_the_multilinear_identity_and_its_two_routes_agree(name):
    """Every ordered pair at 1e-11 relative to max_h |f_uv| (observed when the recursion was first checked: 3e-14), both routes of an
    unrelated pair against each other at the same bound."""
    pb, P, ref = _case(name)
    t = pb.tree
    tips, dP = ar.tips_of(pb), gr.dmatrices(pb)
    is_below = hr.below(t)
    worst = worst_routes = 0.0
    assert np.allclose(_f_plain(pb, P, tips), ref["f"], rtol=1e-13, atol=0)
    for u in range(t.n_nodes):
        for v in range(u + 1, t.n_nodes):
            if u == t.root or v == t.root:
                continue
            Q = P.copy()
            Q[:, :, u] = dP[:, :, u]
            Q[:, :, v] = dP[:, :, v]
            fuv = _f_plain(pb, Q, tips)
            scale = np.abs(fuv).max()
            routes = [(u, v), (v, u)]
            if is_below[u, v]:
                routes = [(v, u)]
            elif is_below[v, u]:
                routes = [(u, v)]
            for a, b in routes:
                assert not np.isnan(ref["muv"][a, b]).any(), (a, b)
                dev = np.abs(ref["muv"][a, b] - fuv).max() / scale
                worst = max(worst, dev)
                assert dev <= 1e-11, (a, b, dev)
            if len(routes) == 2:
                dev = np.abs(ref["muv"][u, v] - ref["muv"][v, u]).max() / scale
                worst_routes = max(worst_routes, dev)
                assert dev <= 1e-11, (u, v, dev)
                assert np.isclose(ref["routes"][u, v], ref["routes"][v, u], rtol=1e-11, atol=1e-11 * np.abs(ref["hess"]).max())
            else:
                a, b = routes[0]
                assert np.isnan(ref["muv"][b, a]).all()      # (a pair on one path has one route)
    print("%s: largest deviation from the multilinear identity %.3e, between the two routes %.3e (relative to max_h |f_uv|)" % (name, worst, worst_routes))


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_restatement_is_symmetric_and_its_diagonal_is_the_curvature(name):
    pb, P, ref = _case(name)
    t = pb.tree
    cv, gd = cr.curvature_of(pb, P), gr.gradient_of(pb, P)
    assert np.allclose(np.diag(ref["hess"]), cv["curv"], rtol=1e-9, atol=1e-8)
    assert ref["hess"].tobytes() == ref["hess"].T.tobytes()
    assert not ref["hess"][t.root].any() and not ref["hess"][:, t.root].any()
    assert ref["lnL"] == gd["lnL"] and ref["grad"].tobytes() == gd["grad"].tobytes() and ref["lnf"].tobytes() == gd["lnf"].tobytes()


def _grad_at(pb, P, b, tb):
    """gradient_ref's result with branch b at length tb (P(t) of that branch from the oracle, every other matrix as it is)."""
    q = copy.copy(pb)
    q.tree = copy.copy(pb.tree)
    q.tree.branch = np.array(pb.tree.branch, dtype=np.float64)
    q.tree.branch[b] = tb
    Pq = P.copy()
    for g in range(pb.n_genes):
        for k in range(pb.K):
            Pq[g, k, b] = oracle.pmat_branch(q, g, k, b)
    return gr.gradient_of(q, Pq)


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_restatement_equals_differences_of_the_gradient(name):
    """Column j of the Hessian against the Richardson pair of central differences of gradient_ref's grad in branch[j] at h = 1e-4 and
    h / 2.  The bound is derived here, entry by entry, as test_modelgrad_cpu.py derives its bound: 10 |D(h) - D(h/2)| (the differences'
    own truncation estimate) + 1e-12 S_i / h, the rounding of a difference quotient of grad[i] = sum_h w_h s_i(h), a sum of terms of
    total magnitude S_i = sum_h w_h |s_i(h)| evaluated to ~1e-12 relative."""
    pb, P, ref = _case(name)
    t = pb.tree
    h = 1e-4
    S = np.abs(gr.gradient_of(pb, P)["scores"]) @ np.asarray(pb.weights, dtype=np.float64)
    worst = worst_ratio = 0.0
    for j in range(t.n_nodes):
        if j == t.root:
            continue
        tj = float(t.branch[j])
        assert tj >= 0.005
        D = lambda s: (_grad_at(pb, P, j, tj + s)["grad"] - _grad_at(pb, P, j, tj - s)["grad"]) / (2 * s)
        d1, d2 = D(h), D(h / 2)
        R = (4 * d2 - d1) / 3
        bound = 10 * np.abs(d1 - d2) + 1e-12 * S / h
        dev = np.abs(ref["hess"][:, j] - R)
        dev[t.root] = 0
        worst = max(worst, float(dev.max()))
        worst_ratio = max(worst_ratio, float((dev / np.maximum(bound, 1e-300)).max()))
        assert (dev <= bound).all(), (j, dev, bound)
    print("%s: largest deviation from differences of the gradient %.3e (|H| max %.3e), largest share of its bound %.3f"
          % (name, worst, float(np.abs(ref["hess"]).max()), worst_ratio))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/hessian_host_check.cpp under ASan + UBSan, built once for the module."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import hessian_host_check as hc
    prog = str(tmp_path_factory.mktemp("hess") / "hessian_host_check")
    subprocess.run([os.environ.get("CXX", "g++")] + hc.SANITIZE + [os.path.join(REPO, "tools", "hessian_host_check.cpp"), "-o", prog], check=True)
    return prog


def _random_tree(rng, n_tips, polytomies):
    """Son lists: the tips 0 .. n_tips - 1, the root n_tips, internal nodes after it."""
    free = list(range(n_tips))
    sons = {}
    nxt = n_tips + 1
    n_root = 3 if n_tips >= 3 and rng.random() < 0.7 else 2
    while len(free) > n_root:
        k = 3 if polytomies and len(free) - n_root >= 2 and rng.random() < 0.4 else 2
        kids = [free.pop(int(rng.integers(len(free)))) for _ in range(k)]
        sons[nxt] = kids
        free.append(nxt)
        nxt += 1
    sons[n_tips] = free
    return [sons.get(v, []) for v in range(nxt)]


def _plan(prog, tmp, sons, n_tips, nodes):
    ptr = np.cumsum([0] + [len(s) for s in sons]).astype(np.int32)
    flat = np.array([c for s in sons for c in s], dtype=np.int32)
    fin, fout = os.path.join(tmp, "plan_in"), os.path.join(tmp, "plan_out")
    with open(fin, "wb") as f:
        f.write(np.array([n_tips, len(sons), n_tips, len(flat), len(nodes)], dtype=np.int32).tobytes())
        f.write(ptr.tobytes() + flat.tobytes() + np.array(nodes, dtype=np.int32).tobytes())
    subprocess.run([prog, "plan", fin, fout], check=True)
    raw = np.fromfile(fout, dtype=np.int32)
    ns, nst, nf, npair = raw[:4]
    o = 4
    sources = raw[o:o + 4 * ns].reshape(ns, 4); o += 4 * ns
    steps = raw[o:o + 8 * nst].reshape(nst, 8); o += 8 * nst
    factors = raw[o:o + 2 * nf].reshape(nf, 2); o += 2 * nf
    pairs = raw[o:o + 2 * npair].reshape(npair, 2)
    return sources, steps, factors, pairs


UP, OUT, TARGET = 0, 1, 2
HEAD_SCRATCH, FAC_PATH = 2, 2


def _closures(plan):
    """{frozenset(pair): the steps its target depends on, in order, without the row} after checking that no step reads a scratch vector
    before a step of the same source writes it."""
    sources, steps, factors, pairs = plan
    out = {}
    for u, s0, ns, row0 in sources:
        wrote, dep = {}, {}      # (kind, node) -> the step that wrote it; step -> the steps it needs
        for i in range(s0, s0 + ns):
            op, node, hk, hn, f0, nf, flag, row = steps[i]
            reads = [("A", hn)] if hk == HEAD_SCRATCH else []
            reads += [("L", int(nd)) for kind, nd in factors[f0:f0 + nf] if kind == FAC_PATH]
            if op == TARGET and flag:
                reads.append(("L", node))
            for r in reads:
                assert r in wrote, "source %d: step %d reads %s before it is written" % (u, i, r)
            need = []
            for r in reads:
                need += dep[wrote[r]] + [wrote[r]]
            dep[i] = sorted(set(need))
            if op == UP:
                wrote[("L", node)] = i
            elif op == OUT:
                wrote[("A", node)] = i
            else:
                assert tuple(pairs[row]) == (u, node) and row >= row0
                key = frozenset((int(u), int(node)))
                assert key not in out, "the pair %s is planned twice" % sorted(key)
                text = lambda j: (tuple(int(x) for x in steps[j][:4]), tuple(map(tuple, factors[steps[j][4]:steps[j][4] + steps[j][5]].tolist())), int(steps[j][6]))
                out[key] = (int(u), [text(j) for j in dep[i] + [i]])
    return out


@pytest.mark.parametrize("polytomies", [False, True])
def test_plan_covers_every_pair_once_in_a_valid_order_and_a_sub_list_plans_the_same_steps(host_check, tmp_path, polytomies):
    rng = np.random.default_rng(7 + polytomies)
    for n_tips in range(3, 13):
        sons = _random_tree(rng, n_tips, polytomies)
        nn = len(sons)
        every = [v for v in range(nn) if v != n_tips]
        full = _closures(_plan(host_check, str(tmp_path), sons, n_tips, every))
        assert set(full) == {frozenset((a, b)) for a in every for b in every if a < b}
        father = _father(type("T", (), dict(n_nodes=nn, sons=sons))())
        for key, (src, _) in full.items():      # the rule of the pair: the lower node of a path, else the smaller number
            a, b = sorted(key)
            anc = lambda x, y: any(z == x for z in _ancestors(father, y))
            assert src == (b if anc(a, b) else a if anc(b, a) else a)
        sub = [int(v) for v in rng.permutation(every)[:max(2, len(every) // 2)]]
        part = _closures(_plan(host_check, str(tmp_path), sons, n_tips, sub))
        assert set(part) == {frozenset((a, b)) for a in sub for b in sub if a < b}
        for key in part:
            assert part[key] == full[key], (n_tips, sorted(key))


def _ancestors(father, v):
    v = father[v]
    while v >= 0:
        yield v
        v = father[v]


def test_plan_refuses_a_bad_list(host_check, tmp_path):
    sons = [[], [], [], [0, 1, 2]]
    for nodes in ([0, 4], [0, 3], [1, 1]):
        with pytest.raises(subprocess.CalledProcessError):
            _plan(host_check, str(tmp_path), sons, 3, nodes)


def test_the_host_sanitizer_program_passes(host_check):
    """tools/hessian_host_check.cpp (the plan and the per-lane bodies with no HIP at all) under ASan + UBSan as a program of its own, on the
    cases of tools/hessian_host_check.py, against the restatement."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "hessian_host_check.py"), host_check], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "all cases reproduce the restatement" in r.stdout
