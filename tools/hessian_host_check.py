"""Drives tools/hessian_host_check.cpp (the plan of hessian_plan.h and the per-lane bodies of kernels_hessian.h compiled for the host, for
the host sanitizers): writes 4 / 5 / 20-state cases — reversible ones with ambiguity codes, scaling nodes and a polytomy, eigen systems
with their own pi per branch label, a root that is a tip, the three-tip star, the caterpillar, zero weights, a sub-list of nodes, groups
of a few rows — with the oracle's matrices and the restatement's dP and d2P, runs the program, and compares what it wrote with the numpy
restatement (tests/hessian_ref.py): grad and hess at rtol 1e-9 / atol 1e-8, lnf at 1e-9.
    python tools/hessian_host_check.py PATH_TO_PROGRAM
    python tools/hessian_host_check.py --build      (compiles the program with ASan + UBSan into a temporary directory first)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import helpers            # noqa: E402
import ancestral_ref as ar      # noqa: E402
import curvature_ref as cr      # noqa: E402
import gradient_ref as gr       # noqa: E402
import hessian_ref as hr        # noqa: E402
from test_ancestral_gpu import _rooted_at_tip0      # noqa: E402
from test_engine_gpu import _branch_model_problem   # noqa: E402

SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHESS_HOST_ONLY"]


def cases():
    """(name, problem, nodes or None, cap)"""
    for n, K, amb, every, extra in [(4, 1, False, None, {}), (4, 3, True, 3, {}), (5, 2, False, None, {}), (20, 2, True, None, {}),
                                    (20, 1, False, 2, dict(polytomy=True))]:
        yield ("random n=%d K=%d amb=%s scale=%s %s" % (n, K, amb, every, extra),
               helpers.random_problem(n, 9, 70, K=K, seed=51 + n, ambiguity=amb, scale_every=every, **extra), None, 0)
    yield "labels with their own pi, n=4 K=2", _branch_model_problem(4, 2, 306), None, 0
    yield "rooted at tip 0, n=4 K=2", _rooted_at_tip0(helpers.random_problem(4, 9, 70, K=2, seed=55)), None, 0
    pb = helpers.random_problem(5, 9, 70, K=2, seed=8, scale_every=3)
    pb.weights[::3] = 0
    yield "a third of the weights 0, n=5 K=2, scaling, groups of 7 rows", pb, None, 7
    yield "star of three tips, n=4 K=2", hr.star_problem(4, 70, seed=3, K=2), None, 0
    yield "two tips, n=5", hr.two_tip_problem(5, 40, seed=4), None, 0
    yield "caterpillar of 7 tips, n=4 K=2, groups of 6 rows", hr.caterpillar_problem(4, 7, 70, seed=5, K=2), None, 6
    yield "a sub-list in another order, n=4 K=3, scaling", helpers.random_problem(4, 9, 70, K=3, seed=55, ambiguity=True, scale_every=3), [12, 3, 14, 0, 10, 7], 0


def write_case(f, pb, P, dP, d2P, tips, nodes, cap):
    t = pb.tree
    ptr, flat = t.csr()
    mask = np.array([sum(1 << s for s in st) for st in tips[1]], dtype=np.uint64)
    scale = np.zeros(t.n_nodes, dtype=np.int32) if pb.scale_node is None else pb.scale_node.astype(np.int32)
    nl = [] if nodes is None else nodes
    f.write(np.array([pb.n, pb.K, t.n_nodes, t.n_tips, t.root, pb.n_patt, pb.n_codes, int(scale.any()), len(flat), len(nl), cap], dtype=np.int32).tobytes())
    for a, dt in ((ptr, np.int32), (flat, np.int32), (scale, np.int32), (nl, np.int32), (pb.z, np.uint8), (mask, np.uint64), (P[0], np.float64), (dP[0], np.float64),
                  (d2P[0], np.float64), (pb.pi[0], np.float64), (pb.freqK, np.float64), (pb.weights, np.float64)):
        f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def run(prog):
    worst = dict(grad=0.0, hess=0.0, lnf=0.0)
    for name, pb, nodes, cap in cases():
        assert pb.n_genes == 1
        t = pb.tree
        P, dP, d2P, tips = ar.matrices_from_oracle(pb), gr.dmatrices(pb), cr.d2matrices(pb), ar.tips_of(pb)
        with tempfile.TemporaryDirectory() as d:
            fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
            with open(fin, "wb") as f:
                write_case(f, pb, P, dP, d2P, tips, nodes, cap)
            subprocess.run([prog, "run", fin, fout], check=True)
            raw = np.fromfile(fout, dtype=np.float64)
        nn, npt = t.n_nodes, pb.n_patt
        dim = nn if nodes is None else len(nodes)
        lnf, grad, lnL = raw[:npt], raw[npt:npt + nn], raw[npt + 2 * nn]
        hess = raw[npt + 2 * nn + 1:].reshape(dim, dim)
        ref = hr.hessian(P, dP, d2P, pb.pi, pb.freqK, tips, t, pb.weights)
        want = ref["hess"] if nodes is None else ref["hess"][np.ix_(nodes, nodes)]
        live = pb.weights > 0
        e = dict(grad=float(np.max(np.abs(grad - ref["grad"]))), hess=float(np.max(np.abs(hess - want))), lnf=float(np.max(np.abs(lnf - ref["lnf"])[live])))
        assert np.allclose(grad, ref["grad"], rtol=1e-9, atol=1e-8) and np.allclose(hess, want, rtol=1e-9, atol=1e-8), (name, e)
        assert e["lnf"] <= 1e-9 and abs(lnL - ref["lnL"]) <= 1e-10 * abs(ref["lnL"]), (name, e)
        assert hess.tobytes() == hess.T.tobytes() and np.abs(want).max() > 0
        if nodes is None:
            assert not hess[t.root].any() and not hess[:, t.root].any()
        for key in worst:
            worst[key] = max(worst[key], e[key])
        print("case %s: ok %s" % (name, e), flush=True)
    print("all cases reproduce the restatement; worst absolute errors:", worst)


if __name__ == "__main__":
    if sys.argv[1:] == ["--build"]:
        with tempfile.TemporaryDirectory() as d:
            prog = os.path.join(d, "hessian_host_check")
            subprocess.run([os.environ.get("CXX", "g++")] + SANITIZE + [os.path.join(ROOT, "tools", "hessian_host_check.cpp"), "-o", prog], check=True)
            run(prog)
    else:
        run(sys.argv[1])
