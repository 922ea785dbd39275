"""Drives tools/counts_host_check.cpp (the per-lane bodies of kernels_counts.h compiled for the host, for the host sanitizers): writes
4 / 5 / 20-state cases — K classes, ambiguity codes, scaling nodes, a polytomy, eigen systems with their own pi per branch label, a root
that is a tip, zero weights — with the oracle's matrices and the restatement's label integrals (Van Loan), runs the program once with the
whole alignment in one batch and once in batches of 64 patterns, on every non-root node and on a permuted sub-list, and compares what it
wrote with the numpy restatement (tests/counts_ref.py): per-pattern values and totals at rtol 1e-9 / atol 1e-8, lnf at 1e-9, lnL at
1e-10 |lnL|; the two batchings give the same bytes per pattern, and the sub-list the bytes of the full list's entries.
    python tools/counts_host_check.py PATH_TO_PROGRAM
    python tools/counts_host_check.py --build      (compiles the program with ASan + UBSan into a temporary directory first)"""
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
import counts_ref as cref       # noqa: E402
from test_ancestral_gpu import _rooted_at_tip0      # noqa: E402
from test_engine_gpu import _branch_model_problem   # noqa: E402

SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCOUNTS_HOST_ONLY"]
TOL = dict(rtol=1e-9, atol=1e-8)


def cases():
    yield "n=4 K=3 amb scale", helpers.random_problem(4, 9, 150, K=3, seed=55, ambiguity=True, scale_every=3)
    yield "n=5 K=2", helpers.random_problem(5, 9, 150, K=2, seed=56)
    yield "n=20 K=2 amb", helpers.random_problem(20, 7, 70, K=2, seed=71, ambiguity=True)
    yield "n=20 K=1 polytomy scale", helpers.random_problem(20, 9, 70, K=1, seed=72, scale_every=2, polytomy=True)
    yield "labels with their own pi, n=4 K=2", _branch_model_problem(4, 2, 306)
    yield "rooted at tip 0, n=4 K=2", _rooted_at_tip0(helpers.random_problem(4, 9, 140, K=2, seed=55))
    pb = helpers.random_problem(5, 9, 150, K=2, seed=8, scale_every=3)
    pb.weights[::3] = 0
    yield "a third of the weights 0, n=5 K=2, scaling", pb


def call(prog, pb, P, I, nodes, batch):
    t, n, K = pb.tree, pb.n, pb.K
    tips = ar.tips_of(pb)
    ptr, flat = t.csr()
    mask = np.array([sum(1 << s for s in st) for st in tips[1]], dtype=np.uint64)
    scale = np.zeros(t.n_nodes, dtype=np.int32) if pb.scale_node is None else pb.scale_node.astype(np.int32)
    n_lab = I.shape[3]
    Iq = np.ascontiguousarray(I[0][:, nodes])      # [K][n_query][n_lab][n][n]
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(np.array([n, K, t.n_nodes, t.n_tips, t.root, pb.n_patt, pb.n_codes, int(scale.any()), len(flat), n_lab, len(nodes)], dtype=np.int32).tobytes())
            for a, dt in ((ptr, np.int32), (flat, np.int32), (scale, np.int32), (nodes, np.int32), (pb.z, np.uint8), (mask, np.uint64), (P[0], np.float64),
                          (Iq, np.float64), (pb.pi[0], np.float64), (pb.freqK, np.float64), (pb.weights, np.float64)):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        subprocess.run([prog, fin, fout, str(batch)], check=True)
        raw = np.fromfile(fout, dtype=np.float64)
    npt, rows = pb.n_patt, n_lab * len(nodes)
    return dict(lnf=raw[:npt], site_counts=raw[npt:npt + rows * npt].reshape(n_lab, len(nodes), npt),
                counts=raw[npt + rows * npt:npt + rows * npt + rows].reshape(n_lab, len(nodes)), lnL=raw[-1])


def run(prog):
    worst = dict(site=0.0, counts=0.0, lnf=0.0)
    for name, pb in cases():
        assert pb.n_genes == 1
        t = pb.tree
        P = ar.matrices_from_oracle(pb)
        labels = cref.mask_labels(pb.n, 7)
        I = cref.label_integrals(pb, labels)
        ref = cref.subst_counts(P, I, pb.pi, pb.freqK, ar.tips_of(pb), t, pb.weights)
        every = np.array([v for v in range(t.n_nodes) if v != t.root], dtype=np.int32)
        some = every[::-2].copy()
        whole = (pb.n_patt + 63) // 64 * 64
        full = call(prog, pb, P, I, every, whole)
        cut = call(prog, pb, P, I, every, 64)
        part = call(prog, pb, P, I, some, whole)
        live = pb.weights > 0
        e = dict(site=float(np.max(np.abs(full["site_counts"] - ref["site_counts"][:, every]))), counts=float(np.max(np.abs(full["counts"] - ref["counts"][:, every]))),
                 lnf=float(np.max(np.abs(full["lnf"] - ref["lnf"])[live])))
        assert np.allclose(full["site_counts"], ref["site_counts"][:, every], **TOL) and np.allclose(full["counts"], ref["counts"][:, every], **TOL), (name, e)
        assert np.allclose(cut["counts"], ref["counts"][:, every], **TOL), name
        assert e["lnf"] <= 1e-9 and abs(full["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"]), (name, e)
        assert not full["site_counts"][:, :, ~live].any()
        # the dwell time (the identity as a label) is the branch length at every live pattern
        assert np.allclose(full["site_counts"][2][:, live], t.branch[every][:, None], **TOL), name
        assert full["site_counts"].tobytes() == cut["site_counts"].tobytes() and full["lnf"].tobytes() == cut["lnf"].tobytes(), (name, "batches")
        pos = {int(v): i for i, v in enumerate(every)}
        assert part["site_counts"].tobytes() == np.ascontiguousarray(full["site_counts"][:, [pos[int(v)] for v in some]]).tobytes(), (name, "sub-list")
        for key in worst:
            worst[key] = max(worst[key], e[key])
        print("case %s: ok %s" % (name, e), flush=True)
    print("all cases reproduce the restatement; worst absolute errors:", worst)


if __name__ == "__main__":
    if sys.argv[1:] == ["--build"]:
        with tempfile.TemporaryDirectory() as d:
            prog = os.path.join(d, "counts_host_check")
            subprocess.run([os.environ.get("CXX", "g++")] + SANITIZE + [os.path.join(ROOT, "tools", "counts_host_check.cpp"), "-o", prog], check=True)
            run(prog)
    else:
        run(sys.argv[1])
