"""Drives tools/modelgrad_host_check.cpp (the per-lane bodies of kernels_modelgrad.h compiled for the host, for the host sanitizers):
writes 4 / 5 / 20-state cases — K classes, ambiguity codes, scaling nodes, a polytomy, a root that is a tip, zero weights — with the
oracle's matrices, runs the program once with the whole alignment in one batch and once in batches of 64 patterns (a segment carried
across the batch borders), and compares what it wrote with the numpy restatement (tests/modelgrad_ref.py): W, g_freqK and g_pi at 1e-9 of
the array's largest magnitude, lnL at 1e-10 |lnL|, and Psi at a repeated, a nearly repeated and a distinct pair of eigenvalues.
    python tools/modelgrad_host_check.py PATH_TO_PROGRAM [smallest]"""
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
import modelgrad_ref as mr      # noqa: E402
from test_ancestral_gpu import _rooted_at_tip0      # noqa: E402

prog = sys.argv[1]
smallest = len(sys.argv) > 2 and sys.argv[2] == "smallest"


def cases():
    yield "n=4 K=2 amb, 5 tips", mr.small_problem(4, tips=5)
    if smallest:
        return
    yield "n=4 K=3 amb scale", helpers.random_problem(4, 9, 150, K=3, seed=55, ambiguity=True, scale_every=3)
    yield "n=5 K=2", mr.small_problem(5, tips=9, ambiguity=False)
    yield "n=20 K=2 amb", mr.small_problem(20)
    yield "n=20 K=1 polytomy scale", helpers.random_problem(20, 9, 150, K=1, seed=71, scale_every=2, polytomy=True)
    yield "rooted at tip 0, n=4 K=2", _rooted_at_tip0(mr.small_problem(4, tips=9, seed=1))


def psi(lr, ls, tau):
    return tau * np.exp(lr * tau) if lr == ls else (np.exp(lr * tau) - np.exp(ls * tau)) / (lr - ls)


for name, pb in cases():
    assert pb.n_genes == 1
    t, n, K = pb.tree, pb.n, pb.K
    P, tips = ar.matrices_from_oracle(pb), ar.tips_of(pb)
    ptr, flat = t.csr()
    mask = np.array([sum(1 << s for s in st) for st in tips[1]], dtype=np.uint64)
    scale = np.zeros(t.n_nodes, dtype=np.int32) if pb.scale_node is None else pb.scale_node.astype(np.int32)
    ref = mr.pair_sums(P, pb.pi, pb.freqK, tips, t, pb.weights)
    whole = (pb.n_patt + 63) // 64 * 64
    got = {}
    for batch in (whole, 64):
        with tempfile.TemporaryDirectory() as d:
            fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
            with open(fin, "wb") as f:
                f.write(np.array([n, K, t.n_nodes, t.n_tips, t.root, pb.n_patt, pb.n_codes, int(scale.any()), len(flat)], dtype=np.int32).tobytes())
                for a, dt in ((ptr, np.int32), (flat, np.int32), (scale, np.int32), (pb.z, np.uint8), (mask, np.uint64), (P[0], np.float64),
                              (pb.pi[0], np.float64), (pb.freqK, np.float64), (pb.weights, np.float64)):
                    f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            subprocess.run([prog, fin, fout, str(batch)], check=True)
            raw = np.fromfile(fout, dtype=np.float64)
        nw = K * t.n_nodes * n * n
        W, rows, ps = raw[:nw].reshape(K, t.n_nodes, n, n), raw[nw:nw + 1 + K + n], raw[nw + 1 + K + n:]
        got[batch] = raw
        close = lambda a, b: np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b))
        assert close(W, ref["W"][0]), (name, batch, "W")
        assert abs(rows[0] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"]), (name, batch, "lnL")
        assert close(rows[1:1 + K], ref["g_freqK"]) and close(rows[1 + K:], ref["g_pi"][0]), (name, batch, "rows")
        want = np.array([psi(-1.0, -1.0, 0.3), 0.3 * np.exp(-0.3) * (1 - 0.5 * 0.3e-9), psi(-0.2, -3.0, 0.7)])
        assert np.max(np.abs(ps - want)) <= 1e-15, (ps, want)
    assert got[whole][:nw].tobytes() == got[64][:nw].tobytes(), (name, "W differs between one batch and batches of 64 patterns")
    print("case %s: ok" % name, flush=True)
print("all cases reproduce the restatement")
