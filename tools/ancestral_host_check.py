"""Drives tools/ancestral_host_check.cpp (the per-lane bodies of kernels_ancestral.h compiled for the host, for the host sanitizers): writes
the 9-tip x 140-pattern cases of tests/test_ancestral_gpu.py with the oracle's matrices, runs the program, and compares what it wrote with
the numpy restatement (tests/ancestral_ref.py): posteriors at rtol 1e-9 / atol 1e-13, ln_best at 1e-9, the returned states' score at 1e-9.
    python tools/ancestral_host_check.py PATH_TO_PROGRAM"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers            # noqa: E402
import ancestral_ref as ar      # noqa: E402

prog = sys.argv[1]
CASES = [(4, 1, False, None, {}), (4, 3, True, 3, {}), (5, 2, False, None, {}), (20, 2, False, None, {}), (20, 1, False, None, dict(polytomy=True)),
         (61, 1, False, 4, {}), (61, 1, True, None, {})]
worst = dict(post=0.0, ln_best=0.0, score=0.0)
for n, K, amb, every, extra in CASES:
    pb = helpers.random_problem(n, 9, 140, K=K, seed=51 + n, ambiguity=amb, scale_every=every, **extra)
    t = pb.tree
    P, tips = ar.matrices_from_oracle(pb), ar.tips_of(pb)
    ptr, flat = t.csr()
    mask = np.array([sum(1 << s for s in st) for st in tips[1]], dtype=np.uint64)
    scale = np.zeros(t.n_nodes, dtype=np.int32) if pb.scale_node is None else pb.scale_node.astype(np.int32)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(np.array([n, K, t.n_nodes, t.n_tips, t.root, pb.n_patt, pb.n_codes, int(scale.any()), len(flat)], dtype=np.int32).tobytes())
            for a, dt in ((ptr, np.int32), (flat, np.int32), (scale, np.int32), (pb.z, np.uint8), (mask, np.uint64), (P[0], np.float64),
                          (pb.pi[0], np.float64), (pb.freqK, np.float64)):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        subprocess.run([prog, fin, fout], check=True)
        raw = open(fout, "rb").read()
    ni = t.n_nodes - t.n_tips
    npost = ni * pb.n_patt * n
    post = np.frombuffer(raw, dtype=np.float64, count=npost).reshape(ni, pb.n_patt, n)
    states = np.frombuffer(raw, dtype=np.uint8, count=ni * pb.n_patt, offset=npost * 8).reshape(ni, pb.n_patt)
    ln_best = np.frombuffer(raw, dtype=np.float64, count=pb.n_patt, offset=npost * 8 + ni * pb.n_patt)
    if n in (4, 5, 20):
        ref = ar.marginal(P, pb.pi, pb.freqK, tips, t)
        assert np.allclose(post, ref, rtol=1e-9, atol=1e-13), (n, K, float(np.max(np.abs(post - ref))))
        worst["post"] = max(worst["post"], float(np.max(np.abs(post - ref))))
    P1 = P[:, :1]
    rs, rl = ar.joint(P1, pb.pi, tips, t)
    e1 = float(np.max(np.abs(ln_best - rl)))
    e2 = float(np.max(np.abs(ar.joint_score(P1, pb.pi, tips, t, states) - rl)))
    assert e1 <= 1e-9 and e2 <= 1e-9, (n, K, e1, e2)
    worst["ln_best"], worst["score"] = max(worst["ln_best"], e1), max(worst["score"], e2)
    print("case n=%d K=%d amb=%s scale=%s %s: ok (states equal to the restatement's: %s)" % (n, K, amb, every, extra, bool(np.array_equal(states, rs))), flush=True)
print("all cases reproduce the restatement; worst errors:", worst)
