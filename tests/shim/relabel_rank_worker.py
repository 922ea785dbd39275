"""One rank of a world-size-N job with every rank on GPU 0, as rank_worker.py (test infrastructure; run by
tests/test_relabel_multirank_gpu.py with PAML_AMD_RCCL_LIB pointing at librccl_shim.so), for paml_amd_relabel_scores: the call is for one
rank and an engine whose communicator has more refuses it.  usage: relabel_rank_worker.py <rank> <world> <exchange dir>
Writes the return code and the message of the relabel_scores call, and the lnL of an evaluation made after it, to out<rank>.json."""
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (before the engine library: torch ships its own copy of the HIP runtime, see tests/conftest.py)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    rank, world, xdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import helpers
    from paml_amd import distributed, engine
    pb = helpers.random_problem(4, 9, 2048, K=2, seed=21)
    idfile = os.path.join(xdir, "id")
    if rank == 0:
        uid = engine.comm_unique_id()
        with open(idfile + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            time.sleep(0.05)
            if time.time() - t0 > 120:
                raise SystemExit("rank %d: no id from rank 0" % rank)
        uid = open(idfile, "rb").read()
    lo, hi = distributed.shard_bounds(pb.n_patt, world, rank)
    eng = engine.engine_for(pb.slice_patterns(lo, hi), flags=engine.SHARD)
    eng.comm_init(rank, world, uid, pb.n_patt, lo)
    L = eng._L
    L.paml_amd_relabel_scores.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6
    rows = np.asarray([(v, 0) for v in range(pb.tree.n_nodes) if v != pb.tree.root], dtype=np.int32)
    br, out, lnl = np.ascontiguousarray(pb.tree.branch), np.zeros(len(rows)), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.paml_amd_relabel_scores(eng._h, p(br), None, None, len(rows), p(rows), p(lnl), p(out), None, None, None)
    msg = L.paml_amd_last_error(eng._h).decode()
    after = eng.eval(pb.tree.branch, pb.gene_rate)["lnL"]      # (collective: every rank refused alike, so the ranks are still in step)
    eng.close()
    with open(os.path.join(xdir, "out%d.json" % rank), "w") as f:
        json.dump(dict(rc=rc, msg=msg, eval_after=float(after).hex(), untouched=bool(not out.any() and lnl[0] == 0)), f)


if __name__ == "__main__":
    main()
