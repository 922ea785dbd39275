"""paml_amd_relabel_scores is for one rank: an engine whose communicator has more refuses it with PAML_AMD_EUNSUPPORTED and a message, on
every rank alike, and the ranks stay in step (an evaluation afterwards returns the one-engine lnL).  Two ranks on the one GPU through the
shared-memory stand-in for the collective library, as tests/test_nni_multirank_gpu.py."""
import json
import os
import subprocess
import sys

import pytest

import helpers
from paml_amd.engine import engine_for
from test_multirank_gpu import shim_env

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "relabel_rank_worker.py")
EUNSUPPORTED = -4


def test_relabel_scores_refuses_an_engine_of_two_ranks(tmp_path):
    world = 2
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(tmp_path)], env=shim_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    pb = helpers.random_problem(4, 9, 2048, K=2, seed=21)
    one = float(engine_for(pb).eval(pb.tree.branch, pb.gene_rate)["lnL"])
    for r in range(world):
        res = json.load(open(tmp_path / ("out%d.json" % r)))
        assert res["rc"] == EUNSUPPORTED, res
        assert res["msg"].startswith("relabel_scores: one rank only") and "2" in res["msg"], res
        assert res["untouched"] and abs(float.fromhex(res["eval_after"]) - one) <= 1e-10 * abs(one), res
