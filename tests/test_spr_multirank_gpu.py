"""paml_amd_spr_scores is for one rank: an engine whose communicator has more refuses it with PAML_AMD_EUNSUPPORTED and a message, on every
rank alike, and the ranks stay in step (an evaluation afterwards returns the one-engine lnL).  Two ranks on the one GPU through the
shared-memory stand-in for the collective library, as tests/test_multirank_gpu.py.
The other two refusals that paml_amd_spr_scores states with PAML_AMD_EUNSUPPORTED cannot be reached through the ABI, so they have no
test: tips that are not the nodes 0 .. n_tips - 1 (paml_amd_set_tree already refuses such a tree, "tip with sons" / "internal node
without sons") and more than 64 states (paml_amd_create refuses n > 64, so no engine of that size exists to call it on)."""
import json
import os
import subprocess
import sys

import pytest

import helpers
from paml_amd.engine import engine_for
from test_multirank_gpu import shim_env

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "spr_rank_worker.py")
EUNSUPPORTED = -4


def test_spr_scores_refuses_an_engine_of_two_ranks(tmp_path):
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
        assert res["msg"].startswith("spr_scores: one rank only") and "2" in res["msg"], res
        assert res["untouched"] and abs(float.fromhex(res["eval_after"]) - one) <= 1e-10 * abs(one), res
