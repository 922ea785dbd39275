"""Bootstrap replicates of the tree comparison: the device path (paml_amd_rell_replicates, 10 000 replicates) next to the host loop of
pamlh_tree_comparison (one core, 50 and 200 replicates -> its time per replicate) on the headline data: 16 taxa x 10^6 patterns (synth),
with 3 and 8 "trees" of per-pattern values (the lnf of the headline tree plus noise: the resampling does not care where they come from).
Also 100 sites x 10 000 replicates.  One warm call is discarded, then three timed ones: wall time around the call (upload, site list,
transpose, kernels, download) and the kernels alone by HIP events.
    python tools/rell_timing.py [n_patt] > profiles/rell_device.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, hostlib, synth      # noqa: E402

n_patt = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
N_REP = 10_000
pb = synth.codon_m0_problem(n_tips=16, n_patt=n_patt)
eng = engine.engine_for(pb)
base = eng.eval(pb.tree.branch, want_lnf=True)["lnf"]
eng.close()
w = np.asarray(pb.weights, dtype=np.float64)
ls = int(w.sum())
rng = np.random.default_rng(1)
print("data: 16 taxa x %d patterns, %d sites; kernel of the likelihoods: %s" % (n_patt, ls, "per-tree (synth.codon_m0_problem)"))
print("reference rate: cmp_hist of the compress kernels, one 1-byte gather per site through the sort permutation: 10^7 sites in 166 us = 60 G gathers/s"
      " (profiles/r01_compress_kernel_stats.csv, its longest call)")


def device(lnf, w, n_rep, label):
    engine.rell_replicates(lnf, w, n_rep=min(n_rep, 100), seed=1)      # warm: code objects, first launches
    engine.rell_replicates(lnf, w, n_rep=n_rep, seed=1)                # warm at the timed shape, discarded
    wall, kern = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        rep = engine.rell_replicates(lnf, w, n_rep=n_rep, seed=1)
        wall.append(time.perf_counter() - t0)
        kern.append(engine.rell_info()["last_kernel_ms"] * 1e-3)
    draws = float(n_rep) * w.sum()
    k = min(kern)
    print("device %-28s %6d replicates: wall %s s, kernels %s s (HIP events), batches %d -> %.1f G draws/s, %.1f G gathers/s (site list + table row)"
          % (label, n_rep, " ".join("%.3f" % v for v in wall), " ".join("%.3f" % v for v in kern), engine.rell_info()["last_batches"],
             draws / k / 1e9, 2 * draws / k / 1e9), flush=True)
    return rep, min(wall)


for n_trees in (3, 8):
    lnf = base[None, :] + rng.normal(0, 0.05, (n_trees, n_patt))
    lnf[0] = base
    rep, t_dev = device(lnf, w, N_REP, "%d trees x %d sites" % (n_trees, ls))
    per = []
    for n in (50, 200):
        t0 = time.perf_counter()
        hostlib.tree_comparison(lnf, w, n_rep=n, seed=1)
        dt = time.perf_counter() - t0
        per.append(dt / n)
        print("host   %-28s %6d replicates: %.3f s = %.4f s a replicate" % ("%d trees x %d sites" % (n_trees, ls), n, dt, dt / n), flush=True)
    print("       host scaled to %d replicates: %.1f s; device %.3f s -> %.0fx" % (N_REP, min(per) * N_REP, t_dev, min(per) * N_REP / t_dev), flush=True)
    r = hostlib.tree_comparison_from_replicates(lnf, w, rep)
    print("       table from the device replicates: pRELL %s  pSH %s" % (np.round(r["pRELL"], 4).tolist(), np.round(r["pSH"], 4).tolist()), flush=True)

lnf = rng.uniform(-8, -1, (3, 100))
device(lnf, np.ones(100), N_REP, "3 trees x 100 sites")
t0 = time.perf_counter()
hostlib.tree_comparison(lnf, np.ones(100), n_rep=N_REP, seed=1)
print("host   %-28s %6d replicates: %.3f s" % ("3 trees x 100 sites", N_REP, time.perf_counter() - t0))
