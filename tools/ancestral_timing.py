"""Ancestral reconstruction at every internal node: the all-nodes marginal call (paml_amd_ancestral_marginal) next to a loop of
paml_amd_node_posterior over the same nodes, and the device joint call (paml_amd_ancestral_joint), in the same run, at
    40 taxa x 10^5 patterns, 4 / 20 / 61 states;
    16 taxa x 10^6 codon patterns.
One warm call of each is discarded, then wall time around one call of each (the loop: all its calls) and the kernels of the new calls by
HIP events (paml_amd_ancestral_info).  The all-nodes call is timed with every posterior returned (what the loop's calls copy back) and,
beside it, with best state and probability only.  One line per row.
The host joint reconstruction (pamlh_joint_reconstruction) takes an analysis read from a control file: it is timed against the device
joint (pamlh_ancestral_joint) on the same analysis in the same run, at 4 / 20 / 61 states on the committed golden analyses (one line
each; both include the evaluation they start with).  These are small alignments: the host routine is not timed at 10^6 patterns here.
    python tools/ancestral_timing.py > profiles/ancestral_timing.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from paml_amd import engine, hostlib      # noqa: E402
import helpers                   # noqa: E402


def run(label, pb):
    eng = engine.engine_for(pb)
    t = pb.tree
    nodes = list(range(t.n_tips, t.n_nodes))
    eng.ancestral_marginal(t.branch, pb.gene_rate)
    t0 = time.perf_counter()
    eng.ancestral_marginal(t.branch, pb.gene_rate)
    t_all = time.perf_counter() - t0
    info = engine.ancestral_info()
    t0 = time.perf_counter()
    eng.ancestral_marginal(t.branch, pb.gene_rate, want_post=False)
    t_best = time.perf_counter() - t0
    eng.node_posterior(nodes[0], t.branch, pb.gene_rate)
    t0 = time.perf_counter()
    for v in nodes:
        eng.node_posterior(v, t.branch, pb.gene_rate)
    t_loop = time.perf_counter() - t0
    eng.ancestral_joint(t.branch, pb.gene_rate)
    t0 = time.perf_counter()
    eng.ancestral_joint(t.branch, pb.gene_rate)
    t_joint = time.perf_counter() - t0
    jinfo = engine.ancestral_info()
    print("%-34s %3d nodes: marginal all-nodes with posteriors %.3f s (kernels %.3f s, %d batches; best and probability only %.3f s), node_posterior loop %.3f s -> %.1fx; joint %.3f s (kernels %.3f s, %d batches)"
          % (label, len(nodes), t_all, info["last_kernel_ms"] * 1e-3, info["last_batches"], t_best, t_loop, t_loop / t_all, t_joint,
             jinfo["last_kernel_ms"] * 1e-3, jinfo["last_batches"]), flush=True)
    eng.close()


for n in (4, 20, 61):
    run("40 taxa x 10^5 patterns, %d states" % n, helpers.random_problem(n, 40, 100_000, seed=n))
run("16 taxa x 10^6 patterns, 61 states", helpers.random_problem(61, 16, 1_000_000, seed=1))


def run_joint(label, ctl, prog):
    a = hostlib.Analysis(ctl, prog)
    x = a.default_x()
    a.ancestral_joint(x)
    t0 = time.perf_counter()
    a.ancestral_joint(x)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    a.joint_reconstruction(x)
    t_host = time.perf_counter() - t0
    print("%-34s %d taxa x %d patterns, %d states: device joint %.4f s, host pamlh_joint_reconstruction %.4f s -> %.1fx"
          % (label, a.n_tips, a.n_patt, a.n, t_dev, t_host, t_host / t_dev), flush=True)


CTL = os.path.join(ROOT, "tests", "golden", "ctl")
for name, prog in (("brown_hky85.ctl", "baseml"), ("mtcdnapri_jtt.ctl", "codeml"), ("hiv_ns0.ctl", "codeml")):
    run_joint(name, os.path.join(CTL, name), prog)
