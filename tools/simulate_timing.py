"""Simulation under the loaded model: the device path (paml_amd_simulate) next to the one-core numpy simulator (synth.simulate_tips) on
    16 taxa x 10^6 codon sites, K = 1 (M0);
    the same at K = 11 (the M8 table of bench.py's sweep);
    32 taxa x 10^7 nucleotide sites, GTR + Gamma-4.
One warm call at the timed shape is discarded, then three timed ones: wall time around the call (P(t), tables, walk, download of the
states) and the kernels alone by HIP events (paml_amd_simulate_info).  The host simulator draws a 10^5-site slice with the matrices of
class 0 (its work per site does not depend on the class) and is scaled to the shape: marked "scaled".
    python tools/simulate_timing.py > profiles/simulate_timing.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paml_amd import engine, models, synth      # noqa: E402

HOST_SLICE = 100_000


def run(label, pb, n_sites):
    eng = engine.engine_for(pb)
    t = pb.tree
    br = t.branch
    eng.simulate(br, n_sites, seed=1)      # warm at the timed shape, discarded
    wall, kern = [], []
    for r in range(3):
        t0 = time.perf_counter()
        eng.simulate(br, n_sites, seed=1, replicate=r)
        wall.append(time.perf_counter() - t0)
        kern.append(engine.simulate_info()["last_kernel_ms"] * 1e-3)
    k = min(kern)
    searches = t.n_nodes - 1
    print("device %-44s wall %s s, kernels %s s (HIP events), batches %d" %
          (label, " ".join("%.3f" % v for v in wall), " ".join("%.4f" % v for v in kern), engine.simulate_info()["last_batches"]))
    print("       per site: %d bytes written to the caller (n_tips), %d state bytes on the device (n_nodes), %d gathers (n_nodes - 1 searches)"
          % (t.n_tips, t.n_nodes, searches))
    print("       %.2f G sites/s, %.1f G searches/s, %.1f GB/s of state bytes in the kernels" %
          (n_sites / k / 1e9, n_sites * searches / k / 1e9, n_sites * t.n_nodes / k / 1e9), flush=True)
    P = {v: eng.get_pmat(0, 0, v) for v in range(t.n_nodes) if v != t.root}
    pi = np.asarray(pb.pi).reshape(-1)[:pb.n]
    t0 = time.perf_counter()
    synth.simulate_tips(t, pi, lambda v: P[v], HOST_SLICE, seed=1)
    dt = time.perf_counter() - t0
    print("host   synth.simulate_tips, one core, %d sites: %.3f s -> scaled to %d sites: %.1f s; device wall %.3f s -> %.0fx, kernels -> %.0fx"
          % (HOST_SLICE, dt, n_sites, dt * n_sites / HOST_SLICE, min(wall), dt * n_sites / HOST_SLICE / min(wall), dt * n_sites / HOST_SLICE / k), flush=True)
    eng.close()


base = synth.codon_m0_problem(n_tips=16, n_patt=500)
run("16 taxa x 10^6 codon sites, K = 1", base, 1_000_000)
freqs, omegas = models.nssites_classes(8, [0.9, 0.5, 1.2, 2.5], 10)
run("16 taxa x 10^6 codon sites, K = 11 (M8)", synth.codon_nssites_problem(base, 2.0, omegas, freqs), 1_000_000)
run("32 taxa x 10^7 nucleotide sites, GTR + Gamma-4", synth.nuc_gtr_gamma_problem(n_tips=32, n_patt=500), 10_000_000)
