"""One rank of a world-size-N job with every rank on GPU 0, for tests/test_subtree_tables_gpu.py: rank_worker.py (its sharding, its
communicator hand-over, its out<rank>.json) with a case of its own — 16 taxa x 40 000 codon patterns with subtree tables — and a run
that writes lnL of eval and of a run of eval_device calls (hexadecimal doubles) and what paml_amd_subtree_tables reports.
usage: subtree_rank_worker.py <rank> <world> <exchange dir> subtree16"""
import rank_worker      # (imports torch before the engine library, puts the repository on the path)


def problem(case):
    from paml_amd import synth
    if case != "subtree16":
        raise SystemExit("unknown case " + case)
    return synth.codon_m0_problem(n_tips=16, n_patt=40000), 0


def run(pb, eng, n_dev=4):
    import torch
    br = pb.tree.branch
    out = {"lnL": float(eng.eval(br, pb.gene_rate)["lnL"]).hex()}
    d = torch.zeros(n_dev, dtype=torch.float64, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for i in range(n_dev):
        eng.eval_device(br * (1.0 + 0.01 * i), d.data_ptr() + 8 * i, pb.gene_rate)
    eng.flush()
    torch.cuda.current_stream().synchronize()
    out["lnL_device"] = [float(v).hex() for v in d.cpu().numpy()]
    rep = eng.subtree_tables()
    out.update(nodes=rep["nodes"], u=rep["u"], kernel=eng.kernel_name)
    return out


if __name__ == "__main__":
    rank_worker.problem, rank_worker.run = problem, run
    rank_worker.main()
