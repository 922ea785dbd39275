"""One rank of tests/test_gather_walk_gpu.py: subtree_rank_worker.py's evaluations, and what Engine.gather_walk() says after them — whether the
rank's last evaluation (an eval_device call inside the communicator) ran on gather_walk_kernel, and its tiles.
usage: gather_rank_worker.py <rank> <world> <exchange dir> subtree16"""
import rank_worker      # (imports torch before the engine library, puts the repository on the path)
import subtree_rank_worker


def run(pb, eng, n_dev=4):
    out = subtree_rank_worker.run(pb, eng, n_dev)
    out["gather_walk"] = eng.gather_walk()
    return out


if __name__ == "__main__":
    rank_worker.problem, rank_worker.run = subtree_rank_worker.problem, run
    rank_worker.main()
