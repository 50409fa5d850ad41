"""Helper for tests/test_gpu_agreement.py (not collected by pytest): fits ConsensusClustering as a
W-rank torch.distributed job (gloo backend, every rank on cuda:0), then every rank calls
agreement_sums (each rank the pairs of its own share of the tiles, int64 SUM all-reduce) and rank 0
saves the sums.  Started as a child process, so the ranks are spawned by a parent that has not
touched the GPU.

    python tests/agreement_dist_worker.py <fixture> <world> <K> <out.npz>
"""
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def given_labels(n):
    """A 5-cluster partition that does not come from predict."""
    return (np.arange(n) * 7 % 5).astype(np.int64)


def _rank(rank, world, port, name, K, out):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from consensus_clustering_amd import ConsensusClustering
        from tests.conftest import load_fixture

        f = load_fixture(name)
        meta = f["meta"]
        cc = ConsensusClustering(K_range=[int(k) for k in f["K_range"]], n_iterations=meta["H"],
                                 subsampling=meta["subsampling"], random_state=meta["random_state"],
                                 plot_cdf=False, keep_matrices=False)
        cc.fit(f["X"])
        res = dict(pairs=cc.agreement_sums(K),
                   given=cc.agreement_sums(K, given_labels(f["X"].shape[0])))
        if rank == 0:
            np.savez(out, **res)
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp

    name, world, K, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    mp.spawn(_rank, args=(world, _free_port(), name, K, out), nprocs=world, join=True)


if __name__ == "__main__":
    main()
