"""Two ranks over gloo, each owning some chromosomes: per-chromosome run moments {sum, span, T, min, max, 0}
(engine.DeviceRuns.moments on the GPU node; here the reference's sequential update stands in for the device kernel, as
_moments_sequential does for Pearson in test_dist_gloo.py), shard.allgather_moments, shard.merge_run_moments in genome
order: both ranks end with the same six genome-wide statistics, those of one pass over the whole genome."""
import os
import sys

import numpy as np

from test_dist_gloo import _free_port
from test_integrator_moments import VAR_FAMILY, _close, _closing, _sequential

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("var", "stddev", "cv", "max", "min", "span")


def _case():
    from wiggletools_amd.runlists import synth
    return synth(5, [9000, 300, 5000, 1200], mean_run=5, seed=12, gap_prob=0.2, nan_prob=0.02)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle as O
    from wiggletools_amd import shard
    t = _case()
    c, s, f, v = O.reduce(t.as_dict(), "mean")
    mine = np.zeros((t.n_chrom, 6))
    for k in range(t.n_chrom):
        if k % world != rank:
            continue
        m = c == k
        T, total, count, mn, mx = _sequential(s[m], f[m], v[m])
        mine[k] = [total, float(count), T, mn, mx, 0.0]
    table = shard.allgather_moments(mine)
    q.put((rank, [shard.stats_from_moments(table, kind) for kind in KINDS]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_agree_on_the_genome_wide_statistics(oracle):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(np.array(got[0]), np.array(got[1]), equal_nan=True)
    c, s, f, v = oracle.reduce(_case().as_dict(), "mean")
    T, total, count, mn, mx = _sequential(s, f, v)
    for i, kind in enumerate(KINDS):
        if kind in VAR_FAMILY:
            assert _close(got[0][i], _closing(T, total, count, kind)), kind
    assert got[0][3] == mx and got[0][4] == mn and got[0][5] == count
