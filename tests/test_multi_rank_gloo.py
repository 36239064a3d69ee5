"""The N > 1 path of bench.py on CPU: world_size-2 gloo, the REAL shard step on the emulated library.

bench.py's default multi-GPU mode is "ONE gate graph: sort + numbering + emission replicated on every rank, boolify
sharded by sorted-position range, no data-path collective" (DESIGN.md §7).  What has to be right:
  (a) every rank, on its own, produces exactly its range of the boolean circuit — the ranks' chunks, concatenated in rank
      order, are bit-for-bit the oracle's boolify of the whole circuit;
  (b) the timed region: W untimed + exactly K timed steps, barrier on both sides, MAX over ranks;
  (c) the whole-job rate counts ONE graph in shard mode (strong scaling) and N graphs in the replicas mode.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH = 16


def _graph(c2a, seed_offset=0):
    mix = tuple(m for m in c2a.synth.MIX_ALL if m[0] != "APow")
    return c2a.synth.layered_dag(9, 14, n_in=6, n_const=2, window=3, mix=mix, seed=c2a.synth.SEED + seed_offset)


def _worker(rank, world, port, emul_lib, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    c2a = importlib.import_module("circom-2-arithc_amd")
    fg = _graph(c2a)                                         # shard mode: the SAME graph on every rank
    be = c2a.Backend(0, lib_path=emul_lib)
    be.load_gates(fg.lh, fg.rh, fg.out, fg.op, fg.n_nodes, fg.input_nodes, fg.output_nodes)
    calls = {"warm": 0, "timed": 0}
    got = {}

    def warm():
        calls["warm"] += 1
        bench.shard_step(be, WIDTH, rank, world)

    def step():
        calls["timed"] += 1
        got["info"], got["chunk"], got["range"] = bench.shard_step(be, WIDTH, rank, world, fetch=True)

    elapsed = bench.timed_region(warm, step, steps=2, warmup=1, dist=dist, torch=torch, device=None)
    q0, (in0, in1, out, op) = got["chunk"]
    lo, hi = got["range"][0], got["range"][0] + got["range"][1]
    q.put((rank, elapsed, calls["warm"], calls["timed"], lo, hi, int(q0), in0, in1, out, op, int(got["info"].n_gates),
           int(_graph(c2a, rank).lh.sum())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_shard_step_equals_the_whole_circuit(emul_lib, orc, c2a):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, emul_lib, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    fg = _graph(c2a)
    exp_c = orc.build_circuit(fg.lh, fg.rh, fg.out, fg.op, fg.n_nodes, fg.input_nodes, fg.output_nodes, mode=1)
    exp = orc.boolify(exp_c, WIDTH)
    (_, e0, w0, t0, lo0, hi0, q00, *a0, g0, s0), (_, e1, w1, t1, lo1, hi1, q01, *a1, g1, s1) = res
    assert (w0, t0, w1, t1) == (1, 2, 1, 2)                  # W untimed + exactly K timed steps on every rank
    assert abs(e0 - e1) < 1e-9                               # both ranks hold the MAX
    # the cut: two ranges of sorted positions with (nearly) equal numbers of BOOLEAN gates — the first position whose
    # boolean offset reaches half of the total (c2a_boolify_shard_range)
    T = np.array([orc.template_size(o, WIDTH)[0] for o in range(20)], dtype=np.int64)
    goff = np.concatenate([[0], np.cumsum(T[exp_c.op])])
    mid = int(np.searchsorted(goff, goff[-1] // 2, side="left"))
    assert (lo0, hi0, lo1, hi1) == (0, mid, mid, fg.n) and g0 == g1 == len(exp.in0)
    assert abs(len(a0[0]) - len(a1[0])) <= int(T[exp_c.op].max())
    assert q00 == 0 and q01 == len(a0[0])                    # rank 1 starts where rank 0 ends: no exchange needed to know it
    for k, e in enumerate((exp.in0, exp.in1, exp.out, exp.op)):
        np.testing.assert_array_equal(np.concatenate([a0[k], a1[k]]), e)
    assert s0 != s1                                          # (the replicas mode would have given the ranks different graphs)
    import bench
    assert bench.whole_job_rate(1, 1000, 3, 2.0) == 1500.0   # shard mode: one graph whatever N is
    assert bench.whole_job_rate(2, 1000, 3, 2.0) == 3000.0   # replicas mode: N graphs


def test_bench_main_runs_its_two_rank_flow_on_cpus(emul_lib, tmp_path):
    """`python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2` — the launch line of the driver's scaling run —
    executed end to end on CPUs (the emulated library + gloo through bench.py's test-only hook), with --full: both ranks sort the
    same graph, bit-blast their own range, check their results against the oracle, and rank 0 prints the one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, C2A_BENCH_TEST_LIB=emul_lib, MASTER_ADDR="127.0.0.1")
    port = 29700 + (os.getpid() % 1500)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--layers", "14", "--layer-width", "24", "--cpu-bool-chunk", "60", "--width", "8", "--full"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.split("\n") if ln.startswith("{")]
    assert len(lines) == 1                                  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong" and d["unit"] == "gates/s"
    assert d["config"]["n_gates"] == 14 * 24 and d["value"] > 0
    assert d["checked"].startswith("every one of the 2 ranks")
    assert len(d["per_rank"]) == 2 and all(r["checked"] for r in d["per_rank"])
    (lo0, n0), (lo1, n1) = d["per_rank"][0]["shard"], d["per_rank"][1]["shard"]
    assert lo0 == 0 and lo1 == n0 and n0 + n1 == 14 * 24     # two ranges that tile the sorted positions
    b = d["config"]["strong_scaling_bound"]["speedup_at_n_gpus"]
    assert 1.0 <= b["2"] <= b["8"] < 8.0
    assert d["cpu_baseline"]["kind"] == "port" and d["roofline"]["bound"] == "hbm"
    # the same launch also ran the throughput region: N independent graphs, one per rank, every rank checked its own
    ar = d["aggregate_replicas"]
    assert ar["scaling"] == "weak" and ar["graphs"] == 2 and ar["value"] > 0 and ar["checked"]
    assert all(r["replica_checked"] for r in d["per_rank"])
