"""bench.py's single-process command line on CPU (the emulated library through bench.py's test-only hook): a plain run is
the headline alone, and --dump-outputs writes what the last timed step computed — checked here against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, LAYER_WIDTH, WIDTH = 40, 300, 32     # 12 000 gates, ~0.9 M boolean gates: more than the dump's 2^19, so it samples


def test_plain_run_is_the_headline_and_dumps_the_last_step(emul_lib, orc, c2a, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "TORCHELASTIC_RUN_ID")}
    env["C2A_BENCH_TEST_LIB"] = emul_lib
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--layers", str(LAYERS), "--layer-width", str(LAYER_WIDTH), "--width", str(WIDTH), "--dump-outputs", str(dump)],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.split("\n") if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "gates/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["metric"].startswith("gates/sec") and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["n_gates"] == LAYERS * LAYER_WIDTH
    assert d["cold"]["ms"] > 0                              # (kept in a plain run: the timed context is the process's second)
    for moved in ("cpu_baseline", "width64", "reference_shaped", "configs", "artefacts", "prune", "aggregate_replicas", "checked"):
        assert d[moved] is None, moved

    files = {f: np.load(dump / f) for f in os.listdir(dump)}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    fg = c2a.synth.layered_dag(LAYERS, LAYER_WIDTH, seed=c2a.synth.SEED)
    exp = orc.build_circuit(fg.lh, fg.rh, fg.out, fg.op, fg.n_nodes, fg.input_nodes, fg.output_nodes, mode=1)
    eb = orc.boolify(exp, WIDTH)
    np.testing.assert_array_equal(files["counts.npy"], [fg.n, exp.wire_count, len(eb.in0), eb.wire_count])
    for prefix, want in (("arith", (exp.in0, exp.in1, exp.out, exp.op)), ("bool", (eb.in0, eb.in1, eb.out, eb.op))):
        pos = files[prefix + "_pos.npy"].astype(np.int64)
        assert len(pos) == min(len(want[0]), 1 << 19) and len(np.unique(pos)) == len(pos)
        for name, w in zip(("in0", "in1", "out", "op"), want):
            np.testing.assert_array_equal(files[f"{prefix}_{name}.npy"], w[pos].astype(np.float64), err_msg=f"{prefix}_{name}")
