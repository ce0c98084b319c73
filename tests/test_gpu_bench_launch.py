"""bench.py's N > 1 path on a one-GPU box: the RCCL (nccl backend) branch with a one-rank group on device tensors, and a
plain `python bench.py --gpus 2` that starts its two ranks itself (gloo collectives, both ranks on device 0: a rehearsal of the code path, not a
scaling figure)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SMALL = ["--no-cpu", "--no-full", "--stream-batch", "0", "--steps", "4", "--warmup", "2", "--min-timed-s", "0.05", "--inputs", "3", "--streams", "2"]


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # ONE JSON line, rank 0's
    return json.loads(lines[0])


def test_rccl_branch_with_a_one_rank_group():
    d = _run(["--gpus", "1", "--force-dist", "--backend", "nccl"])
    c = d["config"]
    assert d["n_gpus"] == 1 and "RCCL" in c["sharding"] and c["results_on_host_verified"] is True
    assert c["undetected_errors"] == 0 and c["pipeline_instances_verified"] == c["streams"] == 2 and d["value"] > 0


def test_plain_gpus_2_starts_two_ranks():
    d = _run(["--gpus", "2", "--backend", "gloo", "--force-device", "0"])
    c = d["config"]
    assert d["n_gpus"] == 2 and "gloo" in c["sharding"] and c["results_on_host_verified"] is True
    assert c["undetected_errors"] == 0 and c["pipeline_instances_verified"] == 2 and d["scaling"] == "weak"
    assert d["cpu_baseline"] is None  # a rank-0, N = 1 figure


def test_dump_outputs_do_not_depend_on_the_timing(tmp_path):
    """--dump-outputs: the same arguments give the same inputs and the dumped step does not depend on how many repeats --min-timed-s needs,
    so a run that repeats the region and one that runs it once deliver the same transport blocks and CRC flags - and every block whose CRC
    passed is the payload that was sent."""
    import importlib

    import numpy as np
    from lte_sim import DlConfig, make_subframe
    runs = []
    for d, min_s in (("a", "0.05"), ("b", "0")):
        line = _run(["--gpus", "1", "--dump-outputs", str(tmp_path / d), "--min-timed-s", min_s])
        runs.append((np.load(tmp_path / d / "transport_blocks.npy"), np.load(tmp_path / d / "crc_ok.npy")))
        assert line["steps"] == 4 and line["config"]["undetected_errors"] == 0
        assert (line["config"]["repeats"] > 1) if d == "a" else (line["config"]["repeats"] == 1)
    (tb, ok), (tb2, ok2) = runs
    assert tb.dtype == ok.dtype == np.float32 and tb.shape == (1, 128, 75376 // 8) and ok.shape == (1, 128)
    assert np.array_equal(tb, tb2) and np.array_equal(ok, ok2)
    assert ok.sum() > 0 and set(np.unique(ok)) <= {0.0, 1.0}
    # the payload bench.py sends on rank 0 (its synthetic input: seed 1000 + rank, TTIs 0..127; every input batch carries the same one)
    ue = importlib.import_module("srslte-emane_amd.sharding").ue_for_rank(0)
    cfg = DlConfig(100, ue["cell_id"], 3, 75376, cfi=1, rnti=ue["rnti"], max_iter=6)
    rng = np.random.default_rng(1000)
    sent = np.stack([make_subframe(cfg, t, rng, snr_db=None, amp=0.1)[1] for t in range(128)])
    good = ok[0].astype(bool)
    assert np.array_equal(tb[0][good], sent[good].astype(np.float32))
