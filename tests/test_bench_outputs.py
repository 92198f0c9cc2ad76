"""bench.py's plain run and `--dump-outputs`: a plain run prints the headline line only (what moved
behind `--full` is absent from it), and `--dump-outputs DIR` writes the last timed step's outputs (a
fixed sample of the emitted TX records, verify's status bytes) as float .npy files that are the same
from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)

FULL_ONLY = ("roofline", "kernels_ms", "kernels_launched", "kernels_roofline", "emit_same_batch", "cpu_baseline",
             "parity_sample", "stream_read_probe", "unfused_tx", "verify_rejected")


def test_options_default_off():
    import bench

    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_steps_below_one_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.parametrize("n,max_len", [(1 << 20, 1500), (1 << 27, 1500), (1 << 20, 9000), (100, 1500), (1, 64),
                                       (5333, 1500), (5334, 1500)])
def test_dump_sample(n, max_len):
    """The sampled records: ascending, distinct, in range, within the byte budget, the same on every
    call; the head and the tail of the batch are in it."""
    import bench

    s = bench.dump_sample(n, max_len)
    assert s.dtype == np.int64 and s.size >= 1
    assert np.all(np.diff(s) > 0) and s[0] == 0 and s[-1] == n - 1
    assert s.size * max_len <= bench.DUMP_TX_BYTES or s.size == 1
    assert np.array_equal(s, bench.dump_sample(n, max_len))
    if n * max_len <= bench.DUMP_TX_BYTES:
        assert np.array_equal(s, np.arange(n))
    else:
        q = (bench.DUMP_TX_BYTES // max_len) // 4
        assert np.array_equal(s[:q], np.arange(q)) and np.array_equal(s[-q:], np.arange(n - q, n))
        assert s.size > 2 * q  # and the draw over the whole batch between them


def _fake_workload(desc):
    """A CPU stand-in for bench.Workload: 2 TX batches of 50 records whose bytes are known."""
    import torch

    from smoltcp_amd import engine as E

    rng = np.random.default_rng(3)
    n = 50
    if desc:
        lens = rng.integers(20, 90, n).astype(np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 3)  # gaps between the records
        batch = E.Batch.from_records(offs, lens, E.KIND_IP, "cpu")
        total = int(offs[-1] + lens[-1]) + 5
    else:
        offs, lens = np.arange(n, dtype=np.uint64) * 72, np.full(n, 60, dtype=np.uint32)
        batch = E.Batch.fixed(n, 72, 60, E.KIND_IP)
        total = n * 72
    txs = [torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)) for _ in range(2)]
    status = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8))
    return E, types.SimpleNamespace(n=n, batch=batch, txs=txs, status=status), offs, lens


@pytest.mark.parametrize("desc", [False, True])
def test_dump_outputs_files(tmp_path, desc):
    """The files hold the chosen TX batch's record bytes (not the gaps, not the other batch) and the
    status bytes, as float32 / float64; the summary names them."""
    import bench

    E, wl, offs, lens = _fake_workload(desc)
    out = bench.dump_outputs(str(tmp_path / "o"), E, wl, 1, 0, 1)
    rec = np.load(tmp_path / "o" / "tx_records.npy")
    txb = np.load(tmp_path / "o" / "tx_bytes.npy")
    st = np.load(tmp_path / "o" / "status.npy")
    assert rec.dtype == np.float64 and txb.dtype == np.float32 and st.dtype == np.float32
    assert np.array_equal(rec, np.arange(wl.n))  # 50 small records: all of them
    tx = wl.txs[1].numpy()
    want = np.concatenate([tx[int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)])
    assert np.array_equal(txb, want.astype(np.float32))
    assert np.array_equal(st, wl.status.numpy().astype(np.float32))
    assert out["tx_batch"] == 1 and out["status_every"] == 1
    assert sorted(out["files"]) == ["status.npy", "tx_bytes.npy", "tx_records.npy"]
    assert out["bytes"] == rec.nbytes + txb.nbytes + st.nbytes


def test_dump_outputs_per_rank_names(tmp_path):
    import bench

    E, wl, _, _ = _fake_workload(False)
    out = bench.dump_outputs(str(tmp_path), E, wl, 0, 3, 8)
    assert sorted(out["files"]) == ["status.rank3.npy", "tx_bytes.rank3.npy", "tx_records.rank3.npy"]
    assert all(os.path.exists(os.path.join(str(tmp_path), f)) for f in out["files"])


def _plain_run(outdir, config):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", config, "--n", "70001", "--steps", "3",
                        "--warmup", "1", "--ramp-ms", "20", "--dump-outputs", str(outdir)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["c2", "c3", "c2copy"])
def test_plain_run_dumps_repeatable_outputs(tmp_path, config):
    """A plain run: the headline line without --full's figures; its dumped outputs are float arrays
    within 64 MB, equal between two runs, and they are what the oracle computes: the sampled TX
    records pass the oracle's verify, and the status bytes reject about 1 record in 64."""
    import oracle
    from smoltcp_amd import engine as E

    d = _plain_run(tmp_path / "a", config)
    d2 = _plain_run(tmp_path / "b", config)
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert d["metric"] == base["metric"] and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step state the same elapsed time
    per_step = d["config"]["checksummed_bytes_per_step_per_gpu"]
    assert abs(per_step / (d["ms_per_step"] * 1e-3) / (1 << 30) - d["value"]) <= 0.01 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    o = d["outputs"]
    assert o["bytes"] <= 64_000_000 and o["tx_batch"] == (d["ramp"]["steps"] + 1 + 3 - 1) % d["batches"]["pairs"]
    arrays = {}
    for name in o["files"]:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and a.size == o["files"][name][1]
        assert np.array_equal(a, b), name
        arrays[name] = a
    assert d2["outputs"]["files"] == o["files"]
    n = d["config"]["records_per_gpu"]
    st = arrays["status.npy"].astype(np.uint8)
    assert n == 70001 and st.size == n
    rejected = int(((st & E.ST_ACCEPT) == 0).sum())
    assert n // 64 - 16 <= rejected <= n // 64 + 1  # 1/64 single-bit flips (a few the gates cannot see)
    if config != "c3":  # fixed 1500-B records: the oracle accepts every emitted record of the sample
        tx = arrays["tx_bytes.npy"].astype(np.uint8)
        m = arrays["tx_records.npy"].size
        assert tx.size == m * 1500
        ref = oracle.batch_verify(tx, None, m, 1500, 1500, E.KIND_IP, (0, 0, 0, 0, 0))
        assert np.all(ref & E.ST_ACCEPT)
