"""GPU: OffloadRing::emit_fields (host ring -> HBM -> smol_csum_batch_emit_fields -> 16 B per frame back
-> the host patches the ring) through the two C++ tools that use it."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def tools():
    assert _has_gpu()
    subprocess.run(["make", "-s", "-C", TOOLS, "loopback_ring", "ring_fields"], check=True)
    return TOOLS


def test_loopback_ring_fields_tx_path(tools):
    """tools/loopback_ring with the TX pass on emit_fields: every frame the host patched passes the GPU
    verify and the host scalar gates, and the sampled ring frames (every 97th) equal the oracle's emit
    of the frames as built, byte for byte, with the status verify reports for them."""
    with tempfile.TemporaryDirectory() as td:
        pre = os.path.join(td, "c1f")
        r = subprocess.run([os.path.join(tools, "loopback_ring"), "70001", "1", pre, "fields"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["tx_path"] == "emit_fields"
        assert out["gpu_offload"]["accepted"] == 70001
        assert out["gpu_offload"]["host_gate_sample_accepted"] == out["gpu_offload"]["host_gate_sample"]
        assert out["cpu_inline_1thread"]["accepted"] == 70001
        before = np.fromfile(pre + ".before", np.uint8)
        after = np.fromfile(pre + ".after", np.uint8)
        status = np.fromfile(pre + ".status", np.uint8)
    frame = out["frame_bytes"]
    m = (70001 + 96) // 97
    assert before.size == after.size == m * frame and status.size == m
    ref = before.copy()
    oracle.batch_emit(ref, None, m, frame, frame, 2)
    assert np.array_equal(ref, after), np.nonzero(ref != after)[0][:8]
    assert np.array_equal(oracle.batch_verify(after.copy(), None, m, frame, frame, 2), status)


def test_loopback_ring_rejects_an_unknown_tx_path(tools):
    r = subprocess.run([os.path.join(tools, "loopback_ring"), "64", "1", "unused", "feilds"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "fields" in r.stderr


def test_ring_fields_equals_in_place_ring(tools):
    """tools/ring_fields: 7003 frames, every third a raw socket's, through emit on one ring and
    emit_fields on another; the rings must be byte-identical."""
    r = subprocess.run([os.path.join(tools, "ring_fields")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fields ring equals in-place ring" in r.stdout
