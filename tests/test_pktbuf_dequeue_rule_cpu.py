"""ASan + UBSan over the dequeue rule of udp_dequeue_emit: tests/cpp/pktbuf_dequeue_asan.cpp (a stand-alone program)
includes smoltcp_amd/csrc/csum_pktbuf.h, the host / device functions udptx_kernel calls, and walks them on the CPU
over payload rings of 0 .. 17 bytes, metadata rings of 0 .. 5 entries, every start state, front entries of every
kind (PACKET, PADDING, invalid) and size 0 .. 18 and runs of up to 4 dequeues, each step against a plain
restatement of PacketBuffer::dequeue_with.  Host code only; any report aborts the binary
(-fno-sanitize-recover=all).

The program prints a digest of every single step (the first step of every run): the step's nine
words (res, ring_off, meta_idx, size, family, and pr, pl, mr, ml after it) hashed with FNV-1a (64 bit, little-endian
bytes) and the step hashes folded in sweep order, d = (d ^ h) * prime.  This test recomputes the digest with
tests/udp_dequeue_ref.py over the same sweep, which ties the kernel's rule to the Python model the GPU tests expect
from."""
import os
import subprocess

import numpy as np

from tests import udp_dequeue_ref as D
from tests import udp_enqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
FNV_OFFSET, FNV_PRIME, M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1
MAXP, MAXM, MAXSIZE = 17, 5, 18


def _entry(k0, z0, j):
    """The program's entry_of: (size, header) as the model's PacketBuffer holds an entry."""
    code, t = (k0 + j * (1 + z0 % 3)) % 3, (z0 + j) % 3
    size = (z0 + 7 * j) % (MAXSIZE + 1)
    if code == 0:
        return size, {"kind": D.PACKET, "family": 6 if t == 1 else 4}
    if code == 1:
        return size, None
    return size, {"kind": (0, 3, D.PACKET)[t], "family": 5}


def _reference_digest():
    """The program's single steps in its order through the model: (steps, digest)."""
    rows = []
    pb = R.PacketBuffer(0, 0)
    for P in range(MAXP + 1):
        for M in range(MAXM + 1):
            pb.P, pb.M = P, M
            rings = {}
            for mr in range(max(M, 1)):
                for z0 in range(MAXSIZE + 1):
                    for k0 in range(3):
                        ring = [None] * M
                        for j in range(M):
                            ring[(mr + j) % M] = _entry(k0, z0, j)
                        rings[mr, k0, z0] = ring
            order = [(k0, z0) for k0 in range(3) for z0 in range(MAXSIZE + 1)]  # the program's inner loops
            for pr in range(max(P, 1)):
                for pl in range(P + 1):
                    for mr in range(max(M, 1)):
                        for ml in range(M + 1):
                            for k0, z0 in order:
                                pb.pr, pb.pl, pb.mr, pb.ml, pb.meta = pr, pl, mr, ml, rings[mr, k0, z0]
                                rows.append(D.dequeue(pb, D.meta_kind) + (pb.pr, pb.pl, pb.mr, pb.ml))
    words = np.array(rows, np.uint64)
    with np.errstate(over="ignore"):
        h = np.full(len(rows), FNV_OFFSET, np.uint64)
        for col in range(9):
            for b in range(4):
                h = (h ^ ((words[:, col] >> np.uint64(8 * b)) & np.uint64(0xFF))) * np.uint64(FNV_PRIME)
    d = FNV_OFFSET
    for x in h.tolist():
        d = ((d ^ x) * FNV_PRIME) & M64
    return len(rows), d


def test_pktbuf_dequeue_rule_walk_asan_and_reference_digest(tmp_path):
    out = str(tmp_path / "pktbuf_dequeue_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "pktbuf_dequeue_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    _, steps, singles, digest = r.stdout.split()
    n, d = _reference_digest()
    assert int(singles) == n and int(steps) > n
    assert int(digest, 16) == d, "csum_pktbuf.h and tests/udp_dequeue_ref.py disagree on some step of the sweep"
