"""ASan + UBSan over the enqueue rule of verify_udp_enqueue: tests/cpp/pktbuf_asan.cpp (a stand-alone program)
includes smoltcp_amd/csrc/csum_pktbuf.h, the host / device function udprx_kernel calls, and walks it on the CPU
over payload rings of 0 .. 17 bytes, metadata rings of 0 .. 5 entries, every start state, sizes 0 .. 18 and
sequences of up to 4 enqueues, each step against a plain restatement of PacketBuffer::enqueue and a byte map
of the ring.  Host code only; any report aborts the binary (-fno-sanitize-recover=all).

The program prints a digest of every single step's outputs (every P, M, start state and size): the step's nine
words (res, ring_off, meta_idx, pad_idx, pad_size, and pr, pl, mr, ml after it) hashed with FNV-1a (64 bit,
little-endian bytes) and the step hashes folded in sweep order, d = (d ^ h) * prime.  This test recomputes the
digest with tests/udp_enqueue_ref.py over the same sweep, which ties the kernel's rule to the Python model the
GPU tests expect from."""
import os
import subprocess

import numpy as np

from tests import udp_enqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
FNV_OFFSET, FNV_PRIME, M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1
MAXP, MAXM, MAXSIZE = 17, 5, 18


def _reference_digest():
    """The program's single steps in its order through the model: (steps, digest)."""
    rows = []
    pb = R.PacketBuffer(0, 0)
    for P in range(MAXP + 1):
        for M in range(MAXM + 1):
            pb.P, pb.M, pb.meta = P, M, [None] * M
            for pr in range(max(P, 1)):
                for pl in range(P + 1):
                    for mr in range(max(M, 1)):
                        for ml in range(M + 1):
                            for size in range(MAXSIZE + 1):
                                pb.pr, pb.pl, pb.mr, pb.ml = pr, pl, mr, ml
                                rows.append(pb.enqueue(size) + (pb.pr, pb.pl, pb.mr, pb.ml))
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


def test_pktbuf_rule_walk_asan_and_reference_digest(tmp_path):
    out = str(tmp_path / "pktbuf_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "pktbuf_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    _, steps, singles, digest = r.stdout.split()
    n, d = _reference_digest()
    assert int(singles) == n and int(steps) > n
    assert int(digest, 16) == d, "csum_pktbuf.h and tests/udp_enqueue_ref.py disagree on some step of the sweep"
