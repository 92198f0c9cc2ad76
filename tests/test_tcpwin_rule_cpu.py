"""ASan + UBSan over the receive-window rule of verify_tcp_assemble: tests/cpp/tcpwin_asan.cpp (a stand-alone
program) includes smoltcp_amd/csrc/csum_tcpwin.h, the host / device function tcpasm_kernel calls, and walks it
on the CPU over window lengths 0 .. 20, sequence offsets -26 .. 26, payload lengths 0 .. 24, rings of
W .. W + 3 bytes at every ring position and window_start near 0, 2^31 and 2^32 - 1, each case against a
per-byte brute force of its own.  Host code only; any report aborts the binary (-fno-sanitize-recover=all).

The program prints a digest of every case's outputs: each case's seven words (in_window, win_off, len,
trim, pos0, len0, len1) hashed with FNV-1a (64 bit, little-endian bytes) and the case hashes folded in
sweep order, d = (d ^ h) * prime.  This test recomputes the digest with tests/tcp_assemble_ref.py over the
same sweep, which ties the kernel's rule to the Python reference the GPU tests expect from."""
import os
import subprocess

import numpy as np

from tests import tcp_assemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
FNV_OFFSET, FNV_PRIME, M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1
STARTS = (1, 0x7FFFFFF8, 0xFFFFFFFB)


def _sweep():
    """The program's sweep as flat int64 arrays, in its order: window_start, W, ring_len, ring_pos, s, p."""
    cols = []
    s_ax, p_ax = np.arange(-26, 27), np.arange(0, 25)
    for ws in STARTS:
        for W in range(21):
            for rl in range(W, W + 4):
                rp, s, p = np.meshgrid(np.arange(max(rl, 1)), s_ax, p_ax, indexing="ij")
                n = rp.size
                cols.append(np.stack([np.full(n, ws), np.full(n, W), np.full(n, rl), rp.ravel(), s.ravel(), p.ravel()]))
    return np.concatenate(cols, axis=1).astype(np.int64)


def _reference_digest():
    ws, W, rl, rp, s, p = _sweep()
    inw, wo, ln, trim = R.window_rule((ws + s) & 0xFFFFFFFF, p, ws, W)
    pos0, len0, len1 = R.ring_split(wo, ln, rp, rl)
    with np.errstate(over="ignore"):
        h = np.full(ws.size, FNV_OFFSET, np.uint64)
        for word in (inw, wo, ln, trim, pos0, len0, len1):
            w = word.astype(np.uint64)
            for b in range(4):
                h = (h ^ ((w >> np.uint64(8 * b)) & np.uint64(0xFF))) * np.uint64(FNV_PRIME)
    d = FNV_OFFSET
    for x in h.tolist():
        d = ((d ^ x) * FNV_PRIME) & M64
    return ws.size, d


def test_tcpwin_rule_walk_asan_and_reference_digest(tmp_path):
    out = str(tmp_path / "tcpwin_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "tcpwin_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    _, cases, digest = r.stdout.split()
    n, d = _reference_digest()
    assert int(cases) == n
    assert int(digest, 16) == d, "csum_tcpwin.h and tests/tcp_assemble_ref.py disagree on some case of the sweep"
