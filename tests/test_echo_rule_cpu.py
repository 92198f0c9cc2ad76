"""ASan + UBSan over the reply-head rule of verify_echo_reply: tests/cpp/echo_rule_asan.cpp (a stand-alone
program) includes smoltcp_amd/csrc/csum_echo.h, the host / device functions echo_kernel calls, and walks them
on the CPU over kind IP / ETH x IPv4 / IPv6, source and destination from a table of unicast, multicast,
unspecified, limited-broadcast and directed-broadcast addresses, bcast_v4 set and unset, MACs with and without
the group bit, and data lengths 0, 1, 2, 3, 56, 1472 and the longest.  Host code only; any report aborts the
binary (-fno-sanitize-recover=all).

The program prints a digest of every case's outputs: flags, head_len and the head's bytes (head_len 0 and no
bytes unless ANSWERED) hashed with FNV-1a (64 bit) and the case hashes folded in sweep order,
d = (d ^ h) * prime.  This test recomputes the digest with tests/echo_ref.py over the same sweep, which ties
the kernel's rule to the Python reference the GPU tests expect from."""
import os
import subprocess

from smoltcp_amd import engine as E
from tests import echo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
FNV_OFFSET, FNV_PRIME, M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1

V4 = [bytes(a) for a in ((10, 1, 2, 3), (192, 168, 7, 9), (224, 0, 0, 1), (239, 255, 255, 250), (0, 0, 0, 0),
                         (255, 255, 255, 255), (10, 1, 2, 255))]
BCAST = bytes((10, 1, 2, 255))
V6 = [bytes.fromhex("fe80") + bytes(13) + b"\x01", bytes.fromhex("20010db8") + bytes(10) + b"\x12\x34",
      bytes.fromhex("ff02") + bytes(13) + b"\x01", bytes(16), bytes(15) + b"\x01"]
DLEN = (0, 1, 2, 3, 56, 1472, None)  # None: the longest the length fields hold (65507 / 65527)


def sweep():
    """The program's cases, in its order: (kind, ver, mac_dst, mac_src, ethertype, src, dst, bcast, idseq, dlen)."""
    c = 0
    for kind in (E.KIND_IP, E.KIND_ETH):
        for ver in (4, 6):
            table = V4 if ver == 4 else V6
            for s in table:
                for d in table:
                    for bc in (None, BCAST):
                        for mg in range(4):
                            for ln in DLEN:
                                md = bytes([0x02 | (mg & 1), 0x11, 0x22, 0x33, 0x44, 0x55])
                                ms = bytes([0x04 | (mg >> 1), 0xA1, 0xA2, 0xA3, 0xA4, 0xA5])
                                ids = ((c * 2654435761) & 0xFFFFFFFF).to_bytes(4, "big")
                                yield (kind, ver, md, ms, b"\x08\x00" if ver == 4 else b"\x86\xdd", s, d, bc, ids,
                                       ln if ln is not None else (65507 if ver == 4 else 65527))
                                c += 1


def _reference_digest():
    n, dg = 0, FNV_OFFSET
    for kind, ver, md, ms, et, s, d, bc, ids, ln in sweep():
        fl = R.rule(kind, ver, md, ms, s, d, bc)
        hb = R.head(kind, ver, md, ms, et, s, d, ids, ln) if fl & R.ANSWERED else b""
        h = FNV_OFFSET
        for b in bytes([fl, len(hb)]) + hb:
            h = ((h ^ b) * FNV_PRIME) & M64
        dg = ((dg ^ h) * FNV_PRIME) & M64
        n += 1
    return n, dg


def test_echo_rule_walk_asan_and_reference_digest(tmp_path):
    out = str(tmp_path / "echo_rule_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "echo_rule_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    _, cases, digest = r.stdout.split()
    n, d = _reference_digest()
    assert int(cases) == n
    assert int(digest, 16) == d, "csum_echo.h and tests/echo_ref.py disagree on some case of the sweep"


def test_the_sweep_reaches_every_outcome_of_the_rule():
    """Answered, host (broadcast, multicast destination, a group-bit MAC), and neither, over both versions."""
    seen = set()
    for kind, ver, md, ms, et, s, d, bc, ids, ln in sweep():
        seen.add((kind, ver, R.rule(kind, ver, md, ms, s, d, bc) & (R.ANSWERED | R.HOST)))
    assert seen == {(k, v, o) for k in (E.KIND_IP, E.KIND_ETH) for v in (4, 6) for o in (0, R.ANSWERED, R.HOST)}
    # the directed broadcast address is a unicast one until cfg names it
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], BCAST, None) == R.REQUEST | R.ANSWERED
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], BCAST, BCAST) == R.REQUEST | R.HOST
    assert R.rule(E.KIND_IP, 4, b"", b"", BCAST, V4[0], BCAST) == R.REQUEST
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], V4[2], None) == R.REQUEST  # multicast destination: no reply
