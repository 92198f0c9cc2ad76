"""ASan + UBSan over the refusal rule of verify_unreach_reply: tests/cpp/unreach_rule_asan.cpp (a stand-alone
program) includes smoltcp_amd/csrc/csum_unreach.h, the host / device functions unreach_kernel calls, and walks
them on the CPU over kind IP / ETH x IPv4 / IPv6, source and destination from a table of unicast, multicast,
unspecified, limited-broadcast and directed-broadcast addresses, bcast_v4 set and unset, MACs with and without
the group bit, protocols / next headers 0, 1, 6, 17, 58 and 47, with and without a leading Hop-by-Hop header,
the port map's bit clear and set, and P 0, 8, 528, 1193 and the longest.  Host code only; any report aborts the
binary (-fno-sanitize-recover=all).

The program prints a digest of every case's outputs: flags, type, code, head_len and the head's bytes (type and
code 0 unless REFUSED, head_len 0 and no bytes unless ANSWERED) hashed with FNV-1a (64 bit) and the case hashes
folded in sweep order, d = (d ^ h) * prime.  This test recomputes the digest with tests/unreach_ref.py over the
same sweep, which ties the kernel's rule to the Python reference the GPU tests expect from."""
import os
import subprocess

from smoltcp_amd import engine as E
from tests import unreach_ref as R
from tests.test_echo_rule_cpu import BCAST, ENV, FNV_OFFSET, FNV_PRIME, M64, SAN, V4, V6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = (0, 1, 6, 17, 58, 47)
PLEN = (0, 8, 528, 1193, None)  # None: the longest the length fields hold (65515 / 65535)


def sweep():
    """The program's cases, in its order: (kind, ver, mac_dst, mac_src, ethertype, src, dst, bcast, proto, hbh,
    udp_closed, P, hop)."""
    c = 0
    for kind in (E.KIND_IP, E.KIND_ETH):
        for ver in (4, 6):
            table = V4 if ver == 4 else V6
            for s in table:
                for d in table:
                    for bc in (None, BCAST):
                        for mg in range(4):
                            for proto in PROTO:
                                for hbh in ((False, True) if ver == 6 else (False,)):
                                    for closed in (False, True):
                                        for ln in PLEN:
                                            md = bytes([0x02 | (mg & 1), 0x11, 0x22, 0x33, 0x44, 0x55])
                                            ms = bytes([0x04 | (mg >> 1), 0xA1, 0xA2, 0xA3, 0xA4, 0xA5])
                                            yield (kind, ver, md, ms, b"\x08\x00" if ver == 4 else b"\x86\xdd", s, d, bc, proto,
                                                   hbh, closed, ln if ln is not None else (65515 if ver == 4 else 65535),
                                                   (c * 7 + 1) & 0xFF)
                                            c += 1


def outcome(kind, ver, md, ms, et, s, d, bc, proto, hbh, closed, plen, hop):
    """(flags, type, code, head bytes) of one case by tests/unreach_ref.py."""
    port = R.form_of(ver, proto, hbh, closed)
    if port is None:
        return 0, 0, 0, b""
    fl, t, c = R.rule(kind, ver, md, ms, s, d, hbh, port, bc)
    return fl, t, c, R.head(kind, ver, md, ms, et, s, d, hop, proto, plen, t, c) if fl & R.ANSWERED else b""


def _reference_digest():
    n, dg = 0, FNV_OFFSET
    for case in sweep():
        fl, t, c, hb = outcome(*case)
        h = FNV_OFFSET
        for b in bytes([fl, t, c, len(hb)]) + hb:
            h = ((h ^ b) * FNV_PRIME) & M64
        dg = ((dg ^ h) * FNV_PRIME) & M64
        n += 1
    return n, dg


def test_unreach_rule_walk_asan_and_reference_digest(tmp_path):
    out = str(tmp_path / "unreach_rule_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "unreach_rule_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    _, cases, digest = r.stdout.split()
    n, d = _reference_digest()
    assert int(cases) == n
    assert int(digest, 16) == d, "csum_unreach.h and tests/unreach_ref.py disagree on some case of the sweep"


def test_the_sweep_reaches_every_flag_combination_the_contract_allows():
    """Not refused; refused in the protocol / next-header form and in the port form, each answered, the host's
    (a multicast IPv6 destination, a group-bit MAC, a Hop-by-Hop header) and neither; every ICMP type / code."""
    seen, tc, host_by = set(), set(), set()
    for case in sweep():
        kind, ver, md, ms, et, s, d, bc, proto, hbh, closed, plen, hop = case
        fl, t, c, hb = outcome(*case)
        seen.add(fl)
        if fl:
            tc.add((ver, bool(fl & R.PORT), t, c))
        if fl & R.HOST:
            host_by.add((kind, ver, hbh))
        assert bool(hb) == bool(fl & R.ANSWERED) and not (fl & R.ANSWERED and fl & R.HOST)
        assert not hbh or not fl & R.ANSWERED
    assert seen == {0, R.REFUSED, R.REFUSED | R.ANSWERED, R.REFUSED | R.HOST, R.REFUSED | R.PORT,
                    R.REFUSED | R.PORT | R.ANSWERED, R.REFUSED | R.PORT | R.HOST}
    assert tc == {(4, False, 3, 2), (4, True, 3, 3), (6, False, 4, 1), (6, True, 1, 4)}
    # HOST: over IPv6 at either kind, with and without the Hop-by-Hop header; over IPv4 only through a group MAC
    assert host_by == {(E.KIND_IP, 6, False), (E.KIND_IP, 6, True), (E.KIND_ETH, 6, False), (E.KIND_ETH, 6, True),
                       (E.KIND_ETH, 4, False)}
    # the IPv4 broadcast destination the echo call marks HOST is left unanswered here
    from tests import echo_ref

    assert echo_ref.rule(E.KIND_IP, 4, b"", b"", V4[0], V4[5], None) == echo_ref.REQUEST | echo_ref.HOST
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], V4[5], False, True, None)[0] == R.REFUSED | R.PORT
    # the directed broadcast address is a unicast one until cfg names it
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], BCAST, False, False, None)[0] == R.REFUSED | R.ANSWERED
    assert R.rule(E.KIND_IP, 4, b"", b"", V4[0], BCAST, False, False, BCAST)[0] == R.REFUSED
    assert R.rule(E.KIND_IP, 4, b"", b"", BCAST, V4[0], False, False, BCAST)[0] == R.REFUSED
