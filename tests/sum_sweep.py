"""The sum sweep's corpus, its plain reference and the class bookkeeping (CPU only; tests/test_sum_sweep_cpu.py
and tests/test_gpu_sum_sweep.py use it).

The edge sweep (tests/edge_sweep.py) enumerates where a record's header objects lie; this module enumerates
what a record's sums are.  A one's-complement sum has two zeros (0x0000 and 0xffff), and every kernel family
carries its own copy of the arithmetic: u32 differences before the fold, per-slice folds and byte swaps,
comparisons by equality or against 0xffff.  Each copy breaks at other values, and random payloads reach none
of them.  The corpus steers one 16-bit word of a record so that a chosen sum lands on a chosen value:

  C0, C1, CFFFE  the computed L4 checksum is 0x0000, 0x0001, 0xfffe (UDP writes 0xffff for 0x0000)
  ZERO           every summed byte is zero (ICMPv4 / IGMP only): the computed checksum is 0xffff (CFFFF)
  D0             the L4 bytes alone sum to a non-zero multiple of 0xffff
  PH0            the pseudo-header alone does;  D0PH0: both
  H0, IN0        the IPv4 header checksum, the one of an ICMPv4 error's embedded header, computes to 0x0000
  PARTIAL        the UDP / TCP field holds the pseudo-header's sum (and that +- 1, and both zeros under PH0)
  TOP            the longest records, every byte 0xff that may be: bit 31 of the aligned-word sum is set

Records are the edge sweep's `Rec`s (SRec adds what the builder meant, for messages only), so
edge_sweep.place_desc / place_fixed / verify_model / emit_model and the GPU rig take them unchanged.  The class
of a record is never taken from the builder: `classify` computes it from the bytes with the plain reference
below, which uses Python integers only (no numpy, no folds) over edge_sweep.geometry's parse.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import edge_sweep as S
from tests import pktgen as P

KIND_IP, KIND_ETH = S.KIND_IP, S.KIND_ETH
P_UDP, P_TCP, P_ICMP4, P_IGMP, P_ICMP6 = S.P_UDP, S.P_TCP, S.P_ICMP4, S.P_IGMP, S.P_ICMP6
CAP_OF = {P_UDP: 1, P_TCP: 2, P_ICMP4: 3, P_ICMP6: 4}  # a protocol's entry of the caps tuple (IGMP has none)

# ---------------------------------------------------------------------------------------------
# The plain reference
# ---------------------------------------------------------------------------------------------


def wsum(b) -> int:
    """The sum of the big-endian 16-bit words of b (a lone last byte is a high byte), as an int."""
    b = bytes(b)
    return sum(b[0::2]) * 256 + sum(b[1::2])


def rd16(b, o) -> int:
    return b[o] << 8 | b[o + 1]


class Arith:
    """One's-complement sums with Python integers.  The methods are the places where a kernel's arithmetic
    can differ; tests/test_sum_sweep_cpu.py overrides one per mutant."""

    udp_map = (P_UDP,)    # the protocols whose computed 0x0000 goes out as 0xffff
    zero_skip = (P_UDP,)  # the protocols whose field 0x0000 means "no checksum"
    nhc_map = False       # NHC UDP: no such map, and the field is compared by equality

    def rep(self, x: int) -> int:
        """The representative in 0..0xffff of x modulo 0xffff: 0 for 0 only."""
        return 0 if x == 0 else (x - 1) % 0xFFFF + 1

    def span(self, rec, a: int, b: int, start: int) -> int:
        """The sum of the record's bytes a..b, relative to a (`start`: the record's address)."""
        return wsum(rec[a:b])

    def without(self, total: int, field: int) -> int:
        """A sum taken with the field's old content in it, less that content."""
        return total - field

    def partial(self, ph: int, field: int) -> bool:
        return self.rep(ph) == field

    def csum(self, total: int) -> int:
        return 0xFFFF - self.rep(total)

    def valid(self, total: int) -> bool:
        """A sum with its checksum in it is right."""
        return self.rep(total) == 0xFFFF

    # ---- the record rules over these -------------------------------------------------------

    def pseudo(self, rec, g, n: int) -> int:
        if g.proto in (P_ICMP4, P_IGMP):
            return 0
        o = g.ip_off
        addrs = rec[o + 12:o + 20] if g.fam == 4 else rec[o + 8:o + 40]
        return wsum(addrs) + g.proto + n

    def l4(self, rec, g, start=0):
        """(pseudo-header sum, sum of the L4 span without its field, the field, its record offset)."""
        e = S.span_end(rec, g)
        fo = g.l4_off + S.L4_FIELD[g.proto]
        field = rd16(rec, fo)
        return self.pseudo(rec, g, e - g.l4_off), self.without(self.span(rec, g.l4_off, e, start), field), field, fo

    def header(self, rec, o, hl, start=0):
        """An IPv4 header's sum without its field."""
        return self.without(self.span(rec, o, o + hl, start), rd16(rec, o + 10))

    def verify(self, rec, kind, flags=0, caps=(0, 0, 0, 0, 0), start=0) -> int:
        g = S.geometry(rec, kind, flags)
        ip_valid = l4_valid = ip_gate = l4_gate = True
        partial = False
        if g.fam == 4:
            ip_valid = self.valid(self.header(rec, g.ip_off, g.ip_hl, start) + rd16(rec, g.ip_off + 10))
            ip_gate = caps[0] in (0, 1)
        if not g.malformed and g.proto:
            ph, body, field, _ = self.l4(rec, g, start)
            l4_valid = self.valid(ph + body + field) or (field == 0 and g.proto in self.zero_skip)
            partial = g.proto in (P_UDP, P_TCP) and self.partial(ph, field)
            l4_gate = g.proto != P_IGMP and caps[CAP_OF[g.proto]] in (0, 1)
        ip_ok, l4_ok = ip_valid or not ip_gate, l4_valid or not l4_gate
        st = (S.ST_IP_OK if ip_ok else 0) | (S.ST_L4_OK if l4_ok else 0) | (S.ST_L4_PARTIAL if partial else 0) \
            | (S.ST_IP_VALID if ip_valid else 0) | (S.ST_L4_VALID if l4_valid else 0) \
            | (S.ST_MALFORMED if g.malformed else 0) | (S.ST_UNSUPPORTED if g.unsupported else 0)
        return st | (S.ST_ACCEPT if ip_ok and l4_ok and not g.malformed else 0)

    def emit(self, rec, kind, flags=0, caps=(0, 0, 0, 0, 0), start=0):
        """(status, the record after emit)."""
        rec = bytearray(rec)
        g = S.geometry(rec, kind, flags, emit=True)

        def put(o, v):
            rec[o:o + 2] = v.to_bytes(2, "big")

        def put_header(o, hl):
            c = self.csum(self.header(rec, o, hl, start))
            put(o + 10, c if caps[0] in (0, 2) else 0)

        if g.fam == 4:
            put_header(g.ip_off, g.ip_hl)
        if not g.malformed and g.proto:
            emb = S.embedded_header(rec, g)
            if emb:
                put_header(*emb)
            ph, body, _, fo = self.l4(rec, g, start)
            c = self.csum(ph + body)
            if c == 0 and g.proto in self.udp_map:
                c = 0xFFFF
            put(fo, c if g.proto == P_IGMP or caps[CAP_OF[g.proto]] in (0, 2) else 0)
        return (S.ST_MALFORMED if g.malformed else 0) | (S.ST_UNSUPPORTED if g.unsupported else 0), bytes(rec)

    # ---- 6LoWPAN NHC UDP ---------------------------------------------------------------------

    def nhc_csum(self, p, addrs, emit: bool, start=0):
        """(the computed checksum, the field's offset) of a well-formed NHC UDP packet; the payload lies
        behind the two bytes of an inline checksum (emit: also where the packet's is elided)."""
        m = p[0] & 3
        ps = (4, 3, 3, 1)[m]
        if m == 0:
            sport, dport = rd16(p, 1), rd16(p, 3)
        elif m == 1:  # parse reads the destination's low byte from byte 1, emit from byte 3 (as the reference does)
            sport, dport = rd16(p, 1), 0xF000 + p[3 if emit else 1]
        elif m == 2:
            sport, dport = 0xF000 + p[1], rd16(p, 2)
        else:
            sport, dport = 0xF0B0 + (p[1] >> 4), 0xF0B0 + p[1]
        hdr = 1 + ps + (2 if emit or not p[0] & 4 else 0)
        n = len(p) - hdr + 8
        c = self.csum(wsum(addrs) + 17 + n + sport + dport + n + self.span(p, hdr, len(p), start))
        return (0xFFFF if c == 0 and self.nhc_map else c), 1 + ps, dport

    def nhc_verify(self, p, addrs, caps=(0, 0, 0, 0, 0), start=0) -> int:
        base = S.ST_IP_OK | S.ST_IP_VALID
        dropped = base | S.ST_L4_OK | S.ST_L4_VALID | S.ST_MALFORMED
        if len(p) < 1 or p[0] >> 3 != 0x1E or 1 + (4, 3, 3, 1)[p[0] & 3] + (0 if p[0] & 4 else 2) > len(p):
            return dropped
        c, fo, dport = self.nhc_csum(p, addrs, False, start)
        if dport == 0:
            return dropped
        valid = bool(p[0] & 4) or c == rd16(p, fo)
        ok = valid or caps[1] not in (0, 1)
        return base | (S.ST_L4_VALID if valid else 0) | (S.ST_L4_OK | S.ST_ACCEPT if ok else 0)

    def nhc_emit(self, p, addrs, caps=(0, 0, 0, 0, 0), start=0):
        p = bytearray(p)
        if len(p) < 1 or p[0] >> 3 != 0x1E or 1 + (4, 3, 3, 1)[p[0] & 3] + 2 > len(p):
            return S.ST_MALFORMED, bytes(p)
        if caps[1] in (0, 2):
            c, fo, _ = self.nhc_csum(p, addrs, True, start)
            p[0] &= 0xFB
            p[fo:fo + 2] = c.to_bytes(2, "big")
        return 0, bytes(p)


PLAIN = Arith()


def inc(f: int) -> int:
    """f + 1 in one's complement (both zeros go to 1)."""
    return f % 0xFFFF + 1


def dec(f: int) -> int:
    """f - 1 in one's complement (both zeros go to 0xfffe, 1 goes to 0xffff)."""
    return (f - 2) % 0xFFFF + 1


# ---------------------------------------------------------------------------------------------
# Classes and families, from the bytes
# ---------------------------------------------------------------------------------------------

L4_NAME = {P_UDP: "udp", P_TCP: "tcp", P_IGMP: "igmp", P_ICMP6: "echo"}
SUM_CLASSES = ("C0", "C1", "CFFFE", "CFFFF", "ZERO", "D0", "PH0", "D0PH0", "H0", "HFFFF", "IN0")
PARTIAL_CLASSES = ("PARTIAL", "PARTIAL+1", "PARTIAL-1", "PARTIAL/PH0=ffff", "PARTIAL/PH0=0000")
CLASSES = SUM_CLASSES + PARTIAL_CLASSES
FAMILIES = tuple(f"v4/{p}{o}" for o in ("", "+opt") for p in ("udp", "tcp", "echo", "igmp", "icmperr")) \
    + tuple(f"v6/{p}{o}" for o in ("", "+hbh") for p in ("udp", "tcp", "echo"))
TOP_FAMILIES = (("v4/udp+opt", KIND_ETH), ("v6/tcp", KIND_IP), ("v6/tcp", KIND_ETH))


def family_of(rec, g: S.Geom) -> str:
    l4 = ("icmperr" if S.embedded_header(rec, g) else "echo") if g.proto == P_ICMP4 else L4_NAME[g.proto]
    return f"v{g.fam}/{l4}" + ("+opt" if g.ip_hl > 20 else "") + ("+hbh" if g.hbh else "")


def aligned_le_sum(rec, start: int) -> int:
    """The sum a kernel's accumulator holds after a whole record: its little-endian 16-bit words on the
    buffer's 2-byte grid (an odd start leaves the first byte a lone high byte)."""
    rec = bytes(rec)
    if start % 2:
        return rec[0] * 256 + sum(rec[1::2]) + sum(rec[2::2]) * 256
    return sum(rec[0::2]) + sum(rec[1::2]) * 256


def classify(rec, kind: int, flags: int = 0, start: int = 0):
    """(family, the classes the record's bytes are in), or (None, empty) where it reaches no gate."""
    g = S.geometry(rec, kind, flags)
    if not g.gate:
        return None, set()
    A, out = PLAIN, set()
    ph, body, field, _ = A.l4(rec, g)
    c = A.csum(ph + body)
    out |= {{0: "C0", 1: "C1", 0xFFFE: "CFFFE", 0xFFFF: "CFFFF"}.get(c)} - {None}
    d0, ph0 = body != 0 and body % 0xFFFF == 0, ph != 0 and ph % 0xFFFF == 0
    out |= ({"ZERO"} if ph + body == 0 else set()) | ({"D0"} if d0 else set()) | ({"PH0"} if ph0 else set()) \
        | ({"D0PH0"} if d0 and ph0 else set())
    if g.fam == 4:
        h = A.csum(A.header(rec, g.ip_off, g.ip_hl))
        out |= {{0: "H0", 0xFFFF: "HFFFF"}.get(h)} - {None}
    emb = S.embedded_header(rec, g)
    if emb and A.csum(A.header(rec, *emb)) == 0:
        out.add("IN0")
    if g.proto in (P_UDP, P_TCP):
        r = A.rep(ph)
        out |= {n for n, v in (("PARTIAL", r), ("PARTIAL+1", inc(r)), ("PARTIAL-1", dec(r))) if field == v}
        if ph0:
            out |= {n for n, v in (("PARTIAL/PH0=ffff", 0xFFFF), ("PARTIAL/PH0=0000", 0)) if field == v}
    if 1 << 31 <= aligned_le_sum(rec, start) < 1 << 32:
        out.add("TOP")
    return family_of(rec, g), out


def unreachable(cls: str, family: str):
    """Why no record of `family` can be in `cls`, or None where one can."""
    l4 = family.split("/")[1].split("+")[0]
    v4 = family.startswith("v4/")
    pseudo = l4 in ("udp", "tcp") or not v4
    if cls in ("CFFFF", "ZERO"):
        if pseudo:
            return "the pseudo-header holds the protocol number: the sum is never 0, so never computes to 0xffff"
        if l4 == "icmperr":
            return "the embedded header's version nibble is summed: the sum is never 0"
    if cls in ("PH0", "D0PH0") and not pseudo:
        return "ICMPv4 and IGMP have no pseudo-header"
    if cls.startswith("PARTIAL") and l4 not in ("udp", "tcp"):
        return "SMOL_ST_L4_PARTIAL exists for UDP and TCP only"
    if cls in ("H0", "HFFFF", "IN0") and not v4:
        return "IPv6 has no header checksum"
    if cls == "HFFFF":
        return "the version nibble is summed: an IPv4 header's sum is never 0"
    if cls == "IN0" and l4 != "icmperr":
        return "no embedded header"
    return None


# ---------------------------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------------------------

PATTERNS = {"ff": b"\xff", "00": b"\x00", "ff00": b"\xff\x00", "00ff": b"\x00\xff", "8000": b"\x80\x00"}
CONTROL = "rand"
L4_HDR = {"udp": 8, "tcp": 20, "echo": 8, "igmp": 8, "icmperr": 28}  # the protocol's minimum span
SPARE = {"udp": 0, "tcp": 14, "echo": 6, "igmp": 6, "icmperr": 6}    # a header word to steer where no payload word is
LENGTHS = (63, 64, 65, 1471, 1472)
RESIDUES = (0, 1, 15, 16)  # start addresses modulo 32; Rec.res (mod 128) walks them over the four quarters
MAX_V4, MAX_V6 = 65535, 65535


@dataclass
class SRec(S.Rec):
    cls: str = ""      # what the builder steered for ("CTRL": the random-payload control)
    pattern: str = ""
    copy: str = ""     # which verify copy: "" the correct field, else the field's change


def _fill(pattern: str, n: int, rng) -> bytes:
    if pattern == CONTROL:
        return P.rand_bytes(rng, n)
    p = PATTERNS[pattern]
    return (p * (n // len(p) + 1))[:n]


def _l4(l4: str, v6: bool, n: int, pattern: str, rng, k: int, zero: bool = False) -> bytes:
    """An L4 span of n bytes, its field 0, the bytes behind the header the pattern's."""
    if zero:
        return bytes(n)
    body = _fill(pattern, n - L4_HDR[l4], rng)
    if l4 == "udp":
        return P.udp(1024 + k % 3000, S.CLOSED_PORTS[k % 2], body)
    if l4 == "tcp":
        return P.tcp(2000 + k % 3000, 80, body, seq=int(rng.integers(1, 1 << 32)), ack=int(rng.integers(0, 1 << 32)))
    if l4 == "echo":
        return P.icmp_echo(128 if v6 else 8, body)
    if l4 == "igmp":
        return bytes([0x16, 0, 0, 0, 224, 0, 0, 1 + k % 200]) + body
    inner = P.ipv4(bytes([10, 0, 0, 2]), bytes([10, 0, 0, 1]), 17, body, ident=int(rng.integers(0, 65536)))
    return P.icmp4_error(3, 3, inner)


def _ip(family: str, l4b: bytes, rng, ph0: bool) -> bytes:
    ver, rest = family.split("/")
    l4, wide = rest.split("+")[0], "+" in rest
    n = len(l4b)
    if ver == "v4":
        proto = {"udp": 17, "tcp": 6, "echo": 1, "igmp": 2, "icmperr": 1}[l4]
        s, d = (bytes(4), bytes(2) + P.be16(0xFFFF - proto - n)) if ph0 else (P.rand_bytes(rng, 4), P.rand_bytes(rng, 4))
        return P.ipv4(s, d, proto, l4b, ihl=15 if wide else 5, options=bytes([1]) * 40 if wide else None,
                      ident=int(rng.integers(0, 65536)))
    nh = {"udp": 17, "tcp": 6, "echo": 58}[l4]
    s, d = (bytes(16), bytes(14) + P.be16(0xFFFF - nh - n)) if ph0 else (P.rand_bytes(rng, 16), P.rand_bytes(rng, 16))
    return P.ipv6(s, d, 0, S.hbh_padn(nh, 0) + l4b) if wide else P.ipv6(s, d, nh, l4b)


def _raise(rec: bytearray, o: int, d: int):
    """Raise the word at record offset o by d in one's complement."""
    w = rd16(rec, o) + d
    rec[o:o + 2] = (w - 0xFFFF if w > 0xFFFF else w).to_bytes(2, "big")


def steer_offset(g: S.Geom, l4: str, n: int) -> int:
    """The record offset of the word steered: the last full word of the bytes behind the L4 header (behind every
    header window), or a spare header word where there is none."""
    o = (n & ~1) - 2
    return g.l4_off + (o if o >= L4_HDR[l4] else SPARE[l4])


def twin_of(rec: bytes, g: S.Geom, l4: str, n: int):
    """The record with one 0x0000 word behind its L4 header turned 0xffff (or the other way): the same sum
    modulo 0xffff.  None where no such word is."""
    keep = steer_offset(g, l4, n)
    for o in range(g.l4_off + L4_HDR[l4], g.l4_off + (n & ~1), 2):
        if o != keep and rec[o] == rec[o + 1] and rec[o] in (0, 0xFF):
            return rec[:o] + bytes([rec[o] ^ 0xFF]) * 2 + rec[o + 2:]
    return None


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.recs: list[SRec] = []
        self.turn = {}   # family -> how many (pattern, length) pairs it has used
        self.load = {}   # (kind, start residue mod 128) -> records placed there

    def shape(self, family, pattern=None):
        """The next (pattern, span length) of a family: 5 patterns against 7 lengths, so 35 pairs in turn."""
        l4 = family.split("/")[1].split("+")[0]
        t = self.turn[family] = self.turn.get(family, -1) + 1
        lens = (L4_HDR[l4], L4_HDR[l4] + 1) + LENGTHS
        return pattern or tuple(PATTERNS)[t % 5], lens[t % 7]

    def finish_record(self, rec: bytearray, kind, res, family, cls, pattern, l4, n):
        """Fill the checksums, add the record and its verify copies at start residue `res`."""
        _, data = PLAIN.emit(rec, kind)
        g = S.geometry(data, kind, emit=True)
        parent = len(self.recs)

        def add(b, copy=""):
            ok = PLAIN.verify(b, kind) & S.ST_ACCEPT
            self.recs.append(SRec(bytes(b), kind, 0, res, family, None if ok else copy or "class", parent if copy else -1,
                                  cls, pattern, copy))

        add(data)
        if cls in ("CTRL", "IN0"):
            return  # (no gate reads an embedded header's field on the way in)
        fo = g.ip_off + 10 if cls == "H0" else g.l4_off + S.L4_FIELD[g.proto]
        f = rd16(data, fo)
        vals = [("other-zero", f ^ 0xFFFF)] if f in (0, 0xFFFF) else []
        vals += [("+1", inc(f)), ("-1", dec(f))]
        if f >> 8 != f & 0xFF:
            vals.append(("swapped", (f & 0xFF) << 8 | f >> 8))
        if f != 0 and cls != "H0" and g.proto in (P_UDP, P_TCP):
            vals.append(("field-0", 0))  # UDP: no checksum, accepted; TCP: a wrong one
        seen = {f}
        for name, v in vals:
            if v not in seen:
                seen.add(v)
                add(data[:fo] + v.to_bytes(2, "big") + data[fo + 2:], name)
        if cls != "H0":
            t = twin_of(data, g, l4, n)
            if t is not None:
                add(t, "twin")

    def record(self, family, kind, res, cls, pattern=None, n=None):
        rng = self.rng
        l4 = family.split("/")[1].split("+")[0]
        pat, ln = self.shape(family, pattern)
        n = n or ln
        ph0 = "PH0" in cls
        ip = _ip(family, _l4(l4, family.startswith("v6/"), n, pat, rng, len(self.recs), zero=cls == "ZERO"), rng, ph0)
        rec = bytearray(PLAIN.emit(S._frame(ip, kind), kind)[1])  # (an embedded header's field is part of the L4 sum)
        g = S.geometry(rec, kind, emit=True)
        assert g.gate, (family, kind, n)
        ph, body, _, fo = PLAIN.l4(rec, g)
        so = steer_offset(g, l4, n)
        if cls in ("C0", "C1", "CFFFE"):
            _raise(rec, so, (PLAIN.csum(ph + body) - {"C0": 0, "C1": 1, "CFFFE": 0xFFFE}[cls]) % 0xFFFF)
        elif cls in ("D0", "D0PH0"):
            _raise(rec, so, -body % 0xFFFF)
        elif cls == "H0":
            _raise(rec, g.ip_off + 4, PLAIN.csum(PLAIN.header(rec, g.ip_off, g.ip_hl)))
        elif cls == "IN0":
            o, hl = S.embedded_header(rec, g)
            _raise(rec, o + 4, PLAIN.csum(PLAIN.header(rec, o, hl)))
        if cls.startswith("PARTIAL"):
            r = PLAIN.rep(ph)
            v = {"PARTIAL": r, "PARTIAL+1": inc(r), "PARTIAL-1": dec(r), "PARTIAL/PH0=ffff": 0xFFFF, "PARTIAL/PH0=0000": 0}[cls]
            _, data = PLAIN.emit(rec, kind)
            data = data[:fo] + v.to_bytes(2, "big") + data[fo + 2:]
            ok = PLAIN.verify(data, kind) & S.ST_ACCEPT
            self.recs.append(SRec(data, kind, 0, res, family, None if ok else "partial", -1, cls, pat, ""))
            return
        self.finish_record(rec, kind, res, family, cls, pat, l4, n)

    def residue(self, kind, res):
        """`res` (mod 32) in the least loaded quarter of the 128 bytes: the fixed-stride layouts hold one record of
        a start residue per 128 slots."""
        return min((res + 32 * q for q in range(4)), key=lambda r: self.load.get((kind, r), 0))

    def settle(self, since):
        for r in self.recs[since:]:
            if len(r.data) <= S.LMAX:
                self.load[(r.kind, r.res)] = self.load.get((r.kind, r.res), 0) + 1

    def cell(self, family, cls, pattern=None):
        """One class of one family: both kinds at the four start residues, each with the family's next
        (pattern, length)."""
        for kind in (KIND_IP, KIND_ETH):
            for res in RESIDUES:
                since = len(self.recs)
                self.record(family, kind, self.residue(kind, res), cls, pattern)
                self.settle(since)


def _top(family: str, kind: int, n: int | None = None) -> bytearray:
    """The longest record of a family (or one of n L4 bytes), every byte 0xff that the parse leaves free."""
    ff = b"\xff"
    if family == "v4/udp+opt":
        n = MAX_V4 - 60
        ip = b"\x4f\xff\xff\xff\xff\xff\xc0\x00\xff\x11\x00\x00" + ff * 48 + ff * 4 + P.be16(n) + bytes(2) + ff * (n - 8)
        et = b"\x08\x00"
    else:
        n = n or MAX_V6
        l4b = ff * 16 + bytes(2) + ff * (n - 18)  # TCP: data offset 15, the field at 16
        ip = b"\x6f\xff\xff\xff" + P.be16(n) + b"\x06\xff" + ff * 32 + l4b
        et = b"\x86\xdd"
    return bytearray((ff * 12 + et if kind == KIND_ETH else b"") + ip)


# ---- requests whose REPLY is in a class (verify_echo_reply, verify_unreach_reply) ----------------------------

REPLY_CLASSES = ("C0", "C1", "CFFFE", "ZERO", "H0", "IN0")
UNREACH_PROTO = 200  # a protocol number no gate knows: the protocol / next-header form of the refusal


def echo_reply_frame(rec, kind):
    from tests import echo_ref

    return echo_ref.reply_of(rec, kind)[2]


def unreach_reply_frame(rec, kind):
    from smoltcp_amd import engine as E
    from tests import unreach_ref

    return unreach_ref.reply_of(rec, kind, 0, E.make_port_map(set(range(1, 6000)) - set(S.CLOSED_PORTS)))[2]


def reply_classes(frame, kind):
    """The classes of a reply frame (its checksum fields still zero), from its bytes."""
    return classify(PLAIN.emit(frame, kind)[1], kind)


def request(rng, what: str, ver: int, kind: int, cls: str, pattern: str, n: int, k: int) -> bytes:
    """A record that verify accepts and whose echo reply (what = "echo") or ICMP error (what = "port": a UDP
    datagram to a closed port, "proto": an unknown protocol) is in `cls`.  The reply's sums are steered through
    what the reply takes over from the request: a data word for the ICMP checksum, an address word for the
    IPv4 header's and the embedded header's.  A UDP datagram's own checksum would cancel the steered word in the
    error's sum, so those datagrams carry none (field 0x0000)."""
    al = 4 if ver == 4 else 16
    s, d = (bytes([10 if ver == 4 else 0x20]) + P.rand_bytes(rng, al - 1) for _ in range(2))
    n = max(n, 2) if what == "proto" else n  # (nothing but the data to steer there)
    data = bytes(n) if cls == "ZERO" else _fill(pattern, n, rng)
    if what == "echo":
        l4b = (bytes([8, 0]) + bytes(6) if cls == "ZERO" else P.icmp_echo(8 if ver == 4 else 128, b"")) + data
        proto, frame_of, caps, hdr = 1 if ver == 4 else 58, echo_reply_frame, (0, 0, 0, 0, 0), 8
    elif what == "port":
        l4b, proto, frame_of, caps, hdr = P.udp(1024 + k % 3000, S.CLOSED_PORTS[k % 2], data), 17, unreach_reply_frame, (0, 1, 0, 0, 0), 8
    else:
        l4b, proto, frame_of, caps, hdr = data, UNREACH_PROTO, unreach_reply_frame, (0, 0, 0, 0, 0), 0
    rec = bytearray(S._frame(P.ipv4(s, d, proto, l4b) if ver == 4 else P.ipv6(s, d, proto, l4b), kind))
    ip = 14 if kind == KIND_ETH else 0
    l4 = ip + (20 if ver == 4 else 40)
    taken = min(len(l4b), 528 if ver == 4 else 1192) if what != "echo" else len(l4b)  # what the reply takes over
    word = l4 + ((taken & ~1) - 2 if (taken & ~1) - 2 >= hdr else 6 if what == "echo" else 0)
    frame = PLAIN.emit(frame_of(bytes(rec), kind), kind)[1]
    g = S.geometry(frame, kind, emit=True)
    if cls in ("C0", "C1", "CFFFE"):
        ph, body, _, _ = PLAIN.l4(frame, g)
        _raise(rec, word, (PLAIN.csum(ph + body) - {"C0": 0, "C1": 1, "CFFFE": 0xFFFE}[cls]) % 0xFFFF)
    elif cls == "H0":
        _raise(rec, ip + 14, PLAIN.csum(PLAIN.header(frame, g.ip_off, g.ip_hl)))    # the source address's low word
    elif cls == "IN0":
        _raise(rec, ip + 18, PLAIN.csum(PLAIN.header(frame, *S.embedded_header(frame, g))))  # the destination's
    return PLAIN.emit(rec, kind, 0, caps)[1]


def build_requests(b):
    t = 0
    for what in ("echo", "port", "proto"):
        for ver in (4, 6):
            for cls in REPLY_CLASSES:
                if cls == "ZERO" and (what, ver) != ("echo", 4) or cls == "H0" and ver == 6 or cls == "IN0" and (what == "echo" or ver == 6):
                    continue  # (an ICMPv6 sum holds the pseudo-header, an error's the embedded header: never all zero)
                for kind in (KIND_IP, KIND_ETH):
                    for res in RESIDUES:
                        t += 1
                        pattern, n = tuple(PATTERNS)[t % 5], (0, 1, 2, 63, 64, 65, 527, 1471, 1472)[t % 9]
                        data = request(b.rng, what, ver, kind, cls, pattern, n, t)
                        assert PLAIN.verify(data, kind) & S.ST_ACCEPT
                        fam = family_of(data, S.geometry(data, kind)) if what != "proto" else f"v{ver}/other"
                        b.recs.append(SRec(data, kind, 0, b.residue(kind, res), fam, None, -1, f"REPLY/{what}/{cls}", pattern, ""))
                        b.settle(len(b.recs) - 1)


def build_corpus(seed: int = 0x5C5):
    """The records of the sweep, checksums filled, each with its start residue (mod 128)."""
    b = _Builder(seed)
    for family in FAMILIES:
        b.cell(family, "CTRL", CONTROL)
        for cls in SUM_CLASSES + PARTIAL_CLASSES:
            if cls in ("CFFFF", "HFFFF") or unreachable(cls, family):
                continue  # (CFFFF is what ZERO computes to)
            if cls == "D0" and unreachable("PH0", family):
                continue  # no pseudo-header: D0 is C0 there
            b.cell(family, cls)
    build_requests(b)
    # the longest records: descriptor layouts only (Sweep keeps them out of the fixed strides)
    for family, kind in TOP_FAMILIES + (("v4/udp+opt", KIND_IP),):
        for i, res in enumerate(RESIDUES):
            rec = _top(family, kind)
            n = len(rec) - (14 if kind == KIND_ETH else 0) - (60 if family.startswith("v4") else 40)
            b.finish_record(rec, kind, res + 32 * (i % 4), family, "TOP", "ff", family.split("/")[1].split("+")[0], n)
    return b.recs


# ---------------------------------------------------------------------------------------------
# 6LoWPAN NHC UDP
# ---------------------------------------------------------------------------------------------

NHC_CLASSES = ("CTRL", "C0", "C1", "CFFFE", "D0", "PH0")
NHC_PAYLOADS = (0, 1, 63, 64, 65, 1471, 1472)


@dataclass
class NRec:
    data: bytes
    addrs: bytes   # source and destination address, 32 bytes
    cls: str
    copy: str
    parity: int    # of the start address it is packed at
    bad: bool


def nhc_record(rng, mode: int, elided: bool, plen: int, pattern: str, cls: str):
    """(an NHC UDP packet with its checksum filled, its addresses): ports of `mode` (an inline destination port
    is never 0), `plen` payload bytes of `pattern`, one word steered for `cls`: the payload's last full word, or
    the source address's last where the payload has none."""
    ports = bytearray(P.rand_bytes(rng, P.NHC_PORTS_SIZE[mode]))
    if mode in (0, 2):
        ports[-1] |= 1
    p = bytearray(bytes([0xF0 | mode]) + bytes(ports) + bytes(2) + _fill(pattern, plen, rng))
    hdr = len(p) - plen
    n = plen + 8
    addrs = bytearray(bytes(30) + P.be16(0xFFFF - 17 - n) if cls == "PH0" else P.rand_bytes(rng, 32))
    at = (p, hdr + (plen & ~1) - 2) if plen >= 2 else (addrs, 14)
    # mode 0b01 sums another destination port on the way in than on the way out (the reference's accessors, as
    # written): an inline field is steered for verify, which reads it; an elided one for emit, which writes it
    c, fo, _ = PLAIN.nhc_csum(p, addrs, elided)
    if cls in ("C0", "C1", "CFFFE"):
        _raise(at[0], at[1], (c - {"C0": 0, "C1": 1, "CFFFE": 0xFFFE}[cls]) % 0xFFFF)
    if cls == "D0" and plen >= 2:
        _raise(p, at[1], -wsum(p[hdr:]) % 0xFFFF)
    p[fo:fo + 2] = PLAIN.nhc_csum(p, addrs, elided)[0].to_bytes(2, "big")
    if elided:  # emit's input: the C bit set, the field's two bytes there for emit to fill (verify: payload bytes)
        p[0] |= 4
        p[fo:fo + 2] = bytes(2)
    return bytes(p), bytes(addrs)


def build_nhc(seed: int = 0x6C0):
    """Every port mode, inline and elided, every class at both start parities; an inline field's verify copies."""
    rng = np.random.default_rng(seed)
    out, t = [], 0
    for mode in range(4):
        for elided in (False, True):
            for cls in NHC_CLASSES:
                for parity in (0, 1):
                    for _ in range(4):
                        t += 1
                        pattern = CONTROL if cls == "CTRL" else tuple(PATTERNS)[t % 5]
                        data, addrs = nhc_record(rng, mode, elided, NHC_PAYLOADS[t % 7], pattern, cls)
                        fo = 1 + P.NHC_PORTS_SIZE[mode]
                        f = rd16(data, fo) if not elided else None
                        vals = [("", f)]
                        if not elided and cls != "CTRL":
                            vals += [("other-zero", f ^ 0xFFFF)] if f in (0, 0xFFFF) else []
                            vals += [("+1", inc(f)), ("-1", dec(f)), ("swapped", (f & 0xFF) << 8 | f >> 8)]
                        seen = set()
                        for name, v in vals:
                            if v in seen:
                                continue
                            seen.add(v)
                            d = data if v is None else data[:fo] + v.to_bytes(2, "big") + data[fo + 2:]
                            ok = PLAIN.nhc_verify(d, addrs) & S.ST_ACCEPT
                            out.append(NRec(d, addrs, cls, name, parity, not ok))
    return out


def nhc_pack(recs):
    """(buffer, offsets, lengths, n x 32 addresses): each record at a start address of its parity, a sentinel
    byte between two records where the parity asks for one."""
    chunks, offs, pos = [], [], 0
    for r in recs:
        if pos % 2 != r.parity:
            chunks.append(bytes([S.SENTINEL]))
            pos += 1
        offs.append(pos)
        chunks.append(r.data)
        pos += len(r.data)
    chunks.append(bytes([S.SENTINEL]) * 16)
    return (np.frombuffer(b"".join(chunks), np.uint8).copy(), np.array(offs, np.uint64), np.array([len(r.data) for r in recs], np.uint32),
            np.frombuffer(b"".join(r.addrs for r in recs), np.uint8).reshape(-1, 32).copy())


def nhc_class(p, addrs):
    """The classes of a well-formed NHC UDP packet, from its bytes: as verify sums it where the field is inline,
    as emit does where it is elided."""
    c, _, _ = PLAIN.nhc_csum(p, addrs, bool(p[0] & 4))
    hdr = 1 + P.NHC_PORTS_SIZE[p[0] & 3] + 2
    body, ph = wsum(p[hdr:]), wsum(addrs) + 17 + len(p) - hdr + 8
    return ({{0: "C0", 1: "C1", 0xFFFE: "CFFFE"}.get(c)} - {None}) | ({"D0"} if body and body % 0xFFFF == 0 else set()) \
        | ({"PH0"} if ph % 0xFFFF == 0 else set())


XWALK_LONGEST = 1024 * 16 - 127  # csum_dispatch.h xwalk_records: the last length the transposed walk's forms take


def xwalk_headroom(count: int = 130):
    """The transposed walk's longest records, Ethernet / IPv6 / TCP with every free byte 0xff, checksums filled;
    every third one's field is one too high.  (records, which are wrong)"""
    good = PLAIN.emit(_top("v6/tcp", KIND_ETH, XWALK_LONGEST - 54), KIND_ETH)[1]
    assert len(good) == XWALK_LONGEST and PLAIN.verify(good, KIND_ETH) & S.ST_ACCEPT
    fo = 54 + 16
    wrong = good[:fo] + inc(rd16(good, fo)).to_bytes(2, "big") + good[fo + 2:]
    return [wrong if i % 3 == 2 else good for i in range(count)], [i % 3 == 2 for i in range(count)]


# ---------------------------------------------------------------------------------------------
# Pieces: fragment groups and TCP sends (the fragment kernels and the two cut kernels)
# ---------------------------------------------------------------------------------------------
# These kernels fold each piece's sum to 16 bits, byte-swap it by the piece's address parity and add the folded
# values: a piece whose sum is a non-zero multiple of 0xffff folds to 0xffff, an all-zero one to 0, and the sum of
# the folded values carries out of 16 bits again.

TARGET = {"C0": 0, "C1": 1, "CFFFE": 0xFFFE}
PIECE_MODES = ("plain", "each0", "zeros")


def frag_step(mtu: int) -> int:
    return (mtu - 20) // 8 * 8


def frag_datagram(rng, proto: str, T: int, mtu: int, pattern: str, cls: str, mode: str, ident: int = 0) -> bytes:
    """An IPv4 datagram (IHL 5, checksum fields 0) of T L4 bytes whose L4 checksum computes to `cls`, one word
    steered in each of the slices an IP MTU of `mtu` cuts it into:
      plain  each slice's word moved by a random amount, the last slice's so that the class is met;
      each0  each slice's word set so that the slice (the L4 field 0) sums to a non-zero multiple of 0xffff, and the
             destination address's low word so that the class is met (ICMP has no pseudo-header: C0 there);
      zeros  a zero payload: every slice behind the first is all zero, the first one's word meets the class."""
    hdr, num = {"udp": (8, 17), "tcp": (20, 6), "echo": (8, 1)}[proto]
    body = bytes(T - hdr) if mode == "zeros" else _fill(pattern, T - hdr, rng)
    l4b = {"udp": lambda: P.udp(5000 + ident % 1000, 53, body), "tcp": lambda: P.tcp(6000 + ident % 1000, 80, body, seq=0xFFFFFF00),
           "echo": lambda: P.icmp_echo(8, body)}[proto]()
    d = bytearray(P.ipv4(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), num, l4b, flags_frag=0, ident=ident))
    step = frag_step(mtu)
    words = []
    for a in range(0, T, step):
        end = min(a + step, T)
        o = (end & ~1) - 2
        if o >= max(a, hdr if a == 0 else 0) or a == 0:  # (a slice of one byte has no word)
            words.append((a, 20 + (o if o >= hdr else SPARE[proto])))
    g = S.geometry(d, KIND_IP, emit=True)

    def need():
        ph, data, _, _ = PLAIN.l4(d, g)
        return (PLAIN.csum(ph + data) - TARGET[cls]) % 0xFFFF

    if mode == "each0":
        for a, w in words:
            _raise(d, w, -wsum(d[20 + a:20 + min(a + step, T)]) % 0xFFFF or 0xFFFF)  # (an all-zero slice: 0xffff in its word)
        if proto != "echo":
            _raise(d, 18, need())
    else:
        for _, w in words[:-1] if mode == "plain" else ():
            _raise(d, w, int(rng.integers(1, 0xFFFF)))
        _raise(d, (words[0] if mode == "zeros" else words[-1])[1], need())
    return bytes(d)


def frag_classes(d: bytes, mtu: int):
    """(the L4 class of a datagram, per slice: "zero", "mult" (a non-zero multiple of 0xffff) or "other")."""
    g = S.geometry(d, KIND_IP, emit=True)
    ph, data, _, _ = PLAIN.l4(d, g)
    step, T = frag_step(mtu), len(d) - 20
    fo = 20 + S.L4_FIELD[g.proto]
    z = d[:fo] + bytes(2) + d[fo + 2:]
    sums = [wsum(z[20 + a:20 + min(a + step, T)]) for a in range(0, T, step)]
    return {v: k for k, v in TARGET.items()}.get(PLAIN.csum(ph + data)), ["zero" if s == 0 else "mult" if s % 0xFFFF == 0 else "other" for s in sums]


def steer_send(payload: bytearray, frames_of, mss: int, cls: str, io_t: int):
    """Steer one word of each MSS slice of a TCP send's payload so that every frame's TCP checksum is `cls`.
    frames_of(payload) gives the frames with their checksums filled (tests/tcp_segment_ref.py); io_t: the TCP
    header's offset in a frame.  Slices of fewer than 2 bytes have no word and stay as they are."""
    frames = frames_of(bytes(payload))
    for k, f in enumerate(frames):
        a, n = k * mss, min(mss, len(payload) - k * mss)
        if n >= 2:
            _raise(payload, a + (n & ~1) - 2, (rd16(f, io_t + 16) - TARGET[cls]) % 0xFFFF)
    return payload
