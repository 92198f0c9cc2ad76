"""The edge sweep's corpus, placement and bookkeeping (CPU only; tests/test_edge_sweep_cpu.py and
tests/test_gpu_edge_sweep.py use it).

Every kernel reads a record's header bytes through a per-record LDS window with a fall-back to global
memory for the bytes behind it.  Three window models exist: 96 B from the record's 16-B chunk
(the tile kernel), 128 B from the 16-B chunk (the 16-B-grid walks, the copy kernels and the receive-side
batched calls), 256 B from the record's 128-B line (the line-grid walks, the transposed and the
descriptor walk).  Whether a record takes one of a kernel's slow paths depends on its start address
modulo 16 / 64 / 128 together with the record offset of the object read or written.  This module builds
one corpus in which every object meets every edge of every model, places it at exactly chosen start
addresses in three layouts, and computes which (object, edge) cells a placed corpus hits.

The geometry used here (`geometry`, `verify_model`, `emit_model`) is a Python restatement of the record
rules over oracle/pyref.py's checksum primitives, independent of oracle/csum_oracle.c and of every kernel;
tests/test_edge_sweep_cpu.py holds the two against each other over the whole corpus.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import pyref
from tests import pktgen as P

KIND_IP, KIND_ETH = 1, 2
REC_IPHDR_ONLY = 0x01
ST_IP_OK, ST_L4_OK, ST_L4_PARTIAL, ST_IP_VALID, ST_L4_VALID = 0x01, 0x02, 0x04, 0x08, 0x10
ST_MALFORMED, ST_UNSUPPORTED, ST_ACCEPT = 0x20, 0x40, 0x80
NO_FIELD = 0xFFFF
P_UDP, P_TCP, P_ICMP4, P_IGMP, P_ICMP6 = 17, 6, 1, 2, 58
PROTO_NAME = {P_UDP: "udp", P_TCP: "tcp", P_ICMP4: "icmp4", P_IGMP: "igmp", P_ICMP6: "icmp6"}
L4_FIELD = {P_UDP: 6, P_TCP: 16, P_ICMP4: 2, P_IGMP: 2, P_ICMP6: 2}

MODELS = [(96, 16), (128, 16), (256, 128)]  # (window bytes, the grid the window starts on)
SENTINEL = 0x5C                             # every byte of a placed buffer that belongs to no record
LMAX = 2200                                 # the longest record; the span-end family's records are this long
SPAN_T = (0, 1, 2, 3, 15, 16, 17)           # span end cells: bytes between the span's end and the record's
FAR_X = (1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049)
CLOSED_PORTS = (4000, 4001)                 # the corpus's UDP destination ports (verify_unreach_reply: closed)
ICMP6_MIN = {0x01: 8, 0x02: 8, 0x03: 8, 0x04: 8, 0x80: 8, 0x81: 8, 0x82: 28, 0x85: 8, 0x86: 16, 0x87: 24, 0x88: 24,
             0x89: 40, 0x8F: 8}


# ---------------------------------------------------------------------------------------------
# Record geometry and the verify / emit models (pure Python)
# ---------------------------------------------------------------------------------------------


@dataclass
class Geom:
    malformed: bool = False
    unsupported: bool = False
    fam: int = 0
    ip_off: int = 0
    ip_hl: int = 0
    proto: int = 0
    l4_off: int = 0
    l4_len: int = 0
    hbh: int = 0     # bytes of the leading Hop-by-Hop header
    cut: int = 0     # bytes the record is short of its IP length (a malformed, truncated record)
    ip_end: int = 0  # record offset of the end of the IP packet by its own length field

    @property
    def gate(self) -> bool:
        """The record reaches its checksum gate: neither MALFORMED nor UNSUPPORTED."""
        return not self.malformed and not self.unsupported and self.fam != 0


def _rd16(b, o):
    return b[o] << 8 | b[o + 1]


def _l4_malformed(rec, g: Geom, emit: bool) -> bool:
    l4, n = g.l4_off, g.l4_len
    if g.proto == P_UDP:
        if n < 8:
            return True
        ul = _rd16(rec, l4 + 4)
        if n < ul or ul < 8:
            return True
        return not emit and _rd16(rec, l4 + 2) == 0
    if g.proto == P_TCP:
        if n < 20:
            return True
        thl = (rec[l4 + 12] >> 4) * 4
        if n < thl or thl < 20:
            return True
        return not emit and (_rd16(rec, l4) == 0 or _rd16(rec, l4 + 2) == 0)
    if g.proto in (P_ICMP4, P_IGMP):
        return n < 8
    if g.proto == P_ICMP6:
        if n < 4:
            return True
        if emit:
            return False
        need = ICMP6_MIN.get(rec[l4], 0)
        return need == 0 or n < need
    return False


def geometry(rec, kind: int, flags: int = 0, emit: bool = False) -> Geom:
    """Where the reference's parse finds a record's headers, or why it drops the record."""
    g = Geom()
    n = len(rec)
    io = 0
    if kind == KIND_ETH:
        if n < 14:
            g.malformed = True
            return g
        et = _rd16(rec, 12)
        if et not in (0x0800, 0x86DD):
            g.unsupported = True
            return g
        io = 14
    elif kind != KIND_IP:
        g.unsupported = True
        return g
    lb = n - io
    if lb < 1:
        g.malformed = True
        return g
    ver = rec[io] >> 4
    if kind == KIND_ETH and ver != (4 if et == 0x0800 else 6):
        g.malformed = True
        return g
    if ver == 4:
        if lb < 20:
            g.malformed = True
            return g
        hl, total = (rec[io] & 15) * 4, _rd16(rec, io + 2)
        if lb < hl or hl > total or lb < total or hl < 20:
            g.malformed = True
            if hl >= 20 and hl <= total and lb >= hl:
                g.cut = total - lb
            return g
        g.fam, g.ip_off, g.ip_hl, g.ip_end = 4, io, hl, io + total
        if flags & REC_IPHDR_ONLY:
            g.unsupported = True
            return g
        if _rd16(rec, io + 6) & 0x3FFF:
            g.unsupported = True
            return g
        g.l4_off, g.l4_len = io + hl, total - hl
        if rec[io + 9] not in (P_UDP, P_TCP, P_ICMP4, P_IGMP):
            g.unsupported = True
            return g
        g.proto = rec[io + 9]
    elif ver == 6:
        if lb < 40:
            g.malformed = True
            return g
        plen = _rd16(rec, io + 4)
        if lb < 40 + plen:
            g.malformed = True
            g.cut = 40 + plen - lb
            return g
        g.fam, g.ip_off, g.ip_end = 6, io, io + 40 + plen
        if flags & REC_IPHDR_ONLY:
            g.unsupported = True
            return g
        cur, rem, nh = io + 40, plen, rec[io + 6]
        if nh == 0:
            if rem < 8:
                g.malformed = True
                return g
            ext = (rec[cur + 1] + 1) * 8
            if rem < ext:
                g.malformed = True
                return g
            if not emit and pyref.hbh_options_drop(bytes(rec[cur + 2:cur + ext])):
                g.malformed = True
                return g
            nh, cur, rem, g.hbh = rec[cur], cur + ext, rem - ext, ext
        g.l4_off, g.l4_len = cur, rem
        if nh not in (P_UDP, P_TCP, P_ICMP6):
            g.unsupported = True
            return g
        g.proto = nh
    else:
        g.malformed = True
        return g
    g.malformed = _l4_malformed(rec, g, emit)
    return g


def embedded_header(rec, g: Geom):
    """(record offset, header length) of the IPv4 header an ICMPv4 DstUnreachable / TimeExceeded message
    embeds, or None."""
    if g.malformed or g.proto != P_ICMP4:
        return None
    l4, n = g.l4_off, g.l4_len
    if rec[l4] in (3, 11) and n >= 28 and rec[l4 + 8] >> 4 == 4:
        ihl = (rec[l4 + 8] & 15) * 4
        if ihl >= 20 and 8 + ihl <= n:
            return l4 + 8, ihl
    return None


def span_end(rec, g: Geom) -> int:
    """Record offset of the byte after the L4 gate's summed span (UDP: its length field rules)."""
    if g.proto == P_UDP:
        return g.l4_off + _rd16(rec, g.l4_off + 4)
    return g.l4_off + g.l4_len


def field_offsets(rec, kind: int, flags: int = 0):
    """Record offsets of the checksum fields emit writes: [IPv4 header, L4, embedded header], None where
    the record has none."""
    g = geometry(rec, kind, flags, emit=True)
    out = [None, None, None]
    if g.fam == 4:
        out[0] = g.ip_off + 10
    if not g.malformed and g.proto:
        out[1] = g.l4_off + L4_FIELD[g.proto]
        emb = embedded_header(rec, g)
        if emb:
            out[2] = emb[0] + 10
    return out


def _rx(c):
    return c in (0, 1)


def _tx(c):
    return c in (0, 2)


def _addrs(rec, g: Geom):
    o = g.ip_off
    return (bytes(rec[o + 12:o + 16]), bytes(rec[o + 16:o + 20])) if g.fam == 4 else (bytes(rec[o + 8:o + 24]), bytes(rec[o + 24:o + 40]))


def verify_model(rec, kind: int, flags: int = 0, caps=(0, 0, 0, 0, 0)) -> int:
    """The status byte verify reports for one record."""
    g = geometry(rec, kind, flags)
    ip_valid = ip_ok = l4_valid = l4_ok = True
    partial = False
    if g.fam == 4:
        ip_valid = pyref.ipv4_verify(bytes(rec[g.ip_off:g.ip_off + g.ip_hl]))
        ip_ok = ip_valid if _rx(caps[0]) else True
    if not g.malformed and g.proto:
        l4 = bytes(rec[g.l4_off:g.l4_off + g.l4_len])
        src, dst = _addrs(rec, g)
        gate = 3
        if g.proto == P_UDP:
            l4_valid = pyref.udp_verify(l4, src, dst)
            partial = pyref.pseudo_header(src, dst, 17, _rd16(l4, 4)) == _rd16(l4, 6)
            gate = caps[1]
        elif g.proto == P_TCP:
            l4_valid = pyref.tcp_verify(l4, src, dst)
            partial = pyref.tcp_verify_partial(l4, src, dst)
            gate = caps[2]
        elif g.proto == P_ICMP4:
            l4_valid, gate = pyref.icmpv4_verify(l4), caps[3]
        elif g.proto == P_IGMP:
            l4_valid = pyref.icmpv4_verify(l4)  # never verified on ingress: the gate stays NONE
        else:
            l4_valid, gate = pyref.icmpv6_verify(l4, src, dst), caps[4]
        l4_ok = l4_valid if _rx(gate) else True
    st = (ST_IP_OK if ip_ok else 0) | (ST_L4_OK if l4_ok else 0) | (ST_L4_PARTIAL if partial else 0) \
        | (ST_IP_VALID if ip_valid else 0) | (ST_L4_VALID if l4_valid else 0) | (ST_MALFORMED if g.malformed else 0) \
        | (ST_UNSUPPORTED if g.unsupported else 0)
    if ip_ok and l4_ok and not g.malformed:
        st |= ST_ACCEPT
    return st


def emit_model(rec: bytearray, kind: int, flags: int = 0, caps=(0, 0, 0, 0, 0)):
    """Emit one record in place; returns (status byte, the three (off, val) field entries with NO_FIELD
    and 0 where the record has no such field)."""
    g = geometry(rec, kind, flags, emit=True)
    offs = field_offsets(rec, kind, flags)
    if g.fam == 4:
        h = bytearray(rec[g.ip_off:g.ip_off + g.ip_hl])
        if _tx(caps[0]):
            pyref.ipv4_fill(h)
        else:
            h[10:12] = b"\0\0"
        rec[g.ip_off:g.ip_off + g.ip_hl] = h
    if not g.malformed and g.proto:
        src, dst = _addrs(rec, g)
        l4 = bytearray(rec[g.l4_off:g.l4_off + g.l4_len])
        if g.proto == P_UDP:
            pyref.udp_fill(l4, src, dst) if _tx(caps[1]) else pyref.fill_l4(l4, 6, 0)
        elif g.proto == P_TCP:
            pyref.tcp_fill(l4, src, dst) if _tx(caps[2]) else pyref.fill_l4(l4, 16, 0)
        elif g.proto == P_ICMP4:
            if offs[2] is not None:
                ihl = (l4[8] & 15) * 4
                inner = bytearray(l4[8:8 + ihl])
                if _tx(caps[0]):
                    pyref.ipv4_fill(inner)
                else:
                    inner[10:12] = b"\0\0"
                l4[8:8 + ihl] = inner
            pyref.icmpv4_fill(l4) if _tx(caps[3]) else pyref.fill_l4(l4, 2, 0)
        elif g.proto == P_IGMP:
            pyref.icmpv4_fill(l4)
        else:
            pyref.icmpv6_fill(l4, src, dst) if _tx(caps[4]) else pyref.fill_l4(l4, 2, 0)
        rec[g.l4_off:g.l4_off + g.l4_len] = l4
    st = (ST_MALFORMED if g.malformed else 0) | (ST_UNSUPPORTED if g.unsupported else 0)
    return st, [(NO_FIELD, 0) if o is None else (o, _rd16(rec, o)) for o in offs]


# ---------------------------------------------------------------------------------------------
# Cells
# ---------------------------------------------------------------------------------------------

TWO = (-2, -1, 0)   # a 2-byte field: its first byte two and one before the window's end, and the first byte behind it
BYTE = (-1, 0)      # a byte: the window's last byte, the first byte behind it
LAST = (-1, 0, 1)   # a header's last byte (the byte after it is the next object's first)


def objects_of(rec, g: Geom):
    """(class, record offset, x offsets relative to W) of the objects a kernel reads or writes in the
    header of a record, and the checksum fields (class, record offset) among them."""
    objs, fields = [], []
    if g.fam == 4:
        objs += [("ipck", g.ip_off + 10, TWO), ("iplast", g.ip_off + g.ip_hl - 1, LAST)]
        fields.append(("ipck", g.ip_off + 10))
    if g.malformed or not g.proto:
        return objs, fields
    p, l4 = PROTO_NAME[g.proto], g.l4_off
    objs += [("l4ck_" + p, l4 + L4_FIELD[g.proto], TWO), ("l4first", l4, BYTE)]
    fields.append(("l4ck_" + p, l4 + L4_FIELD[g.proto]))
    if g.proto == P_UDP:
        objs += [("udplen", l4 + 4, TWO), ("dport_udp", l4 + 2, TWO)]
    elif g.proto == P_TCP:
        objs += [("dport_tcp", l4 + 2, TWO), ("doff", l4 + 12, BYTE)]
    emb = embedded_header(rec, g)
    if emb:
        objs += [("inck", emb[0] + 10, TWO), ("inlast", emb[0] + emb[1] - 1, LAST)]
        fields.append(("inck", emb[0] + 10))
    return objs, fields


# The largest record offset each object class can have, by the arithmetic of the headers before it
# (Ethernet 14, IPv4 header at most 60).  The classes IPv6 carries behind a Hop-by-Hop header of up to
# 2048 B are unbounded for this purpose.
MAX_OFF = {
    "ipck": 14 + 10,                   # 24
    "iplast": 14 + 60 - 1,             # 73
    "l4ck_icmp4": 14 + 60 + 2,         # 76: ICMPv4 rides IPv4 only
    "l4ck_igmp": 14 + 60 + 2,          # 76
    "inck": 14 + 60 + 8 + 10,          # 92
    "inlast": 14 + 60 + 8 + 60 - 1,    # 141
}
REL = {"ipck": TWO, "iplast": LAST, "l4ck_icmp4": TWO, "l4ck_igmp": TWO, "inck": TWO, "inlast": LAST,
       "l4ck_udp": TWO, "l4ck_tcp": TWO, "l4ck_icmp6": TWO, "l4first": BYTE, "udplen": TWO, "dport_udp": TWO,
       "dport_tcp": TWO, "doff": BYTE}
CK_FIELDS = ("ipck", "l4ck_udp", "l4ck_tcp", "l4ck_icmp4", "l4ck_igmp", "l4ck_icmp6", "inck")
CAUSES = ("udplen", "pad", "cut")


def window_cell(model, cls, x):
    return f"win{model[0]}/{model[1]}:{cls}@{x}"


def all_cells(model):
    """Every cell of the issue for one window model, reachable or not."""
    W = model[0]
    cells = {window_cell(model, c, W + d) for c, rel in REL.items() for d in rel}
    cells |= {f"abs64:{c}%{t}" for c in CK_FIELDS for t in (62, 63, 0)}
    cells |= {f"abs128:{c}%{t}" for c in CK_FIELDS for t in (126, 127, 0)}
    cells |= {f"far:l4ck_{p}@{x}" for p in ("udp", "tcp", "icmp6") for x in FAR_X}
    cells |= {f"spanend:{c}%16={v}" for c in CAUSES for v in range(16)}
    cells |= {f"spant:{c}={t}" for c in ("udplen", "pad") for t in SPAN_T}
    return cells


def unreachable_cells(model):
    """The window cells no record can hit: x = head + offset with head < grid, so x above
    grid - 1 + MAX_OFF[class] cannot occur."""
    W, grid = model
    return {window_cell(model, c, W + d) for c, m in MAX_OFF.items() for d in REL[c] if W + d > grid - 1 + m}


def cells_of(start: int, rec, g: Geom, model):
    """The cells one record at byte address `start` hits under `model`."""
    W, grid = model
    head = start % grid
    out = set()
    objs, fields = objects_of(rec, g)
    for cls, off, rel in objs:
        for d in rel:
            if head + off == W + d:
                out.add(window_cell(model, cls, W + d))
    for cls, off in fields:
        a = start + off
        if a % 64 in (62, 63, 0):
            out.add(f"abs64:{cls}%{a % 64}")
        if a % 128 in (126, 127, 0):
            out.add(f"abs128:{cls}%{a % 128}")
        if g.hbh and cls.startswith("l4ck") and start % 128 + off in FAR_X:
            out.add(f"far:{cls}@{start % 128 + off}")
    n = len(rec)
    if g.cut:  # a record cut short: the claimed span ends g.cut bytes behind the record's end
        if 1 <= g.cut <= 17:
            out.add(f"spanend:cut%16={(start + n) % 16}")
    elif not g.malformed and g.proto:
        e = span_end(rec, g)
        if g.proto == P_UDP and e < g.ip_end:
            cause, t = "udplen", g.ip_end - e if g.ip_end == n else None
        elif g.fam == 4 and g.ip_end < n:
            cause, t = "pad", n - e
        else:
            cause, t = None, n - e
        if cause:
            out.add(f"spanend:{cause}%16={(start + e) % 16}")
            if t in SPAN_T:
                out.add(f"spant:{cause}={t}")
        elif t == 0:
            out |= {f"spant:{c}=0" for c in ("udplen", "pad")}  # the span ends with the record, whatever the family
    return out


# ---------------------------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------------------------


@dataclass
class Rec:
    data: bytes
    kind: int
    flags: int
    res: int               # the start address modulo 128 this record is placed at
    family: str
    bad: str | None = None  # a bad-checksum copy: which byte was flipped
    twin: int = -1          # ... of which record


def hbh_padn(nh: int, units: int) -> bytes:
    """A Hop-by-Hop header of (units + 1) * 8 bytes filled with PadN options (each at most 257 bytes)."""
    total = (units + 1) * 8
    body, left = bytearray(), total - 2
    while left:
        dl = min(left - 2, 255)
        if left - 2 - dl == 1:  # a lone last byte could only be a Pad1: keep the header PadN throughout
            dl -= 1
        body += bytes([1, dl]) + bytes(dl)
        left -= 2 + dl
    return bytes([nh, units]) + bytes(body)


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.recs: list[Rec] = []
        self.load = {}          # (kind, flags) -> records per residue
        self.bad_cells = set()  # cells a bad-checksum copy hits already
        self.count = 0

    def _pick(self, kf, mod, val):
        """The least loaded start residue modulo 128 that is `val` modulo `mod`."""
        load = self.load.setdefault(kf, np.zeros(128, np.int64))
        cands = np.arange(val % mod, 128, mod)
        return int(cands[np.argmin(load[cands])])

    def residues(self, rec, kind, flags, extra=()):
        """The start residues (mod 128) at which this record hits a cell: one per cell and model."""
        g = geometry(rec, kind, flags)
        objs, fields = objects_of(rec, g)
        want = []  # (modulus, value)
        for cls, off, rel in objs:
            for W, grid in MODELS:
                for d in rel:
                    if 0 <= W + d - off < grid:
                        want.append((grid, W + d - off))
        for cls, off in fields:
            want += [(128, (t - off) % 128) for t in (126, 127, 0, 62, 63, 64)]  # both 64-B edges of a line
            if g.hbh:
                want += [(128, x - off) for x in FAR_X if 0 <= x - off < 128]
        want += list(extra)
        out = []
        for mod, val in sorted(set(want), key=lambda mv: -mv[0]):  # the exact ones first
            if any(r % mod == val % mod for r in out):
                continue
            out.append(self._pick((kind, flags), mod, val))
        return out

    def add(self, rec, kind, flags, res, family):
        self.load.setdefault((kind, flags), np.zeros(128, np.int64))[res] += 1
        self.recs.append(Rec(bytes(rec), kind, flags, res, family))
        self.count += 1
        return len(self.recs) - 1

    def finish(self, caps=(0, 0, 0, 0, 0)):
        """Fill every checksum (the emit model agrees with the oracle: test_edge_sweep_cpu), then add the
        bad-checksum copies: one record in five, and every record that hits a cell no copy has hit yet."""
        import oracle

        buf, offs, lens = P.pack([r.data for r in self.recs])
        d = P.oracle_desc(offs, lens, [r.kind for r in self.recs], np.array([r.flags for r in self.recs], np.uint8))
        oracle.batch_emit(buf, d, len(d), caps=caps)
        for r, o, n in zip(self.recs, offs, lens):
            r.data = buf[int(o):int(o) + int(n)].tobytes()
        good = len(self.recs)
        turn = 0
        for i in range(good):
            r = self.recs[i]
            g = geometry(r.data, r.kind, r.flags)
            cells = set()
            for m in MODELS:
                cells |= cells_of(r.res, r.data, g, m)
            if not (i % 5 == 0 or (g.gate and cells - self.bad_cells)):
                continue
            flips = flip_offsets(r.data, r.kind, r.flags, g)
            names = [k for k in ("field0", "field1", "last", "after") if flips.get(k) is not None]
            if not names:
                continue
            name = names[turn % len(names)]
            turn += 1
            b = bytearray(r.data)
            b[flips[name]] ^= 0x5A
            self.load[(r.kind, r.flags)][r.res] += 1
            self.recs.append(Rec(bytes(b), r.kind, r.flags, r.res, r.family, bad=name, twin=i))
            if g.gate:
                self.bad_cells |= cells
        return self.recs


def flip_offsets(rec, kind, flags, g: Geom | None = None):
    """The record offsets the four bad-checksum copies flip: the gate's field's two bytes, the last summed
    byte, the first byte after the span (None where the record has none).  The gate is the L4 one where
    verify has one (not IGMP, never verified on ingress), else the IPv4 header's."""
    g = g or geometry(rec, kind, flags)
    out = {}
    if not g.malformed and g.proto and g.proto != P_IGMP:
        f, e = g.l4_off + L4_FIELD[g.proto], span_end(rec, g)
        out = {"field0": f, "field1": f + 1, "last": e - 1, "after": e if e < len(rec) else None}
    elif g.fam == 4:
        f, e = g.ip_off + 10, g.ip_off + g.ip_hl
        # (IGMP's first byte still feeds its L4_VALID bit: no such copy there)
        out = {"field0": f, "field1": f + 1, "last": e - 1, "after": e if e < len(rec) and not g.proto else None}
    return out


def _frame(ip: bytes, kind: int) -> bytes:
    return P.eth(ip, 0x0800 if ip[0] >> 4 == 4 else 0x86DD) if kind == KIND_ETH else ip


def build_corpus(seed: int = 0xED6E):
    """The records of the sweep, checksums filled, each with the start residue (mod 128) it is placed at."""
    b = _Builder(seed)
    rng = b.rng
    port = lambda: CLOSED_PORTS[b.count % 2]  # noqa: E731

    def put(ip, family, twin=False, extra=()):
        for kind in (KIND_IP, KIND_ETH):
            rec = _frame(ip, kind)
            for res in b.residues(rec, kind, 0, extra):
                b.add(rec, kind, 0, res, family)
            if twin:  # the raw-socket twin: the IPv4 header's gate only
                for res in b.residues(rec, kind, REC_IPHDR_ONLY):
                    b.add(rec, kind, REC_IPHDR_ONLY, res, family + "/hdronly")

    def pay(lo=0, hi=40):
        return P.rand_bytes(rng, int(rng.integers(lo, hi)))

    a4 = lambda: (P.rand_bytes(rng, 4), P.rand_bytes(rng, 4))  # noqa: E731
    a6 = lambda: (P.rand_bytes(rng, 16), P.rand_bytes(rng, 16))  # noqa: E731
    # IPv4, IHL 5..15
    for ihl in range(5, 16):
        opts = bytes([1]) * (ihl * 4 - 20)  # No-Operation options
        s, d = a4()
        put(P.ipv4(s, d, 17, P.udp(1024 + ihl, port(), pay()), ihl=ihl, options=opts), "v4/udp", twin=True)
        for doff in (5 + (ihl * 3) % 11, 15):
            put(P.ipv4(s, d, 6, P.tcp(2000 + ihl, 80, pay(), doff=doff, seq=int(rng.integers(1, 1 << 31))), ihl=ihl,
                       options=opts), "v4/tcp", twin=doff == 15)
        put(P.ipv4(s, d, 1, P.icmp_echo(8, pay()), ihl=ihl, options=opts), "v4/echo", twin=True)
        put(P.ipv4(s, d, 2, bytes([0x16, 0, 0, 0]) + P.rand_bytes(rng, 4), ihl=ihl, options=opts), "v4/igmp")
        for in_ihl in sorted({5, 15, 5 + (ihl * 7) % 11}):
            inner = P.ipv4(d, s, 17, P.rand_bytes(rng, 8 + int(rng.integers(0, 24))), ihl=in_ihl,
                           options=bytes([1]) * (in_ihl * 4 - 20), csum=int(rng.integers(0, 65536)))
            put(P.ipv4(s, d, 1, P.icmp4_error(3 if in_ihl % 2 else 11, in_ihl % 4, inner), ihl=ihl, options=opts),
                "v4/icmperr", twin=in_ihl == 15)
    # IPv6: plain, and behind one Hop-by-Hop header whose length walks the L4 header over record offsets
    # 96, 128, 256 (every model's window end and the 128-B line's) and 1024, 2048 (the 1-KiB pieces)
    def l4_of(nh):
        return {17: P.udp(3000, port(), pay()), 6: P.tcp(3001, 443, pay(), doff=5 + b.count % 11, seq=int(rng.integers(1, 1 << 31))),
                58: P.icmp_echo(128, pay())}[nh]

    units = set()
    for edge, back in ((96, 40), (128, 40), (256, 152), (1024, 152), (2048, 152)):
        # the L4 objects lie at l4 + 0 .. l4 + 17 and head is below 16 (below 128 for the line grid):
        # l4 = 40 + 8 * (u + 1) (+ 14) from `back` bytes before the edge to just past it
        for l4 in range(edge - back, edge + 3):
            for io in (0, 14):
                u, rem = divmod(l4 - io - 40, 8)
                if rem == 0 and 1 <= u <= 256:
                    units.add(u - 1)
    for nh in (17, 6, 58):
        s, d = a6()
        put(P.ipv6(s, d, nh, l4_of(nh)), "v6/plain")
        for u in sorted(units):
            put(P.ipv6(s, d, 0, hbh_padn(nh, u) + l4_of(nh)), "v6/hbh")
    # the span-end family: every record LMAX bytes long, the span ends t bytes before the record's end
    for t in range(18):
        for v in range(16):
            for cause in CAUSES:
                for kind in (KIND_IP, KIND_ETH) if (t + v) % 4 == 0 else ((KIND_IP, KIND_ETH)[(t + v) % 2],):
                    io = 14 if kind == KIND_ETH else 0
                    s, d = a4()
                    body = LMAX - io - 20
                    if cause == "udplen":   # the UDP length field ends t bytes before the IP payload does
                        u = bytearray(P.udp(5000 + t, port(), P.rand_bytes(rng, body - 8)))
                        u[4:6] = P.be16(body - t)
                        ip = P.ipv4(s, d, 17, bytes(u))
                    elif cause == "pad":    # the IPv4 total length ends t bytes before the record does
                        l4 = P.tcp(5000 + t, 80, P.rand_bytes(rng, body - t - 20), seq=7) if v % 2 else \
                            P.udp(5000 + t, port(), P.rand_bytes(rng, body - t - 8))
                        ip = P.ipv4(s, d, 6 if v % 2 else 17, l4) + P.rand_bytes(rng, t)
                    else:                   # the record ends t bytes before its IPv4 total length does
                        if t == 0:
                            continue
                        ip = P.ipv4(s, d, 17, P.udp(5000 + t, port(), P.rand_bytes(rng, body + t - 8)))[:LMAX - io]
                    rec = _frame(ip, kind)
                    assert len(rec) == LMAX
                    e = LMAX if cause == "cut" else LMAX - t
                    b.add(rec, kind, 0, b._pick((kind, 0), 16, (v - e) % 16), "spanend/" + cause)
    return b.finish()


# ---------------------------------------------------------------------------------------------
# Placement
# ---------------------------------------------------------------------------------------------


@dataclass
class Placed:
    """Records in a buffer.  `index[i]` is the corpus record behind record i, -1 for a filler; fixed-stride
    layouts carry stride / length / kind / flags of the batch (record i at offs[i] = i * stride)."""
    buf: np.ndarray
    offs: np.ndarray
    lens: np.ndarray
    kinds: np.ndarray
    flags: np.ndarray
    index: np.ndarray
    bad: np.ndarray   # bool: a bad-checksum copy
    form: str
    stride: int = 0
    length: int = 0

    @property
    def n(self):
        return len(self.offs)

    def record(self, i) -> bytes:
        return self.buf[int(self.offs[i]):int(self.offs[i]) + int(self.lens[i])].tobytes()


def _filler(n: int, kind: int, rng) -> bytes:
    """A well-formed IPv4 / UDP record of exactly n >= 42 bytes to an open port (checksums left 0: the IPv4
    header fails verify, which is as good a neighbour as any)."""
    io = 14 if kind == KIND_ETH else 0
    return _frame(P.ipv4(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), 17, P.udp(9, 9, P.rand_bytes(rng, n - io - 28))), kind)


def place_desc(corpus, gaps: bool, keep=lambda res: True, seed: int = 1) -> Placed:
    """The descriptor layouts.  With gaps: sentinel bytes before each record bring it to its start residue.
    Back to back: a filler record of the same kind does (a record of the batch like any other), so that
    every record starts where the one before it ends.  `keep(res)`: thin the corpus by start residue (the
    proof that the coverage test can fail)."""
    rng = np.random.default_rng(seed)
    chunks, offs, lens, kinds, flags, index, bad = [], [], [], [], [], [], []
    pos = 0

    def put(data, kind, fl, idx, isbad):
        nonlocal pos
        for lst, v in ((offs, pos), (lens, len(data)), (kinds, kind), (flags, fl), (index, idx), (bad, isbad), (chunks, data)):
            lst.append(v)
        pos += len(data)

    for i, r in enumerate(corpus):
        if not keep(r.res):
            continue
        gap = (r.res - pos) % 128
        if gaps:
            chunks.append(bytes([SENTINEL]) * gap)
            pos += gap
        elif gap:
            put(_filler(gap + (128 if gap < 42 else 0), r.kind, rng), r.kind, 0, -1, False)
        put(r.data, r.kind, r.flags, i, r.bad is not None)
    chunks.append(bytes([SENTINEL]) * 144)
    return Placed(np.frombuffer(b"".join(chunks), np.uint8).copy(), np.array(offs, np.uint64), np.array(lens, np.uint32),
                  np.array(kinds, np.uint8), np.array(flags, np.uint8), np.array(index, np.int64), np.array(bad, bool),
                  "gaps" if gaps else "packed")


def place_fixed(corpus, kind: int, flags: int, length: int = LMAX, stride: int | None = None, keep=lambda res: True,
                seed: int = 2, limit: int = 64 << 20) -> Placed:
    """The fixed-stride layout of the corpus's records of one (kind, flags): an odd stride (consecutive
    records take all 128 start residues), records padded with random bytes to `length` (longer ones cut to
    it), each record in a slot of its start residue; slots no record wants hold a filler."""
    stride = stride or length + 1
    assert stride % 2 == 1 and stride >= length
    rng = np.random.default_rng(seed)
    queues = {}
    for i, r in enumerate(corpus):
        if r.kind == kind and r.flags == flags and keep(r.res):
            queues.setdefault(r.res, []).append(i)
    # the buffer stays under `limit`: a start residue with more records than there are slots of it gives up
    # records that hit no cell the records kept before them have not hit (never a cell)
    room = (limit - 144) // stride // 128
    seen = {False: set(), True: set()}
    for res in sorted(queues, key=lambda r: len(queues[r])):
        kept = []
        for i in queues[res]:
            r = corpus[i]
            g = geometry(r.data[:length], kind, flags)
            cells = set().union(*(cells_of(res, r.data[:length], g, m) for m in MODELS))
            isbad = r.bad is not None
            if len(queues[res]) <= room or cells - seen[isbad]:
                kept.append(i)
                seen[isbad] |= cells
        queues[res] = kept
    rounds = max(len(q) for q in queues.values())
    n = rounds * 128
    assert n * stride + 144 <= limit, (n, stride)
    buf = np.full(n * stride + 144, SENTINEL, np.uint8)
    index = np.full(n, -1, np.int64)
    bad = np.zeros(n, bool)
    fill = _filler(min(length, 64), kind, rng)
    for slot in range(n):
        q = queues.get(slot * stride % 128)
        o = slot * stride
        buf[o:o + length] = rng.integers(0, 256, length, dtype=np.uint8)
        if q:
            i = q.pop()
            index[slot], bad[slot] = i, corpus[i].bad is not None
            data = corpus[i].data[:length]
        else:
            data = fill
        buf[o:o + len(data)] = np.frombuffer(data, np.uint8)
    assert not any(queues.values())
    return Placed(buf, np.arange(n, dtype=np.uint64) * stride, np.full(n, length, np.uint32), np.full(n, kind, np.uint8),
                  np.full(n, flags, np.uint8), index, bad, "fixed", stride, length)


def coverage(placed_list, model):
    """(cells hit by a record that reaches its gate, cells hit by a bad-checksum copy that does) over the
    placed records, fillers left out.  The span-end cells of the cut cause are counted although such a
    record is MALFORMED: that is the cause."""
    good, bad = set(), set()
    for pl in placed_list:
        for i in range(pl.n):
            if pl.index[i] < 0:
                continue
            rec = pl.record(i)
            g = geometry(rec, int(pl.kinds[i]), int(pl.flags[i]))
            if not (g.gate or g.cut):
                continue
            cells = cells_of(int(pl.offs[i]), rec, g, model)
            (bad if pl.bad[i] else good).update(cells)
    return good, bad
