"""The sum sweep's corpus on the CPU (tests/sum_sweep.py): the oracle, the edge sweep's Python model and the
plain integer reference agree on every record; every class of sums is reached by every family at both start
parities in every layout, the cells arithmetic forbids are listed with their reason and nothing else is
missing; and nine models with one wrong piece of arithmetic each disagree with the oracle on a class the corpus
names, which is the evidence that the GPU comparison (tests/test_gpu_sum_sweep.py) would fail for a kernel that
is wrong in that way."""
import numpy as np
import pytest

import oracle
from oracle import pyref
from tests import edge_sweep as S
from tests import pktgen as P
from tests import sum_sweep as Q

CAPS = [(0, 0, 0, 0, 0), (2, 3, 0, 1, 0)]
NHC_CAPS = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 2, 0, 0, 0), (0, 3, 0, 0, 0)]
FILLS = (0x0000, 0xFFFF, 0xA5A5, None)  # what emit finds in every checksum field (None: what the corpus holds)
LAYOUTS = ("packed", "gaps", "fixed")


@pytest.fixture(scope="module")
def corpus():
    return Q.build_corpus()


@pytest.fixture(scope="module")
def nhc():
    return Q.build_nhc()


def filled(rec: bytes, kind: int, fill) -> bytes:
    """The record with `fill` in every checksum field emit writes."""
    if fill is None:
        return rec
    b = bytearray(rec)
    for fo in S.field_offsets(rec, kind):
        if fo is not None:
            b[fo:fo + 2] = fill.to_bytes(2, "big")
    return bytes(b)


@pytest.fixture(scope="module")
def refs(corpus):
    """The oracle over the whole corpus, once: per caps (verify's status, emit's status, the emitted records).
    Emit runs over each of the four fills; what it leaves does not depend on the fill."""
    kinds = np.array([r.kind for r in corpus], np.uint8)
    buf, offs, lens = P.pack([r.data for r in corpus])
    desc = P.oracle_desc(offs, lens, kinds, 0)
    out = {}
    for caps in CAPS:
        vst = oracle.batch_verify(buf.copy(), desc, len(desc), caps=caps)
        raw = est = None
        for fill in FILLS:
            was = raw, est
            raw, _, _ = P.pack([filled(r.data, r.kind, fill) for r in corpus])
            est = oracle.batch_emit(raw, desc, len(desc), caps=caps)
            assert was[0] is None or (np.array_equal(raw, was[0]) and np.array_equal(est, was[1])), fill
        out[caps] = (vst, est, [raw[int(o):int(o + n)].tobytes() for o, n in zip(offs, lens)])
    return out


def test_corpus_size(corpus):
    assert 3000 <= len(corpus) <= 8862  # no larger than the edge sweep's
    assert {r.family for r in corpus} == set(Q.FAMILIES) | {"v4/other", "v6/other"} and {r.kind for r in corpus} == {S.KIND_IP, S.KIND_ETH}
    for fam in Q.FAMILIES:
        rs = [r for r in corpus if r.family == fam and r.cls != "TOP" and not r.cls.startswith("REPLY")]
        spans = {S.geometry(r.data, r.kind).l4_len for r in rs}
        assert {n % 2 for n in spans} == {0, 1}, fam                      # both parities of span length
        assert {63, 64, 65, 1471, 1472} <= spans and min(spans) + 1 in spans, (fam, sorted(spans))
        assert {r.pattern for r in rs} == set(Q.PATTERNS) | {Q.CONTROL}, fam
    assert max(len(r.data) for r in corpus) == 65589
    copies = {r.copy for r in corpus}
    assert copies == {"", "other-zero", "+1", "-1", "swapped", "field-0", "twin"}
    # the oracle's verdicts on the copies, recorded: a one's-complement neighbour and a byte swap are rejected wherever
    # a gate looks (IGMP has none); the other zero passes everywhere but behind an all-zero sum; a TCP field 0 is a
    # wrong checksum, a UDP one none at all; the invisible twin passes everywhere (behind an all-zero sum too: verify
    # sums the field 0xffff in, and it is emit that tells the two apart)
    for r in corpus:
        igmp = "igmp" in r.family and r.cls != "H0"  # (IGMP's own sum is never a gate; its IPv4 header's is)
        if r.copy in ("+1", "-1", "swapped"):
            assert (r.bad is None) == igmp, (r.family, r.cls, r.copy)
        elif r.copy == "other-zero":
            assert (r.bad is None) == (r.cls != "ZERO" or igmp), (r.family, r.cls, r.copy)
        elif r.copy == "twin":
            assert r.bad is None, (r.family, r.cls)
        elif r.copy == "field-0":
            assert (r.bad is None) == ("udp" in r.family), (r.family, r.cls)


@pytest.mark.parametrize("caps", CAPS)
def test_oracle_model_and_plain_reference_agree(corpus, refs, caps):
    vst, est, emitted = refs[caps]
    for i, r in enumerate(corpus):
        want = int(vst[i])
        assert S.verify_model(r.data, r.kind, 0, caps) == want, (i, r.family, r.cls, r.copy)
        assert Q.PLAIN.verify(r.data, r.kind, 0, caps) == want, (i, r.family, r.cls, r.copy)
        if caps == CAPS[0]:
            assert (r.bad is None) == bool(want & S.ST_ACCEPT), i
        if r.copy:
            continue  # (a verify copy differs from its parent in a field emit overwrites, or is its twin)
        for fill in FILLS:
            raw = filled(r.data, r.kind, fill)
            b = bytearray(raw)
            st, _ = S.emit_model(b, r.kind, 0, caps)
            assert (st, bytes(b)) == (int(est[i]), emitted[i]), (i, r.family, r.cls, fill)
            assert Q.PLAIN.emit(raw, r.kind, 0, caps) == (int(est[i]), emitted[i]), (i, r.family, r.cls, fill)
        if caps == CAPS[0] and not r.cls.startswith(("PARTIAL", "REPLY/port")):
            assert emitted[i] == r.data, i  # emit puts back what the corpus holds


@pytest.mark.parametrize("caps", NHC_CAPS)
def test_nhc_oracle_pyref_and_plain_reference_agree(nhc, caps):
    buf, offs, lens, addrs = Q.nhc_pack(nhc)
    assert {int(o) % 2 for o in offs} == {0, 1}
    desc = P.oracle_desc(offs, lens, 0)
    st = oracle.batch_nhc_udp_verify(buf.copy(), desc, len(nhc), addrs, caps=caps)
    out = buf.copy()
    est = oracle.batch_nhc_udp_emit(out, desc, len(nhc), addrs, caps=caps)
    for i, r in enumerate(nhc):
        assert Q.PLAIN.nhc_verify(r.data, r.addrs, caps) == st[i], i
        v = pyref.nhc_udp_verify(r.data, r.addrs[:16], r.addrs[16:])
        assert v is not None and bool(st[i] & S.ST_L4_VALID) == v and bool(st[i] & S.ST_ACCEPT) == (v or caps[1] in (2, 3)), i
        if caps == NHC_CAPS[0]:
            assert r.bad == (not st[i] & S.ST_ACCEPT), i
        got = out[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()
        assert Q.PLAIN.nhc_emit(r.data, r.addrs, caps) == (int(est[i]), got), i
        py = bytearray(r.data)
        if caps[1] in (0, 2):
            assert pyref.nhc_udp_fill(py, r.addrs[:16], r.addrs[16:])
        assert bytes(py) == got and est[i] == 0, i


def test_nhc_classes(nhc):
    """Every class in every port mode, inline and elided, at both start parities; the copies' verdicts: NHC UDP
    compares by equality, so the other zero is rejected like any other wrong value."""
    _, offs, _, _ = Q.nhc_pack(nhc)
    hit = set()
    for r, o in zip(nhc, offs):
        hit |= {(c, r.data[0] & 7, int(o) % 2) for c in Q.nhc_class(r.data, r.addrs)}
        if not r.data[0] & 4:
            assert r.bad == (r.copy != ""), (r.cls, r.copy)
    want = {(c, m, p) for c in Q.NHC_CLASSES[1:] for m in range(8) for p in (0, 1)}
    # (D0 steers a payload word: of a cell's four payload lengths at most two are the ones without one, 0 and 1)
    assert not want - hit, sorted(want - hit)
    assert any(r.copy == "other-zero" and r.cls == "C0" for r in nhc)
    # emit writes 0x0000 for a computed 0x0000: no map to 0xffff
    for r in nhc:
        if "C0" in Q.nhc_class(r.data, r.addrs) and r.data[0] & 4:
            fo = 1 + P.NHC_PORTS_SIZE[r.data[0] & 3]
            assert Q.PLAIN.nhc_emit(r.data, r.addrs)[1][fo:fo + 2] == b"\0\0"


# ---------------------------------------------------------------------------------------------
# Coverage
# ---------------------------------------------------------------------------------------------


def place(corpus, layout, length=S.LMAX):
    if layout == "fixed":  # the longest records are for the descriptor layouts
        short = [r for r in corpus if len(r.data) <= S.LMAX]
        return [S.place_fixed(short, k, 0, length, length + 1, limit=96 << 20) for k in (S.KIND_IP, S.KIND_ETH)]
    return [S.place_desc(corpus, gaps=layout == "gaps")]


def table(placed):
    """{(class, family, kind, start parity)} and {(class, family, kind, start mod 32)} over placed records that
    reach their gate, from the placed bytes."""
    cells, residues = set(), set()
    for pl in placed:
        for i in np.flatnonzero(pl.index >= 0):
            start, kind = int(pl.offs[i]), int(pl.kinds[i])
            fam, classes = Q.classify(pl.record(i), kind, int(pl.flags[i]), start)
            cells |= {(c, fam, kind, start % 2) for c in classes}
            residues |= {(c, fam, kind, start % 32) for c in classes}
    return cells, residues


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_class_in_every_family(corpus, layout):
    placed = place(corpus, layout)
    if layout == "fixed":
        assert all(pl.stride % 2 == 1 and pl.buf.size < 64 << 20 for pl in placed)
        for pls in (placed, place(corpus, layout, 2304), place(corpus, layout, 4032)):  # none given up, at the transposed walk's lengths too
            assert sum((pl.index >= 0).sum() for pl in pls) == sum(len(r.data) <= S.LMAX for r in corpus)
    cells, residues = table(placed)
    kinds = (S.KIND_IP, S.KIND_ETH)
    want = {(c, f, k, p) for c in Q.CLASSES for f in Q.FAMILIES if not Q.unreachable(c, f) for k in kinds for p in (0, 1)}
    never = {(c, f, k, p) for c in Q.CLASSES for f in Q.FAMILIES if Q.unreachable(c, f) for k in kinds for p in (0, 1)}
    if layout != "fixed":
        want |= {("TOP", f, k, p) for f, k in Q.TOP_FAMILIES for p in (0, 1)}
    assert not want - cells, f"no record in {sorted(want - cells)[:12]}"
    assert not never & cells, sorted(never & cells)[:12]
    # bit 31 needs 2^31 / 0xffff > 32768 words: no IPv4 packet without a frame header has them, and nothing
    # shorter than the longest records comes near
    assert {c for c in cells if c[0] == "TOP"} <= want
    if layout != "fixed":  # every cell at start addresses 0, 1, 15 and 16 (modulo 32)
        lost = {(c, f, k, r) for c, f, k, _ in want for r in Q.RESIDUES} - residues
        assert not lost, sorted(lost)[:12]


def test_the_replies_classes(corpus):
    """The requests whose reply is in a class: the echo reply or the ICMP error, as tests/echo_ref.py and
    tests/unreach_ref.py build it and the plain reference fills it, is in the class, for every kind at both start
    parities.  ZERO is the IPv4 echo reply's alone, H0 IPv4's, IN0 the IPv4 error's."""
    hit = set()
    for r in corpus:
        if r.cls.startswith("REPLY/"):
            _, what, cls = r.cls.split("/")
            frame = (Q.echo_reply_frame if what == "echo" else Q.unreach_reply_frame)(r.data, r.kind)
            assert frame is not None, r.cls
            ver = frame[14 if r.kind == S.KIND_ETH else 0] >> 4
            assert cls in Q.reply_classes(frame, r.kind)[1], (r.cls, ver)
            st = Q.PLAIN.verify(r.data, r.kind)
            assert st & S.ST_ACCEPT and bool(st & S.ST_UNSUPPORTED) == (what == "proto")  # SEND is set for each
            hit.add((what, ver, cls, r.kind, r.res % 2))
    want = {(w, v, c) for w in ("echo", "port", "proto") for v in (4, 6) for c in Q.REPLY_CLASSES
            if not (c == "ZERO" and (w, v) != ("echo", 4) or c == "H0" and v == 6 or c == "IN0" and (w == "echo" or v == 6))}
    assert len(want) == 24
    assert hit == {(w, v, c, k, p) for w, v, c in want for k in (S.KIND_IP, S.KIND_ETH) for p in (0, 1)}


def test_the_unreachable_cells_are_the_listed_ones():
    reasons = {}
    for c in Q.CLASSES:
        for f in Q.FAMILIES:
            why = Q.unreachable(c, f)
            if why:
                reasons.setdefault(why, set()).add((c, f))
    assert len(reasons) == 7
    l4 = lambda f: f.split("/")[1].split("+")[0]  # noqa: E731
    pseudo = lambda f: l4(f) in ("udp", "tcp") or f.startswith("v6/")  # noqa: E731
    for f in Q.FAMILIES:
        gone = {c for c in Q.CLASSES if Q.unreachable(c, f)}
        want = {"HFFFF"} | ({"CFFFF", "ZERO"} if pseudo(f) or l4(f) == "icmperr" else set()) \
            | (set() if pseudo(f) else {"PH0", "D0PH0"}) | (set() if l4(f) in ("udp", "tcp") else set(Q.PARTIAL_CLASSES)) \
            | (set() if f.startswith("v4/") else {"H0"}) | (set() if l4(f) == "icmperr" else {"IN0"})
        assert gone == want, f


def test_top_records_set_bit_31(corpus):
    top = [r for r in corpus if r.cls == "TOP"]
    assert {(r.family, r.kind) for r in top} == set(Q.TOP_FAMILIES) | {("v4/udp+opt", S.KIND_IP)}
    assert {r.res % 32 for r in top} == set(Q.RESIDUES)
    for r in top:
        s = Q.aligned_le_sum(r.data, r.res)
        if (r.family, r.kind) in Q.TOP_FAMILIES:
            assert 1 << 31 <= s < 1 << 32, (r.family, r.kind, hex(s))
        else:  # 65535 bytes: the longest IPv4 packet stays below
            assert len(r.data) == 65535 and s < 1 << 31
    eth6 = [r for r in top if r.family == "v6/tcp" and r.kind == S.KIND_ETH and not r.copy]
    assert len(eth6) == 4 and all(len(r.data) == 65589 and r.data.count(0xFF) >= 65589 - 8 for r in eth6)


# ---------------------------------------------------------------------------------------------
# Mutants
# ---------------------------------------------------------------------------------------------


class ModRep(Q.Arith):
    """0 stands for every multiple of 0xffff, so a right sum is one that comes out 0."""

    def rep(self, x):
        return x % 0xFFFF

    def valid(self, total):
        return total % 0xFFFF == 0


class OneFold(Q.Arith):
    def rep(self, x):
        return ((x >> 16) + (x & 0xFFFF)) & 0xFFFF


class Acc31(Q.Arith):
    """The accumulator runs from the record's first byte and loses bit 31; the span is a difference of two of its
    values, as in the walk kernels."""

    def span(self, rec, a, b, start):
        if a % 2:
            return Q.wsum(rec[a:b])
        return ((Q.wsum(rec[:b]) & 0x7FFFFFFF) - Q.wsum(rec[:a])) & 0xFFFFFFFF


class NoUdpMap(Q.Arith):
    udp_map = ()


class MapEverywhere(Q.Arith):
    udp_map = (S.P_UDP, S.P_TCP)
    nhc_map = True


class TcpZeroSkip(Q.Arith):
    zero_skip = (S.P_UDP, S.P_TCP)


class SwapByLength(Q.Arith):
    """A span is summed on the buffer's 2-byte grid and byte-swapped (a multiplication by 256 modulo 0xffff) where
    it starts at an odd address.  The mutant swaps where its length is odd instead: right where both parities
    agree, the span's own sum there."""

    def span(self, rec, a, b, start):
        lead, chunk = (start + a) % 2, bytes(rec[a:b])
        if lead == (b - a) % 2:
            return Q.wsum(chunk)
        on_grid = (chunk[0] if lead and chunk else 0) + Q.wsum(chunk[lead:])
        return on_grid if lead else on_grid * 256


class PartialModulo(Q.Arith):
    def partial(self, ph, field):
        return (ph - field) % 0xFFFF == 0


class Borrow(Q.Arith):
    """The sum is folded before the field's old content comes off; the u32 borrow counts as 2^32 = 1 (mod 0xffff)."""

    def without(self, total, field):
        return (self.rep(total) - field) & 0xFFFFFFFF


# (the mutant, a (class, family fragment) it must be caught on, whether it is wrong for ordinary data too)
MUTANTS = {
    "1 x % 0xffff as the representative": (ModRep, ("C0", "tcp"), False),
    "2 one fold": (OneFold, ("CFFFE", ""), False),
    "3 a 31-bit accumulator": (Acc31, ("TOP", "v6/tcp"), False),
    "4 no UDP 0 -> 0xffff map": (NoUdpMap, ("C0", "udp"), False),
    "5 the map on TCP and NHC UDP": (MapEverywhere, ("C0", "tcp"), False),
    "6 the zero-field skip on TCP": (TcpZeroSkip, ("C1", "tcp"), False),
    # wrong wherever start and length parity differ, whatever the bytes: half of the controls
    "7 the swap by the span's length": (SwapByLength, ("C0", ""), True),
    "8 PARTIAL modulo 0xffff": (PartialModulo, ("PARTIAL/PH0=0000", "udp"), False),
    # wrong wherever the folded sum is below the field's old content: ordinary data under the 0xffff and 0xA5A5 fills
    "9 a borrow taken as 2^32": (Borrow, ("C0", ""), True),
}


def disagreements(model, corpus, refs):
    """The records on which a model's verify status or emitted bytes (under any fill) differ from the oracle's."""
    out = []
    for i, r in enumerate(corpus):
        for caps in CAPS:
            vst, est, emitted = refs[caps]
            if model.verify(r.data, r.kind, 0, caps, r.res) != vst[i] or any(
                    model.emit(filled(r.data, r.kind, fill), r.kind, 0, caps, r.res) != (int(est[i]), emitted[i])
                    for fill in (FILLS if not r.copy else ())):
                out.append(i)
                break
    return out


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_is_caught_on_a_named_class(corpus, nhc, refs, name):
    cls, (named, fam), ordinary = MUTANTS[name]
    bad = disagreements(cls(), corpus, refs)
    caught = set()
    for i in bad:
        r = corpus[i]
        f, classes = Q.classify(r.data, r.kind, 0, r.res)
        caught |= {(c, f) for c in classes}
    assert any(c == named and fam in f for c, f in caught), sorted(caught)[:20]
    controls = [i for i in bad if corpus[i].cls == "CTRL"]
    assert bool(controls) == ordinary, (name, len(controls))
    if name.startswith("5"):  # ... and on NHC UDP's C0, where the reference writes and expects 0x0000
        m = cls()
        wrong = [r for r in nhc if m.nhc_verify(r.data, r.addrs) != Q.PLAIN.nhc_verify(r.data, r.addrs)
                 or m.nhc_emit(r.data, r.addrs) != Q.PLAIN.nhc_emit(r.data, r.addrs)]
        assert wrong and all("C0" in Q.nhc_class(r.data, r.addrs) for r in wrong)


# ---------------------------------------------------------------------------------------------
# Pieces: fragment groups and TCP sends
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mtu", [68, 576, 1500])
def test_fragment_datagrams_meet_their_class_slice_by_slice(mtu):
    """Q.frag_datagram: the L4 checksum of the whole datagram is the class asked for, and the slices an IP MTU of
    `mtu` cuts are what the mode says: all zero behind the first, each a non-zero multiple of 0xffff (a last slice
    of one byte cannot be), or neither."""
    rng = np.random.default_rng(mtu)
    step = Q.frag_step(mtu)
    for proto in ("udp", "tcp", "echo"):
        for mode in Q.PIECE_MODES:
            for cls in Q.TARGET:
                for T in (2 * step + 1, 3 * step, 4 * step + 6):
                    for pattern in Q.PATTERNS:
                        d = Q.frag_datagram(rng, proto, T, mtu, pattern, cls, mode)
                        got, slices = Q.frag_classes(d, mtu)
                        assert len(slices) == -(-T // step)
                        if (proto, mode) != ("echo", "each0"):  # (no pseudo-header to steer: C0 where every slice is a multiple)
                            assert got == cls, (proto, mode, cls, T, pattern)
                        elif T % 2 == 0:
                            assert got == "C0"
                        if mode == "zeros":
                            assert set(slices[1:]) == {"zero"}
                        elif mode == "each0":
                            assert set(slices[:-1]) == {"mult"} and (slices[-1] == "mult" or T % step == 1)
                        # the oracle fills what the plain reference computes
                        whole = np.frombuffer(d, np.uint8).copy()
                        oracle.batch_emit(whole, None, 1, whole.size, whole.size, 1, CAPS[0])
                        assert whole.tobytes() == Q.PLAIN.emit(d, S.KIND_IP)[1]


def test_steered_sends_meet_their_class_frame_by_frame():
    from tests import tcp_segment_ref as T

    rng = np.random.default_rng(9)
    for mss in (536, 1460):
        for v6, eth in ((False, False), (True, True)):
            kind, io_t = (S.KIND_ETH if eth else S.KIND_IP), (14 if eth else 0) + (40 if v6 else 20)
            for cls in Q.TARGET:
                for pattern in Q.PATTERNS:
                    tpl = T.template(rng, v6=v6, eth=eth, doff=8, seq=0xFFFFFF00)
                    frames_of = lambda p: T.frames_of(tpl, kind, 0, p, mss, CAPS[0])[1]  # noqa: E731
                    pay = Q.steer_send(bytearray(Q._fill(pattern, 2 * mss + 7, rng)), frames_of, mss, cls, io_t)
                    frames = frames_of(bytes(pay))
                    assert len(frames) == 3 and all(Q.rd16(f, io_t + 16) == Q.TARGET[cls] for f in frames)
                    seqs = [int.from_bytes(f[io_t + 4:io_t + 8], "big") for f in frames]
                    assert seqs[0] == 0xFFFFFF00 and seqs[1] < seqs[0]  # the sequence number wraps inside the send
                    assert all(Q.PLAIN.emit(f, kind)[1] == f for f in frames)
