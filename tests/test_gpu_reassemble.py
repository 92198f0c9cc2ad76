"""GPU parity of verify_reassemble (smol_csum_batch_verify_reassemble): verify_frag's status bytes, one
smol_csum_dgram_t per group, and every usable group's fragment payloads put together in the group's slot
of a second device buffer, in one pass.

Every case runs on a descriptor batch with random gaps between the records (one case on a fixed stride)
and compares four things exactly:
  1. the status bytes with oracle.batch_verify_frag;
  2. the status bytes with eng.verify_frag on the same pre-filled status tensor;
  3. the datagram entries with tests/reassemble_ref.py;
  4. the WHOLE destination arena, filled with the sentinel 0xA5 beforehand, with the helper's: a stray
     store or a missing byte anywhere fails.
The batch buffer is compared too: it is only read.
"""
import numpy as np
import pytest

import oracle
from oracle import pyref
from tests import pktgen as P
from tests import reassemble_ref as R
from tests import test_frag_cpu as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)
PRE = 0x5A  # the status tensor's fill: bytes the call must not write keep it


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def _cut(dgram: bytes, sizes, ident: int):
    """Cut an emitted IPv4 datagram (20-byte header) into fragments of the given payload sizes (all but
    the last a multiple of 8), every header filled, as the iface's fragmenter leaves them."""
    hdr, data = dgram[:20], dgram[20:]
    assert sum(sizes) == len(data) and all(s % 8 == 0 for s in sizes[:-1])
    out, off = [], 0
    for i, s in enumerate(sizes):
        h = bytearray(hdr)
        h[2:4] = (20 + s).to_bytes(2, "big")
        h[4:6] = ident.to_bytes(2, "big")
        h[6:8] = ((0x2000 if i + 1 < len(sizes) else 0) | (off // 8)).to_bytes(2, "big")
        h[10:12] = b"\0\0"
        pyref.ipv4_fill(h)
        out.append(bytes(h) + data[off:off + s])
        off += s
    return out


def _udp(rng, T, sport=7, dport=9):
    return F.emit_whole(P.ipv4(F.A, F.B, 17, P.udp(sport, dport, P.rand_bytes(rng, T - 8))), F.DEFAULT)


def _slots_back_to_back(lens, start=3, gaps=None):
    """Slots one after the other from an odd offset (gaps[i] bytes before slot i, default none)."""
    offs, pos = [], start
    for i, ln in enumerate(lens):
        pos += int(gaps[i]) if gaps is not None else 0
        offs.append(pos)
        pos += int(ln)
    return np.array(offs, np.uint64), pos + 21


def _prepare(recs, groups, kind=E.KIND_IP, flags=0, caps=NOCAPS, slot_offs=None, slot_caps=None, arena_size=None,
             rec_offs=None, fixed=None, seed=0):
    """The host side of one case: the batch buffer and everything expected of the call."""
    n = len(recs)
    groups = [tuple(g) + (0,) * (3 - len(g)) for g in groups]
    kinds = np.broadcast_to(np.asarray(kind, np.uint8), (n,)).copy()
    flags_a = np.broadcast_to(np.asarray(flags, np.uint8), (n,)).copy()
    if fixed is not None:
        stride, base = fixed
        buf = np.random.default_rng(seed).integers(0, 256, base + n * stride + 64, dtype=np.uint8)
        offs = base + np.arange(n, dtype=np.uint64) * stride
        for o, r in zip(offs, recs):
            assert len(r) <= stride
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
        lens = np.full(n, stride, np.uint32)
    elif rec_offs is not None:
        offs = np.asarray(rec_offs, np.uint64)
        lens = np.array([len(r) for r in recs], np.uint32)
        buf = np.random.default_rng(seed).integers(0, 256, max(int(o) + len(r) for o, r in zip(offs, recs)) + 32, dtype=np.uint8)
        for o, r in zip(offs, recs):
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    else:
        buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(seed))
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    gh = np.array(groups, dtype=oracle.FRAG_GROUP_DTYPE)

    # default slots: every datagram's own length (a first pass of the helper with caps of 0 reports it)
    ng = len(groups)
    if slot_caps is None:
        slot_caps = R.expected(placed, kinds, flags_a, groups, np.zeros(ng, np.uint64), np.zeros(ng, np.int64), 1)[0]["len"]
    if slot_offs is None:
        slot_offs, arena_size = _slots_back_to_back(slot_caps)
    ref_dg, ref_arena = R.expected(placed, kinds, flags_a, groups, slot_offs, slot_caps, arena_size)

    if fixed is not None:
        ref_st = oracle.batch_verify_frag(buf[fixed[1]:].copy(), None, n, gh, stride=fixed[0], length=fixed[0],
                                          kind=oracle.kind_flags(int(kinds[0]), int(flags_a[0])), caps=caps)
    else:
        ref_st = oracle.batch_verify_frag(buf.copy(), E.make_descriptors(offs, lens, kinds, flags_a), n, gh, caps=caps)
    written = np.zeros(n, bool)  # records of valid groups: every other status byte keeps its fill
    for f, c, r in groups:
        if R.group_valid(int(f), int(c), int(r), n):
            written[int(f):int(f) + int(c)] = True
    return dict(n=n, buf=buf, offs=offs, lens=lens, kinds=kinds, flags=flags_a, gh=gh, slot_offs=slot_offs,
                slot_caps=np.asarray(slot_caps, np.uint32), arena_size=arena_size, dgrams=ref_dg, arena=ref_arena,
                status=np.where(written, ref_st, PRE).astype(np.uint8), written=written)


def _run(eng, recs, groups, caps=NOCAPS, fixed=None, accept=None, **kw):
    """One verify_reassemble call, compared exactly (the four comparisons of the module docstring).
    groups: (first, count) or (first, count, reserved) each.  Slots default to cap == T, back to back from
    offset 3.  Returns (status, dgrams) as numpy arrays."""
    w = _prepare(recs, groups, caps=caps, fixed=fixed, **kw)
    n, buf = w["n"], w["buf"]
    if fixed is not None:
        batch = E.Batch.fixed(n, fixed[0], fixed[0], int(w["kinds"][0]), flags=int(w["flags"][0]))
    else:
        batch = E.Batch.from_records(w["offs"], w["lens"], w["kinds"], "cuda:0", flags=w["flags"])
    d = torch.from_numpy(buf.copy()).cuda()
    dv = d[fixed[1]:] if fixed is not None else d
    gd = torch.from_numpy(w["gh"].view(np.uint8).copy()).cuda()
    dst = torch.full((w["arena_size"],), R.SENTINEL, dtype=torch.uint8, device="cuda")
    slots = torch.from_numpy(E.make_slots(w["slot_offs"], w["slot_caps"]).view(np.uint8).copy()).cuda()
    st0 = torch.full((n,), PRE, dtype=torch.uint8, device="cuda")
    st, dg = eng.verify_reassemble(dv, batch, gd, dst, slots, caps=caps, status=st0.clone())
    launched = eng.last_launch()
    vst = eng.verify_frag(dv, batch, gd, caps=caps, status=st0.clone())
    got_st, got_vst, got_dst = st.cpu().numpy(), vst.cpu().numpy(), dst.cpu().numpy()
    got_dg = dg.cpu().numpy().reshape(-1).view(E.DGRAM_DTYPE)
    assert launched["kernel"] == "fragcopy_kernel", launched
    assert np.array_equal(d.cpu().numpy(), buf), "the batch buffer is only read"
    assert np.array_equal(got_st, w["status"]), ("oracle", np.nonzero(got_st != w["status"])[0][:8])
    assert np.array_equal(got_st, got_vst), ("verify_frag", np.nonzero(got_st != got_vst)[0][:8])
    bad = np.nonzero(got_dg != w["dgrams"])[0]
    assert bad.size == 0, f"datagram entries differ at {bad[:8]}: got {got_dg[bad[:4]]} want {w['dgrams'][bad[:4]]}"
    diff = np.nonzero(got_dst != w["arena"])[0]
    assert diff.size == 0, f"destination bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {w['arena'][diff[:8]]})"
    if accept is not None:
        assert bool((got_st[w["written"]] & E.ST_ACCEPT).all()) == accept
    return got_st, got_dg


# ---- 1. the drop-in route ------------------------------------------------------------------------

@pytest.mark.parametrize("mtu,eth", [(68, True), (576, False), (1500, False)])
def test_drop_in_route(eng, mtu, eth):
    """F.tx_pair groups after emit_frag: UDP, TCP, ICMP echo and ICMP errors, fragment order shuffled, slots
    back to back from an odd offset; every datagram comes back whole and every status has ACCEPT."""
    rng = np.random.default_rng(mtu + 2)
    small = mtu == 68
    dgs = F.datagrams(rng, 40, 60 if small else 600, 900 if small else 8000)
    off, ref, groups = F.tx_pair(dgs, mtu, eth, shuffle_rng=rng)
    kind = E.KIND_ETH if eth else E.KIND_IP
    buf, offs, lens = P.pack(off, gap_rng=np.random.default_rng(mtu))
    batch = E.Batch.from_records(offs, lens, kind, "cuda:0")
    d = torch.from_numpy(buf.copy()).cuda()
    gd = torch.from_numpy(E.make_groups([f for f, _ in groups], [c for _, c in groups]).view(np.uint8).copy()).cuda()
    eng.emit_frag(d, batch, gd)
    got = d.cpu().numpy()
    filled = [got[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)]
    assert filled == ref
    st, dg = _run(eng, filled, groups, kind=kind, seed=mtu, accept=True)
    assert (dg["copied"] == 1).all() and [int(x) for x in dg["len"]] == [len(x) - 20 for x in dgs]
    assert {int(x) for x in dg["protocol"]} == {1, 6, 17}


# ---- 2. every alignment pair ---------------------------------------------------------------------

def test_every_alignment_pair(eng):
    """256 groups of two fragments: group g's first record starts at source offset g % 16 (mod 16), its slot
    at destination offset g // 16 (mod 16).  First fragments of 8, 16 and 24 bytes (half a chunk, one chunk,
    one and a half), last fragments of 1-17 bytes (less than, equal to and one more than a chunk)."""
    rng = np.random.default_rng(21)
    recs, groups, rec_offs, slot_offs, caps, pos, dpos = [], [], [], [], [], 0, 0
    for g in range(256):
        p0, p1 = (8, 16, 24)[g % 3], 1 + (g * 7) % 17
        T = p0 + p1
        fr = _cut(_udp(rng, T, sport=100 + g), [p0, p1], 0x100 + g)
        if g % 2:
            fr.reverse()
        groups.append((len(recs), 2))
        for j, r in enumerate(fr):
            if j == 0:
                pos += (g % 16 - pos) % 16
            else:
                pos += int(rng.integers(0, 8))
            rec_offs.append(pos)
            pos += len(r)
            recs.append(r)
        dpos += (g // 16 - dpos) % 16
        slot_offs.append(dpos)
        caps.append(T)
        dpos += T
    assert {int(rec_offs[2 * g]) % 16 for g in range(256)} == set(range(16))
    assert {(int(rec_offs[2 * g]) % 16, slot_offs[g] % 16) for g in range(256)} == {(a, b) for a in range(16) for b in range(16)}
    st, dg = _run(eng, recs, groups, rec_offs=rec_offs, slot_offs=np.array(slot_offs, np.uint64),
                  slot_caps=np.array(caps, np.uint32), arena_size=dpos + 19, seed=22, accept=True)
    assert (dg["copied"] == 1).all() and set(int(x) for x in dg["len"]) >= {9, 25, 41}


# ---- 3. the cap ----------------------------------------------------------------------------------

def test_cap_decides_the_copy(eng):
    """cap == T delivers; cap == T - 1 and cap == 0 store nothing, report len == T and copied == 0 and leave
    the status as it is; slots of cap 0 sit between full ones."""
    rng = np.random.default_rng(31)
    dgs = F.datagrams(rng, 30, 600, 5000)
    _, ref, groups = F.tx_pair(dgs, 576, shuffle_rng=rng)
    T = np.array([len(d) - 20 for d in dgs], np.int64)
    caps = T.copy()
    caps[1::3] -= 1
    caps[2::3] = 0
    offs, size = _slots_back_to_back(caps, start=5)
    st, dg = _run(eng, ref, groups, slot_offs=offs, slot_caps=caps.astype(np.uint32), arena_size=size, seed=32, accept=True)
    assert np.array_equal(dg["len"], T) and np.array_equal(dg["copied"], (np.arange(30) % 3 == 0).astype(np.uint8))


# ---- 4. the copy does not wait for the verdict ---------------------------------------------------

def test_rejected_datagrams_are_delivered_as_they_stand(eng):
    """One payload bit flipped, or one fragment's TTL flipped: the status rejects as the oracle does, and the
    bytes are delivered as they stand in the batch."""
    rng = np.random.default_rng(41)
    dgs = F.datagrams(rng, 30, 1500, 6000)
    _, ref, groups = F.tx_pair(dgs, 576, shuffle_rng=rng)
    recs = [bytearray(r) for r in ref]
    for gi, (f, c) in enumerate(groups):
        if gi % 3 == 0:  # a payload flip somewhere in the datagram
            r = recs[f + int(rng.integers(c))]
            r[20 + int(rng.integers(len(r) - 20))] ^= 1 << int(rng.integers(8))
        elif gi % 3 == 1:  # a header flip (TTL: not part of the reassembly key) in one fragment
            recs[f + int(rng.integers(c))][8] ^= 0x04
    recs = [bytes(r) for r in recs]
    for caps in (NOCAPS, (2, 0, 0, 0, 0), (0, 2, 2, 2, 0)):
        st, dg = _run(eng, recs, groups, caps=caps, seed=42)
        assert (dg["copied"] == 1).all()
        if caps == NOCAPS:
            for gi, (f, c) in enumerate(groups):
                assert bool((st[f:f + c] & E.ST_ACCEPT).all()) == (gi % 3 == 2), gi
                assert not (st[f:f + c] & E.ST_MALFORMED).any()


# ---- 5. non-usable and invalid groups ------------------------------------------------------------

def test_broken_and_invalid_groups_store_nothing(eng):
    rng = np.random.default_rng(51)
    _, ref, groups = F.tx_pair(F.datagrams(rng, 5, 2500, 2600), 576, shuffle_rng=rng)
    recs, glist = [], []
    (f0, c0), (f1, c1), (f2, c2), (f3, c3), (f4, c4) = groups
    parts = [ref[f0:f0 + c0],                                                # whole
             ref[f1:f1 + c1 - 1],                                            # a missing fragment
             ref[f2:f2 + c2] + [ref[f2]],                                    # a duplicate
             [ref[f3][:4] + b"\x55\x55" + ref[f3][6:]] + ref[f3 + 1:f3 + c3],  # an ident mismatch
             ref[f4:f4 + c4]]                                                # whole
    for part in parts:
        glist.append((len(recs), len(part), 0))
        recs += part
    n = len(recs)
    invalid = [(n, 1, 0), (n - 1, 2, 0), (0, 0, 0), (glist[4][0], glist[4][1], 1), (1 << 63, 3, 0), (0, 257, 0)]
    # the last whole group only appears as an invalid one (reserved != 0): its status bytes keep the fill
    allg = glist[:4] + invalid
    caps = np.full(len(allg), 4000, np.uint32)
    offs, size = _slots_back_to_back(caps, start=1)
    st, dg = _run(eng, recs, allg, slot_offs=offs, slot_caps=caps, arena_size=size, seed=52)
    zero = np.zeros(1, E.DGRAM_DTYPE)[0]
    assert dg[0]["copied"] == 1 and all(dg[i] == zero for i in range(1, len(allg)))
    assert (st[:glist[0][1]] & E.ST_ACCEPT).all()
    assert (st[glist[1][0]:glist[4][0]] & E.ST_MALFORMED).all()
    assert (st[glist[4][0]:] == PRE).all()


# ---- 6. delivered regardless of L4 ---------------------------------------------------------------

def test_delivered_regardless_of_l4(eng):
    rng = np.random.default_rng(61)
    recs, groups, flags = [], [], []

    def add(dgram, sizes=None, raw=False):
        T = len(dgram) - 20
        if sizes is None:
            step = 552
            sizes = [step] * ((T - 1) // step) + [T - (T - 1) // step * step]
        fr = _cut(dgram, sizes, 0x700 + len(groups))
        rng.shuffle(fr)
        groups.append((len(recs), len(fr)))
        for j, r in enumerate(fr):
            recs.append(r)
            flags.append(E.REC_IPHDR_ONLY if raw and j == len(fr) - 1 else 0)

    def whole(d):
        return F.emit_whole(d, F.DEFAULT)

    pay = P.rand_bytes(rng, 1700)
    add(_udp(rng, 1800), raw=True)                                              # 0 a raw socket's datagram
    add(whole(P.ipv4(F.A, F.B, 47, pay)))                                       # 1 GRE: no checksum gate
    add(whole(P.ipv4(F.A, F.B, 17, P.udp(7, 9, pay, length=8 + 1701))))         # 2 UDP length above T
    add(whole(P.ipv4(F.A, F.B, 17, P.udp(7, 9, pay[:1500]) + pay[1500:])))      # 3 UDP length below T
    add(whole(P.ipv4(F.A, F.B, 17, P.udp(7, 0, pay))))                          # 4 UDP destination port 0
    singles = [_udp(rng, 9), _udp(rng, 1472), whole(P.ipv4(F.A, F.B, 6, P.tcp(7, 9, pay[:333], doff=7))),
               whole(P.ipv4(F.A, F.B, 1, P.icmp_echo(8, pay[:64]))), whole(P.ipv4(F.A, F.B, 47, pay[:40]))]
    for s in singles:                                                           # 5.. one unfragmented packet each
        add(s, sizes=[len(s) - 20])
    st, dg = _run(eng, recs, groups, flags=np.array(flags, np.uint8), seed=62)
    assert (dg["copied"] == 1).all()

    def grp(i):
        f, c = groups[i]
        return st[f:f + c]

    assert (grp(0) & E.ST_UNSUPPORTED).all() and (grp(0) & E.ST_ACCEPT).all() and dg[0]["l4_len"] == 0
    assert (grp(1) & E.ST_UNSUPPORTED).all() and dg[1]["protocol"] == 47 and dg[1]["len"] == 1700
    assert (grp(2) & E.ST_MALFORMED).all() and (int(dg[2]["l4_off"]), int(dg[2]["l4_len"])) == (0, 0) and dg[2]["len"] == 1708
    assert (grp(3) & E.ST_ACCEPT).all() and (int(dg[3]["l4_off"]), int(dg[3]["l4_len"]), int(dg[3]["len"])) == (8, 1500, 1708)
    assert (grp(4) & E.ST_MALFORMED).all() and dg[4]["l4_len"] == 0
    assert (grp(5) & E.ST_ACCEPT).all() and (int(dg[5]["len"]), int(dg[5]["l4_len"])) == (9, 1)
    assert (int(dg[7]["l4_off"]), int(dg[7]["l4_len"])) == (28, 333) and (grp(7) & E.ST_ACCEPT).all()
    assert (grp(8) & E.ST_ACCEPT).all() and dg[8]["l4_off"] == 0 and (grp(9) & E.ST_UNSUPPORTED).all()


# ---- 7. a fixed-stride batch ---------------------------------------------------------------------

def test_fixed_stride_batch(eng):
    """Fragment records at a fixed stride of 1501 with slack (a device RX ring): the IP total length
    decides, the rest of each record is random filler."""
    rng = np.random.default_rng(71)
    _, ref, groups = F.tx_pair(F.datagrams(rng, 20, 1000, 5000), 1500, shuffle_rng=rng)
    st, dg = _run(eng, ref, groups, fixed=(1501, 7), seed=72, accept=True)
    assert (dg["copied"] == 1).all()


# ---- 8. extremes ---------------------------------------------------------------------------------

def test_extremes_share_a_launch(eng):
    """256 fragments of 8 bytes, 65 fragments, and one UDP datagram of T = 65515 in 45 fragments at MTU 1500,
    in one batch beside small groups: workgroups of very different length in one launch."""
    rng = np.random.default_rng(81)
    recs, groups = [], []

    def add(fr):
        fr = list(fr)
        rng.shuffle(fr)
        groups.append((len(recs), len(fr)))
        recs.extend(fr)

    small = F.tx_pair(F.datagrams(rng, 6, 100, 900), 576)[1:]
    for f, c in small[1][:3]:
        add(small[0][f:f + c])
    add(_cut(_udp(rng, 2048), [8] * 256, 0x801))
    add(_cut(_udp(rng, 64 * 24 + 5), [24] * 64 + [5], 0x802))
    big = _udp(rng, 65515)
    assert len(big) == 65535
    bf = P.fragment_like_iface(big, 1500, 0x803, fill_header=True)
    assert len(bf) == 45
    add(bf)
    for f, c in small[1][3:]:
        add(small[0][f:f + c])
    st, dg = _run(eng, recs, groups, seed=82, accept=True)
    assert (dg["copied"] == 1).all() and [int(x) for x in dg["len"][3:6]] == [2048, 64 * 24 + 5, 65515]
    assert [c for _, c in groups[3:6]] == [256, 65, 45]


def test_second_piece_after_a_multi_step_one(eng):
    """One group of 6 fragments of 2056 payload bytes (129 or 130 source chunks: a second step of the streamer),
    the last one shorter: waves 0 and 1 take a second fragment, loaded under a two-step one."""
    rng = np.random.default_rng(83)
    fr = _cut(_udp(rng, 5 * 2056 + 1001), [2056] * 5 + [1001], 0x804)
    st, dg = _run(eng, fr, [(0, 6)], seed=84, accept=True)
    assert int(dg[0]["copied"]) == 1 and int(dg[0]["len"]) == 5 * 2056 + 1001


# ---- 9. caps and the launch id -------------------------------------------------------------------

def test_every_caps_row_and_one_record_groups(eng):
    """The caps rows of test_group_caps_and_one_record_groups, groups of one unfragmented packet between
    fragmented datagrams, on batches filled under the same caps; the caps touch neither the entries nor
    the bytes."""
    rng = np.random.default_rng(91)
    dgs = F.datagrams(rng, 24, 300, 3000)
    off, _, groups = F.tx_pair(dgs, 1280, shuffle_rng=rng)
    singles = [F.emit_whole(d, F.IGNORED) for d in F.datagrams(rng, 8, 20, 1200)]
    recs = off + singles
    groups = groups + [(len(off) + i, 1) for i in range(len(singles))]
    seen = set()
    for caps in ((0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 3, 3, 3, 0), (2, 1, 2, 1, 3), (1, 2, 1, 2, 0)):
        # records as the iface left them (fields 0), filled by the oracle under the default caps, then
        # verified under `caps`
        buf, offs, lens = P.pack(recs)
        desc = P.oracle_desc(offs, lens, E.KIND_IP)
        oracle.batch_emit_frag(buf, desc, len(desc), np.array([(f, c, 0) for f, c in groups], dtype=oracle.FRAG_GROUP_DTYPE))
        filled = [buf[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)]
        st, dg = _run(eng, filled, groups, caps=caps, seed=sum(caps))
        assert (dg["copied"] == 1).all()
        seen.add(bytes(st))
        # the unfilled records under the same caps: rejected where a gate checks, delivered all the same
        st, dg = _run(eng, recs, groups, caps=caps, seed=sum(caps) + 1)
        assert (dg["copied"] == 1).all()
        seen.add(bytes(st))
    assert len(seen) > 3  # the caps did change the verdicts


def test_no_groups_launches_nothing(eng):
    e = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st, dg = eng.verify_reassemble(e, E.Batch.fixed(1, 64, 64, E.KIND_IP), e[:0], e, e[:0])
    assert dg.numel() == 0 and not st.cpu().numpy().any()
    with pytest.raises(Exception):  # slots not 16-byte aligned
        eng.verify_reassemble(e, E.Batch.fixed(1, 64, 64, E.KIND_IP), torch.zeros(16, dtype=torch.uint8, device="cuda"), e,
                              torch.zeros(32, dtype=torch.uint8, device="cuda")[8:24])
