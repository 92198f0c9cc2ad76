"""GPU parity of udp_dequeue_emit (smol_csum_batch_udp_dequeue_emit): every socket's transmit PacketBuffer dequeued
and its datagrams written out as whole frames, headers built on the device, checksums filled, in one pass.

Every case compares exactly, against tests/udp_dequeue_ref.py (whose frames are pktgen's with the oracle's emit):
  1. the WHOLE d_tx array, filled with 0x5A beforehand: the entries of the dequeued datagrams hold the model's
     bytes, every other entry keeps its fill;
  2. the group entries (all zero for an invalid group);
  3. the WHOLE destination arena, filled with the sentinel 0xA5 beforehand: the SENT frames hold the model's
     bytes, every other byte (gaps between strided frames, the space behind a group's frames, the areas of
     invalid groups) holds the sentinel;
  4. d_src, d_meta and d_socks: they are only read;
and asserts that the launch was udptx_kernel."""
import numpy as np
import pytest

from tests import pktgen as P
from tests import udp_dequeue_ref as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

BOTH = (0, 0, 0, 0, 0)
PRE = 0x5A  # the fill of the d_tx, d_out and unused d_meta entries: bytes the call must not write keep it
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
ETH = (bytes([2, 0, 0, 0, 0, 9]), bytes([6, 5, 4, 3, 2, 1]))
SENT, OVER, PADDED = E.UTX_SENT, E.UTX_OVERSIZE, E.UTX_PADDED
EMPTY, MAX, NOSPACE, CORRUPT = E.UTX_STOP_EMPTY, E.UTX_STOP_MAX, E.UTX_STOP_NOSPACE, E.UTX_STOP_CORRUPT
STEP = 2048  # bytes of one step of udptx_kernel: 64 lanes x U = 2 chunks x 16 bytes


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def rnd(seed, *sizes):
    rng = np.random.default_rng(seed)
    return [P.rand_bytes(rng, s) for s in sizes]


def pad(n):
    return ("pad", n)


def raw(size, kind=E.UMETA_PACKET, family=4):
    """A metadata entry written as given, with no payload laid out for it."""
    return ("raw", size, kind, family)


def v6(p, **kw):
    return dict(p=p, fam=6, **kw)


class Tx:
    """Sockets whose payload rings lie one after the other in d_src (3 bytes between them), whose metadata rings lie
    one after the other in d_meta and whose d_tx ranges one after the other in d_tx (one unused entry between
    them), and whose frame areas lie one after the other in d_dst (5 bytes between them).  Every byte of d_src
    that is no payload is random."""

    def __init__(self, S=0):
        self.S, self.src_pos, self.meta_pos, self.dst_pos, self.tx_pos = S, 3, 1, 7, 1
        self.rows, self.writes, self.meta, self.overs = [], [], {}, []

    def add(self, entries, P_, M, pr=0, mr=0, pl=None, ml=None, cap=None, maxd=256, port=4000, mtu=1500, hop=64, eth=ETH,
            src_res=None, dst_res=None, over=None):
        """One socket.  entries, from the ring's front: payload bytes (an IPv4 datagram), v6(payload), pad(n),
        raw(...); the payloads are laid out from pr on, each in one piece.  pl / ml: the ring lengths when they are
        not what the entries add up to; cap: dst_cap when it is not exactly what the frames need; src_res /
        dst_res: the residue mod 16 of the first payload's and the first frame's address; over(socks, i): changes
        the finished socket entry.  Returns the group's index."""
        S = self.S
        while src_res is not None and (self.src_pos + pr) % 16 != src_res:
            self.src_pos += 1
        while dst_res is not None and self.dst_pos % 16 != dst_res:
            self.dst_pos += 1
        io = 14 if eth else 0
        w, used, rows, need, nsent, npkt = pr, 0, [], 0, 0, 0
        for j, it in enumerate(entries):
            e = np.zeros(1, E.UDPMETA_DTYPE)[0]
            if isinstance(it, tuple) and it[0] == "pad":
                e["size"], e["kind"] = it[1], E.UMETA_PADDING
                w, used = (w + it[1]) % P_, used + it[1]
            elif isinstance(it, tuple):
                e["size"], e["kind"], e["family"] = it[1:]
                npkt += 1
            else:
                d = it if isinstance(it, dict) else dict(p=it)
                p, fam = d["p"], d.get("fam", 4)
                assert w + len(p) <= P_, "a payload is one piece"
                self.writes.append((self.src_pos + w, p))
                remote, local = d.get("remote", A4 if fam == 4 else A6), d.get("local", B4 if fam == 4 else B6)
                e["size"], e["record"], e["src_port"], e["family"], e["kind"] = len(p), 77 + j, d.get("dport", 7000 + j), fam, E.UMETA_PACKET
                e["remote_addr"][:len(remote)] = np.frombuffer(remote, np.uint8)
                e["local_addr"][:len(local)] = np.frombuffer(local, np.uint8)
                w, used = ((w + len(p)) % P_ if P_ else 0), used + len(p)
                npkt += 1
                flen = io + (28 if fam == 4 else 48) + len(p)
                if flen - io <= mtu:
                    need = nsent * S + flen if S else need + flen
                    nsent += 1
            rows.append(e)
        for j, e in enumerate(rows):
            self.meta[self.meta_pos + (mr + j) % M] = e
        self.rows.append((self.src_pos, self.meta_pos, self.dst_pos, self.tx_pos, P_, pr, used if pl is None else pl, M, mr,
                          len(rows) if ml is None else ml, need if cap is None else cap, maxd, port, mtu, hop, eth))
        self.overs.append(over)
        self.src_pos += P_ + 3
        self.meta_pos += M + 1
        self.dst_pos += max(need, cap or 0) + 5
        self.tx_pos += min(npkt, 256) + 1
        return len(self.rows) - 1

    def build(self):
        src = np.random.default_rng(123).integers(0, 256, self.src_pos + 16, dtype=np.uint8)
        for at, p in self.writes:
            src[at:at + len(p)] = np.frombuffer(p, np.uint8)
        meta = np.full((self.meta_pos + 1) * 48, PRE, np.uint8).view(E.UDPMETA_DTYPE)
        for i, e in self.meta.items():
            meta[i] = e
        cols = list(zip(*self.rows))
        socks = E.make_udptxsocks(*cols[:15])
        for i, eth in enumerate(cols[15]):
            if eth:
                socks[i]["flags"] = E.UTXS_ETH
                socks[i]["eth_dst"], socks[i]["eth_src"] = np.frombuffer(eth[0], np.uint8), np.frombuffer(eth[1], np.uint8)
            if self.overs[i]:
                self.overs[i](socks, i)
        return src, socks, meta, self.dst_pos + 16, self.tx_pos + 1


def _launch(eng, tx, caps=BOTH, stream=None):
    """The call's tensors, filled, and the call issued on `stream`: (built arrays, tensors)."""
    src, socks, meta, dst_size, tx_size = built = tx.build()
    t = dict(src=torch.from_numpy(src.copy()).cuda(), socks=torch.from_numpy(socks.view(np.uint8).copy()).cuda(),
             meta=torch.from_numpy(meta.view(np.uint8).copy()).cuda(),
             dst=torch.full((dst_size,), D.SENTINEL, dtype=torch.uint8, device="cuda"),
             tx=torch.full((tx_size, 16), PRE, dtype=torch.uint8, device="cuda"),
             out=torch.full((len(socks), 32), PRE, dtype=torch.uint8, device="cuda"))
    assert all(x.data_ptr() % 16 == 0 for x in t.values())
    t["call"] = lambda s: eng.udp_dequeue_emit(t["src"], t["socks"], t["meta"], t["dst"], tx.S, caps=caps, tx=t["tx"],
                                               out=t["out"], stream=s)
    return built, t


def _check(tx, built, t, caps=BOTH):
    """The comparisons of the module docstring.  Returns the model's dict plus "got_arena"."""
    src, socks, meta, dst_size, tx_size = built
    exp = D.expected(src, socks, meta, caps, tx.S, dst_size, tx_size)
    want_tx = exp["tx"].view(np.uint8).reshape(tx_size, 16).copy()
    want_tx[~exp["tx_written"]] = PRE
    got_tx = t["tx"].cpu().numpy().reshape(tx_size, 16)
    got_out = t["out"].cpu().numpy().reshape(-1).view(E.UDPTXOUT_DTYPE)
    got_dst = t["dst"].cpu().numpy()
    assert np.array_equal(t["src"].cpu().numpy(), src), "d_src is only read"
    assert np.array_equal(t["meta"].cpu().numpy(), meta.view(np.uint8)), "d_meta is only read"
    assert np.array_equal(t["socks"].cpu().numpy(), socks.view(np.uint8)), "d_socks is only read"
    bad = np.nonzero(got_out != exp["outs"])[0]
    assert bad.size == 0, f"group entries differ at {bad[:8]}: got {got_out[bad[:4]]} want {exp['outs'][bad[:4]]}"
    bad = np.nonzero((got_tx != want_tx).any(axis=1))[0]
    assert bad.size == 0, f"d_tx entries differ at {bad[:8]}: got {got_tx[bad[:4]].copy().view(E.UDPTX_DTYPE)} " \
                          f"want {want_tx[bad[:4]].copy().view(E.UDPTX_DTYPE)}"
    diff = np.nonzero(got_dst != exp["arena"])[0]
    assert diff.size == 0, f"{diff.size} frame bytes differ, first at {diff[:8]} (got {got_dst[diff[:8]]} want " \
                           f"{exp['arena'][diff[:8]]}); frames at {[f[2] for f in exp['frames'][:8]]}"
    exp["got_arena"] = got_dst
    return exp


def _run(eng, tx, caps=BOTH, blocks=0, stream=None, graph=False):
    """One udp_dequeue_emit call, compared exactly.  graph: capture the call on a side stream and replay the graph."""
    eng.set_max_blocks(blocks)
    try:
        built, t = _launch(eng, tx, caps)
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                t["call"](side)  # (warm-up outside the capture)
                side.synchronize()
                t["dst"].fill_(D.SENTINEL), t["tx"].fill_(PRE), t["out"].fill_(PRE)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    t["call"](side)
                side.synchronize()
                assert bool((t["dst"] == D.SENTINEL).all()) and bool((t["out"] == PRE).all()), "the capture itself ran the kernel"
                g.replay()
                side.synchronize()
        elif stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                t["call"](stream)
            stream.synchronize()
        else:
            t["call"](None)
        launched = eng.last_launch()
        torch.cuda.synchronize()
    finally:
        eng.set_max_blocks(0)
    assert launched["kernel"] == "udptx_kernel" and launched["G"] == 64 and launched["U"] * 64 * 16 == STEP, launched
    return _check(tx, built, t, caps)


def _outs(exp, *names):
    return [tuple(int(o[n]) for n in names) for o in exp["outs"]]


# ---- sizes and alignment ----

SIZES = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 1472, STEP - 17, STEP - 16, STEP - 15, STEP - 1, STEP, STEP + 1, STEP + 15,
         STEP + 16, STEP + 17, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1]


@pytest.mark.parametrize("S", [0, 4400])
def test_sizes_over_the_step_boundaries(eng, S):
    """Every size of the list as IPv4 over Ethernet and as bare IPv6, back to back in one ring each: the chunk
    counts run over one, two and three steps of the piece pipeline at every alignment the sums give."""
    tx = Tx(S)
    pay = rnd(11, *SIZES)
    tx.add(pay, P_=sum(SIZES) + 9, M=len(SIZES), pr=5, mtu=9000)
    tx.add([v6(p) for p in pay], P_=sum(SIZES), M=len(SIZES) + 3, mr=7, mtu=9000, eth=None)
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "stop", "meta_len", "payload_len") == [(len(SIZES), EMPTY, 0, 0)] * 2


def test_largest_datagram_all_ones(eng):
    """65507 bytes of 0xff under ip_mtu 65535: the largest UDP payload IPv4 carries, every accumulator at its
    largest (a lane sums 64 chunks of eight 0xffff words)."""
    tx = Tx()
    tx.add([b"\xff" * 65507], P_=65536, M=1, pr=29, mtu=65535)
    tx.add([b"\xff" * 65507], P_=65507, M=1, mtu=65535, eth=None)
    exp = _run(eng, tx)
    assert exp["tx"]["ip_len"][exp["tx_written"]].tolist() == [65535, 65535]


@pytest.mark.parametrize("eth", [ETH, None], ids=["eth", "ip"])
def test_all_source_and_destination_residues(eng, eth):
    """All 16 x 16 residues of the payload's source address and the frame's address, sizes 33 .. 49, one group
    each, IPv4 and IPv6 in turn: every funnel shift, with and without a lead slot, heads at odd addresses (byte
    stores), slices at odd source addresses (RFC 1071 2(B))."""
    tx = Tx()
    pay = rnd(12, *[33 + i % 17 for i in range(256)])
    for sr in range(16):
        for dr in range(16):
            i = sr * 16 + dr
            tx.add([pay[i] if i % 2 else v6(pay[i])], P_=64, M=1, pr=i % 15, eth=eth, src_res=sr, dst_res=dr)
    exp = _run(eng, tx)
    starts = sorted(f[2] % 16 for f in exp["frames"])
    assert starts == sorted(list(range(16)) * 16) and len(exp["frames"]) == 256


def test_families_media_and_hop_limits(eng):
    """IPv4 and IPv6, with and without an Ethernet header, hop limits 1 and 255, different ports and addresses per
    datagram."""
    tx = Tx()
    pay = rnd(13, 40, 7, 300)
    g = 0
    for fam in (4, 6):
        for eth in (ETH, None, (b"\xff" * 6, bytes(range(6)))):
            for hop in (1, 255):
                ents = []
                for j, p in enumerate(pay):
                    a = bytes([g + 1, j]) * (2 if fam == 4 else 8)
                    ents.append(dict(p=p, fam=fam, dport=(1, 65535, 53)[j], remote=a, local=a[::-1]))
                tx.add(ents, P_=400, M=4, pr=g, mr=g % 4, port=(65535, 1, 4000)[g % 3], hop=hop, eth=eth)
                g += 1
    exp = _run(eng, tx)
    assert len(exp["frames"]) == 3 * g
    f = exp["frames"][0][3]
    assert f[:12] == ETH[0] + ETH[1] and f[14 + 8] == 1 and exp["frames"][3][3][14 + 8] == 255


@pytest.mark.parametrize("ip_caps,udp_caps", [(0, 0), (2, 1), (1, 2), (3, 3)])
def test_caps_transmit_settings(eng, ip_caps, udp_caps):
    """The four combinations of caps.ipv4.tx() and caps.udp.tx(): a field that is not filled is 0."""
    tx = Tx()
    pay = rnd(14, 100, 33)
    tx.add([pay[0], v6(pay[1])], P_=200, M=2)
    tx.add([v6(pay[0]), pay[1]], P_=200, M=2, eth=None)
    caps = (ip_caps, udp_caps, 0, 0, 0)
    exp = _run(eng, tx, caps=caps)
    f = exp["frames"][0][3]
    assert (f[14 + 10:14 + 12] != b"\0\0") == (ip_caps in (0, 2)) and (f[14 + 26:14 + 28] != b"\0\0") == (udp_caps in (0, 2))


@pytest.mark.parametrize("fam", [4, 6])
def test_checksum_that_computes_zero_is_written_ffff(eng, fam):
    """A payload steered so that the UDP checksum computes 0: the field carries 0xffff (udp.rs:194-208)."""
    body = rnd(15, 62)[0]
    mk = lambda tail: dict(p=body + tail, fam=fam)
    probe = Tx()
    probe.add([mk(b"\0\0")], P_=64, M=1, eth=None)
    src, socks, meta, dn, tn = probe.build()
    f = D.expected(src, socks, meta, BOTH, 0, dn, tn)["frames"][0][3]
    hl = 28 if fam == 4 else 48
    c = f[hl - 2:hl]  # the checksum with a zero tail is the complement of the sum: the tail that completes it to 0xffff
    tx = Tx()
    tx.add([mk(c), mk(b"\0\0")], P_=128, M=2, eth=None)
    tx.add([mk(c)], P_=64, M=1, pr=0, src_res=1, dst_res=3)
    exp = _run(eng, tx)
    got = [fr[3][(14 if len(fr[3]) == 14 + hl + 64 else 0) + hl - 2:][:2] for fr in exp["frames"]]
    assert got[0] == got[2] == b"\xff\xff" and got[1] not in (b"\xff\xff", b"\0\0")


# ---- ring states ----

def test_ring_states(eng):
    """The last datagram ends at P exactly; a PADDING entry at the front, in the middle and trailing (stop EMPTY
    with meta_len 0 behind it); an empty metadata ring; mr + ml wrapping M; P = 4096 with M = 8 full."""
    tx = Tx()
    p = rnd(16, 20, 20, 30, 20, 30, 20, 9, 8, 7, 6, 5) + rnd(17, *[500] * 8)
    tx.add(p[0:2], P_=64, M=2, pr=24)                                   # 0: ends at 64: payload_read wraps to 0
    tx.add([pad(10), p[2]], P_=64, M=2, pr=54)                          # 1: padding at the front
    tx.add([p[3], pad(14), p[4]], P_=64, M=3, pr=30, mr=2)              # 2: padding in the middle, the ring full
    tx.add([p[5], pad(5)], P_=64, M=2, pr=3)                            # 3: trailing padding: gone, EMPTY
    tx.add([], P_=64, M=1)                                              # 4: nothing queued
    tx.add([], P_=64, M=1, pr=63, pl=0)                                 # 5: ... with a read index
    tx.add(p[6:11], P_=70, M=8, pr=33, mr=6)                            # 6: the metadata ring wraps
    tx.add(p[11:19], P_=4096, M=8, pr=96, mr=3)                         # 7: M = 8, full
    tx.add([pad(4)], P_=64, M=1, pr=60)                                 # 8: a padding alone
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "stop", "payload_read", "payload_len", "meta_read", "meta_len") == [
        (2, EMPTY, 0, 0, 0, 0), (1, EMPTY, 30, 0, 0, 0), (2, EMPTY, 30, 0, 2, 0), (1, EMPTY, 28, 0, 0, 0), (0, EMPTY, 0, 0, 0, 0),
        (0, EMPTY, 63, 0, 0, 0), (5, EMPTY, 68, 0, 3, 0), (8, EMPTY, 0, 0, 3, 0), (0, EMPTY, 0, 0, 0, 0)]
    fl = exp["tx"]["flags"][exp["tx_written"]].tolist()
    assert fl[:5] == [SENT, SENT, SENT | PADDED, SENT, SENT | PADDED]


# ---- stops ----

def test_stop_max(eng):
    """max_dgrams 1 and 256 with more queued, and with a PADDING entry right behind the last one, which stays."""
    tx = Tx()
    small = rnd(18, *[3 + i % 5 for i in range(257)])
    tx.add(small[:3], P_=64, M=4, maxd=1)
    tx.add([small[0], pad(64 - 3 - 10), small[1]], P_=64, M=4, pr=10, maxd=1)
    tx.add(small, P_=2048, M=300, mr=290, maxd=256)
    tx.add(small[:256] + [pad(2048 - 10 - sum(map(len, small[:256]))), small[256]], P_=2048, M=258, pr=10, mr=5, maxd=256)
    tx.add(small[:5], P_=64, M=8, maxd=5)  # exactly max_dgrams queued: MAX, not EMPTY
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "stop", "meta_len") == [(1, MAX, 2), (1, MAX, 2), (256, MAX, 1), (256, MAX, 2), (5, MAX, 0)]


@pytest.mark.parametrize("S", [0, 100])
def test_stop_nospace(eng, S):
    """NOSPACE at frame 0 and at frame k, through dst_cap and (S = 100) through a frame longer than the stride; a
    padding entry in front of the refused datagram is gone, the datagram stays."""
    tx = Tx(S)
    p = rnd(19, 20, 30, 59, 58, 10)
    tx.add([p[0]], P_=64, M=1, cap=14 + 28 + 20 - 1)                                   # 0: frame 0 through dst_cap
    tx.add([p[0], pad(14), p[1]], P_=64, M=3, pr=30, cap=(S or 62) + 72 - 1)           # 1: frame 1 through dst_cap
    tx.add([p[2]], P_=64, M=1, cap=500)                                                # 2: 101 bytes: fits only S = 0
    tx.add([p[3], p[4], pad(64), p[2]], P_=192, M=4, pr=60, cap=500)                   # 3: 100, 52, then 101 refused
    tx.add([p[0]], P_=64, M=1, cap=0)                                                  # 4: no room at all
    exp = _run(eng, tx)
    want = [(0, NOSPACE, 1, 0), (1, NOSPACE, 1, 0), (1, EMPTY, 0, 59) if S == 0 else (0, NOSPACE, 1, 0),
            (3, EMPTY, 0, 59) if S == 0 else (2, NOSPACE, 1, 0), (0, NOSPACE, 1, 0)]
    assert _outs(exp, "sent", "stop", "meta_len", "payload_read") == want


def test_stop_corrupt(eng):
    """CORRUPT by a bad kind, a bad family, padding after padding, and a size past the contiguous allocated bytes
    (past payload_len, and inside it but across the ring's end): the entries in front are sent, nothing more is
    dequeued, and the padding in front of a corrupt entry is gone."""
    tx = Tx()
    p = rnd(20, 20)[0]
    tx.add([p, raw(5, kind=0)], P_=64, M=4, pl=30)
    tx.add([p, raw(5, kind=3)], P_=64, M=4, pl=30)
    tx.add([p, raw(5, family=5)], P_=64, M=4, pl=30)
    tx.add([p, raw(5, family=0)], P_=64, M=4, pl=30)
    tx.add([p, pad(3), pad(3), p], P_=64, M=4, mr=3)
    tx.add([p, raw(11)], P_=64, M=2, pl=30)              # 10 bytes behind the first datagram, 11 asked
    tx.add([raw(20)], P_=64, M=1, pr=50, pl=30)          # 30 allocated, 14 of them before the ring's end
    tx.add([raw(0, kind=0)], P_=0, M=1)                  # P = 0
    tx.add([pad(70), raw(1)], P_=64, M=2, pr=60, pl=3)   # the padding's clamp: min(70, 3, 4) bytes go
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "stop", "meta_len", "payload_read", "payload_len") == [
        (1, CORRUPT, 1, 20, 10), (1, CORRUPT, 1, 20, 10), (1, CORRUPT, 1, 20, 10), (1, CORRUPT, 1, 20, 10),
        (1, CORRUPT, 2, 23, 23), (1, CORRUPT, 1, 20, 10), (0, CORRUPT, 1, 50, 30), (0, CORRUPT, 1, 0, 0), (0, CORRUPT, 1, 63, 0)]


@pytest.mark.parametrize("S", [0, 200])
def test_oversize(eng, S):
    """ip_len > ip_mtu for IPv4 and IPv6, first, middle and last of a group: dequeued, its entry carries ring_off
    and meta_idx, no frame is written and the next frame's place does not advance."""
    tx = Tx(S)
    a, b, big = rnd(21, 20, 30, 80)
    for fam, mtu in ((4, 107), (6, 127)):
        w = (lambda x: x) if fam == 4 else v6
        tx.add([w(big), w(a), w(b)], P_=256, M=3, pr=7, mtu=mtu)
        tx.add([w(a), w(big), w(b)], P_=256, M=3, pr=7, mtu=mtu, eth=None)
        tx.add([w(a), w(b), w(big)], P_=256, M=3, pr=7, mtu=mtu)
        tx.add([w(big), w(big)], P_=256, M=3, mtu=mtu)
        tx.add([w(a + b"x" * 59)], P_=256, M=1, mtu=mtu)  # ip_len == ip_mtu: sent
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "oversize", "stop", "payload_len") == [(2, 1, EMPTY, 0), (2, 1, EMPTY, 0), (2, 1, EMPTY, 0),
                                                                     (0, 2, EMPTY, 0), (1, 0, EMPTY, 0)] * 2
    t = exp["tx"][exp["tx_written"]]
    assert t["flags"][:6].tolist() == [OVER, SENT, SENT, SENT, OVER, SENT] and t["ip_len"][:3].tolist() == [0, 48, 58]
    assert t["frame_off"][:3].tolist() == [0, 0, S or 62] and t["ring_off"][:3].tolist() == [7, 87, 107]
    assert t["frame_off"][3:6].tolist() == [0, S or 48, S or 48]


def test_invalid_groups_among_valid_ones(eng):
    """Reserved bytes, unknown flag bits, max_dgrams 0 and 257, and every way a ring state leaves the contract: the
    group's d_out entry is zero, its frame area, its d_tx range keep their fill; its neighbours are served."""
    tx = Tx()
    p = rnd(22, 20, 30)

    def setf(name, val, idx=None):
        def f(socks, i):
            if idx is None:
                socks[i][name] = val
            else:
                socks[i][name][idx] = val
        return f

    good = lambda: tx.add(p, P_=64, M=2, pr=9)
    good()
    for over in (setf("reserved", 1, 0), setf("reserved", 0x80, 13), setf("flags", 3), setf("flags", 0x80), setf("max_dgrams", 0),
                 setf("max_dgrams", 257), setf("payload_len", 65), setf("meta_len", 3), setf("payload_read", 64),
                 setf("meta_read", 2)):
        tx.add(p, P_=64, M=2, pr=9, over=over)
        good()
    tx.add([], P_=0, M=0, over=setf("payload_read", 1))
    tx.add([], P_=0, M=0, over=setf("meta_read", 1))
    tx.add([], P_=0, M=0)  # valid: nothing to do
    exp = _run(eng, tx)
    assert exp["outs"]["valid"].tolist() == [1, 0] * 10 + [1, 0, 0, 1]
    assert exp["outs"]["sent"].tolist() == [2, 0] * 10 + [2, 0, 0, 0]


# ---- strides, grids, groups ----

@pytest.mark.parametrize("S", [0, 1536])
def test_strides_leave_the_gaps_alone(eng, S):
    """frame_stride 0 (back to back at any alignment) and 1536: the bytes between strided frames keep their fill."""
    tx = Tx(S)
    pay = rnd(23, 1472, 1, 700, 1473, 0, 1472)
    tx.add(pay, P_=6000, M=8, pr=111, mr=5)                          # 1473: ip_len 1501 > 1500, OVERSIZE
    tx.add([v6(x) for x in pay[:3]], P_=6000, M=8, pr=1, eth=None)   # 1472 over IPv6: ip_len 1520, OVERSIZE
    tx.add(pay[:2], P_=1500, M=2, mtu=1508)                          # 1514 bytes a frame
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "oversize", "stop") == [(5, 1, EMPTY), (2, 1, EMPTY), (2, 0, EMPTY)]
    assert int(exp["outs"][0]["bytes"]) == (5 * 1536 if S else 5 * 42 + 1472 * 2 + 701)


def test_grid_stride_over_3000_sockets(eng):
    """3000 one-datagram groups under a grid of 8 workgroups: each walks 375 sockets, its LDS reused."""
    tx = Tx()
    pay = rnd(24, *[1 + (i * 7) % 61 for i in range(3000)])
    for i, p in enumerate(pay):
        tx.add([p if i % 3 else v6(p)], P_=64, M=1 + i % 3, pr=i % 3, mr=i % (1 + i % 3), eth=ETH if i % 2 else None)
    exp = _run(eng, tx, blocks=8)
    assert int(exp["outs"]["sent"].sum()) == 3000


def test_256_datagrams_in_one_group(eng):
    """A group of 256 datagrams: every thread's d_tx entry, 64 frames a wave."""
    tx = Tx()
    pay = rnd(25, *[(i * 37) % 300 for i in range(256)])
    tx.add([p if i % 2 else v6(p) for i, p in enumerate(pay)], P_=40000, M=256, pr=39, mr=255)
    exp = _run(eng, tx)
    assert _outs(exp, "sent", "stop") == [(256, MAX)]


# ---- streams ----

def _mixed(seed, S=0):
    tx = Tx(S)
    p = rnd(seed, 100, 200, 300, 17, 1472)
    tx.add(p, P_=3000, M=8, pr=800)
    tx.add([v6(x) for x in p[:4]], P_=1000, M=4, eth=None)
    return tx


def test_graph_capture_and_replay_on_a_side_stream(eng):
    """The call is captured into a graph on a side stream (no allocation, no event, no host synchronisation) and the
    replay does the work."""
    exp = _run(eng, _mixed(31), graph=True)
    assert _outs(exp, "sent") == [(5,), (4,)]


def test_stream_and_empty_call(eng):
    """A non-default stream; n_groups == 0 launches nothing and writes nothing."""
    _run(eng, _mixed(32), stream=torch.cuda.Stream())
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    eng.verify(d, E.Batch.fixed(4, 64, 64, E.KIND_IP))
    dst = torch.full((64,), D.SENTINEL, dtype=torch.uint8, device="cuda")
    txe = torch.full((4, 16), PRE, dtype=torch.uint8, device="cuda")
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    _, out = eng.udp_dequeue_emit(d, empty, d, dst, 0, tx=txe)
    assert eng.last_launch()["kernel"] != "udptx_kernel"
    assert bool((dst == D.SENTINEL).all()) and bool((txe == PRE).all()) and out.numel() == 0


def test_two_streams_on_one_context(eng):
    """Two calls in flight on two streams of one context: no scratch, no event, nothing shared."""
    txa, txb = _mixed(33), _mixed(34, S=1600)
    ba, ta = _launch(eng, txa)
    bb, tb = _launch(eng, txb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (sa, sb):
        s.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        with torch.cuda.stream(sa):
            ta["call"](sa)
        with torch.cuda.stream(sb):
            tb["call"](sb)
    sa.synchronize(), sb.synchronize()
    _check(txa, ba, ta)
    _check(txb, bb, tb)


# ---- the pair with verify_udp_enqueue ----

def _rx_socket(eng, frames_dev, offs, lens, port, P_, M):
    """verify_udp_enqueue of the frames at offs / lens of frames_dev into one fresh socket bound to `port`:
    (rx entries, out entry, metadata entries, ring bytes, ring tensor, metadata tensor)."""
    n = len(offs)
    batch = E.Batch.from_records(np.asarray(offs, np.uint64), np.asarray(lens, np.uint32), np.full(n, E.KIND_ETH, np.uint8), "cuda:0")
    groups = torch.from_numpy(E.make_groups([0], [n]).view(np.uint8).copy()).cuda()
    socks = torch.from_numpy(E.make_udpsocks([0], 0, P_, 0, 0, M, 0, 0, port).view(np.uint8).copy()).cuda()
    ring = torch.full((P_,), D.SENTINEL, dtype=torch.uint8, device="cuda")
    md = torch.full((M, 48), PRE, dtype=torch.uint8, device="cuda")
    before = frames_dev.clone()
    st, rx, out = eng.verify_udp_enqueue(frames_dev, batch, groups, ring, socks, md)
    assert torch.equal(frames_dev, before), "verify_udp_enqueue's batch buffer is only read"
    assert bool((st & E.ST_ACCEPT).bool().all()), "a frame of udp_dequeue_emit fails verify"
    return (rx.cpu().numpy().reshape(-1).view(E.UDPRX_DTYPE), out.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE)[0],
            md.cpu().numpy().reshape(-1).view(E.UDPMETA_DTYPE), ring.cpu().numpy(), ring, md)


def test_round_trip_through_verify_udp_enqueue(eng):
    """The frames go back through verify_udp_enqueue into a second socket: every record is ENQUEUED, the payloads
    are identical, and each metadata entry is the sent one with the roles of the two addresses and ports swapped."""
    tx = Tx()
    pay = rnd(41, 100, 0, 1472, 33, 700)
    ents = [dict(p=p, fam=4 if j % 2 else 6, dport=6000) for j, p in enumerate(pay)]
    tx.add(ents, P_=3000, M=8, pr=500, port=4321, mtu=1520)
    built, t = _launch(eng, tx)
    t["call"](None)
    exp = _check(tx, built, t)
    offs = [f[2] for f in exp["frames"]]
    lens = [len(f[3]) for f in exp["frames"]]
    rx, out, md, ring, _, _ = _rx_socket(eng, t["dst"], offs, lens, 6000, 4096, 8)
    assert rx["flags"].tolist() == [E.URX_UDP | E.URX_ENQUEUED] * 5 and int(out["enqueued"]) == 5
    sent_meta = built[2]
    for j, p in enumerate(pay):
        assert bytes(ring[int(rx["ring_off"][j]):int(rx["ring_off"][j]) + len(p)]) == p
        got, was = md[int(rx["meta_idx"][j])], sent_meta[1 + j]
        assert (int(got["size"]), int(got["family"]), int(got["kind"])) == (len(p), int(was["family"]), E.UMETA_PACKET)
        assert int(got["src_port"]) == 4321 and int(was["src_port"]) == 6000
        assert bytes(got["remote_addr"]) == bytes(was["local_addr"]) and bytes(got["local_addr"]) == bytes(was["remote_addr"])


def test_echo_a_receive_ring_answered_unchanged(eng):
    """verify_udp_enqueue's own d_meta and ring are given to this call unchanged: each reply frame goes back to its
    sender, from the address and port it was sent to, with the same payload."""
    import oracle

    pay = rnd(42, 50, 300, 0, 1200, 77)
    recs = []
    for j, p in enumerate(pay):
        u = P.udp(3000 + j, 7, p)
        src4, src6 = bytes([10, 9, j, 1]), bytes([0xFD, j] * 8)
        recs.append(P.eth(P.ipv4(src4, B4, 17, u) if j % 2 else P.ipv6(src6, B6, 17, u), 0x0800 if j % 2 else 0x86DD))
    buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(2))
    oracle.batch_emit(buf, E.make_descriptors(offs, lens, np.full(5, E.KIND_ETH, np.uint8)), 5)
    rx, out, md, ring, ring_dev, md_dev = _rx_socket(eng, torch.from_numpy(buf).cuda(), offs, lens, 7, 2048, 8)
    assert int(out["enqueued"]) == 5
    # the reply: the receive ring as the transmit ring, the state verify_udp_enqueue left, the socket's own port
    socks = E.make_udptxsocks([0], 0, 0, 0, 2048, out["payload_read"], out["payload_len"], 8, out["meta_read"], out["meta_len"],
                              8192, 256, 7, 1500, eth=ETH)
    dst = torch.full((8192,), D.SENTINEL, dtype=torch.uint8, device="cuda")
    socks_dev = torch.from_numpy(socks.view(np.uint8).copy()).cuda()
    txe, txo = eng.udp_dequeue_emit(ring_dev, socks_dev, md_dev, dst, 0, n_tx=5)
    assert eng.last_launch()["kernel"] == "udptx_kernel"
    exp = D.expected(ring, socks, md, BOTH, 0, 8192, 5)
    assert np.array_equal(dst.cpu().numpy(), exp["arena"])
    assert np.array_equal(ring_dev.cpu().numpy(), ring), "d_src is only read"
    assert np.array_equal(md_dev.cpu().numpy().reshape(-1), md.view(np.uint8)), "d_meta is only read"
    assert np.array_equal(socks_dev.cpu().numpy(), socks.view(np.uint8)), "d_socks is only read"
    assert np.array_equal(txe.cpu().numpy().reshape(-1).view(E.UDPTX_DTYPE), exp["tx"])
    o = txo.cpu().numpy().reshape(-1).view(E.UDPTXOUT_DTYPE)[0]
    assert (int(o["sent"]), int(o["stop"]), int(o["meta_len"]), int(o["payload_len"])) == (5, EMPTY, 0, 0)
    for j, (_, _, _, f) in enumerate(exp["frames"]):
        req = recs[j]
        if j % 2:
            assert f[14 + 12:14 + 16] == req[14 + 16:14 + 20] and f[14 + 16:14 + 20] == req[14 + 12:14 + 16]
            l4 = 34
        else:
            assert f[14 + 8:14 + 24] == req[14 + 24:14 + 40] and f[14 + 24:14 + 40] == req[14 + 8:14 + 24]
            l4 = 54
        assert f[l4:l4 + 2] == req[l4 + 2:l4 + 4] and f[l4 + 2:l4 + 4] == req[l4:l4 + 2] and f[l4 + 8:] == pay[j]
