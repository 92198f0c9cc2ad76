"""Pure-Python model of smol_csum_batch_udp_dequeue_emit's contract (include/smolcsum.h), for the CPU tests
(tests/test_udp_dequeue_cpu.py, tests/test_pktbuf_dequeue_rule_cpu.py) and the GPU tests
(tests/test_gpu_udp_dequeue*.py), which take their expected d_tx entries, group entries and destination arena from
`expected`.

The rule (`front`, `take`) is PacketBuffer::dequeue_with (src/storage/packet_buffer.rs:169-204) in its two halves,
over tests/udp_enqueue_ref.py's PacketBuffer: its state, its dequeue_padding and its dequeue_many clamp, imported
and not edited.  The frames are built with tests/pktgen.py and their checksums filled by oracle.batch_emit under
the call's caps: nothing here computes a checksum."""
import numpy as np

import oracle
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests.udp_enqueue_ref import PacketBuffer

SENTINEL = 0xA5
OK, PADDED, EMPTY, CORRUPT = 1, 4, 8, 16  # PktBufFront.res of smoltcp_amd/csrc/csum_pktbuf.h
PACKET, PADDING = E.UMETA_PACKET, E.UMETA_PADDING


def kat_kind(header):
    """(kind, family) of a PacketBuffer entry header as udp_enqueue_ref.PacketBuffer.enqueue stores it: None
    is padding, anything else a packet (the reference's tests carry no address family: 4)."""
    return (PADDING, 0) if header is None else (PACKET, 4)


def meta_kind(header):
    """(kind, family) of an entry whose header is its smol_csum_udpmeta_t record; padding is stored as None."""
    return (PADDING, 0) if header is None else (int(header["kind"]), int(header["family"]))


def front(pb: PacketBuffer, kind_of=kat_kind):
    """pktbuf_front: dequeue_padding, then the front entry.  Returns (res, ring_off, meta_idx, size, family)."""
    res = 0
    if pb.ml and kind_of(pb.meta[pb.mr][1])[0] == PADDING:
        # dequeue_padding as PacketBuffer has it, for an entry this model calls padding by its kind
        pb._dequeue_payload(pb.meta[pb.mr][0])
        pb.mr, pb.ml = (pb.mr + 1) % pb.M, pb.ml - 1
        res |= PADDED
    if pb.ml == 0:
        return res | EMPTY, 0, 0, 0, 0
    size, header = pb.meta[pb.mr]
    kind, fam = kind_of(header)
    if kind != PACKET or fam not in (4, 6) or size > min(pb.pl, pb.P - pb.pr):
        return res | CORRUPT, 0, 0, 0, 0
    return res | OK, pb.pr, pb.mr, size, fam


def take(pb: PacketBuffer, size):
    """pktbuf_take: the closure returned Ok."""
    at, got = pb._dequeue_payload(size)
    assert got == size
    pb.mr, pb.ml = (pb.mr + 1) % pb.M, pb.ml - 1
    return at


def dequeue(pb: PacketBuffer, kind_of=kat_kind):
    """pktbuf_dequeue: PacketBuffer::dequeue.  Returns front's tuple."""
    r = front(pb, kind_of)
    if r[0] & OK:
        take(pb, r[3])
    return r


def group_valid(sock) -> bool:
    if np.any(sock["reserved"]) or int(sock["flags"]) & ~E.UTXS_ETH or not 1 <= int(sock["max_dgrams"]) <= E.MAX_SOCKET_DGRAMS:
        return False
    return PacketBuffer(int(sock["payload_cap"]), int(sock["meta_cap"]), int(sock["payload_read"]), int(sock["payload_len"]),
                        int(sock["meta_read"]), int(sock["meta_len"])).valid()


def load(sock, meta) -> PacketBuffer:
    """The socket's PacketBuffer with its metadata ring's entries out of d_meta (a padding entry's header is None,
    every other entry's its record)."""
    pb = PacketBuffer(int(sock["payload_cap"]), int(sock["meta_cap"]), int(sock["payload_read"]), int(sock["payload_len"]),
                      int(sock["meta_read"]), int(sock["meta_len"]))
    first = int(sock["meta_first"])
    for j in range(pb.ml):
        i = (pb.mr + j) % pb.M
        e = meta[first + i]
        pb.meta[i] = (int(e["size"]), None if int(e["kind"]) == PADDING else e)
    return pb


def walk(sock, meta, frame_stride):
    """The dequeue rule and the placement over one valid group.  Returns (tx rows, out row, sends): tx rows as
    (frame_off, ring_off, meta_idx, ip_len, flags), sends as (frame_off, ring_off, size, entry) for the SENT ones."""
    pb = load(sock, meta)
    io = 14 if int(sock["flags"]) & E.UTXS_ETH else 0
    mtu, cap, maxd, S = int(sock["ip_mtu"]), int(sock["dst_cap"]), int(sock["max_dgrams"]), int(frame_stride)
    tx, sends = [], []
    sent = over = nxt = 0
    while True:
        if len(tx) == maxd:
            stop = E.UTX_STOP_MAX
            break
        res, ring_off, meta_idx, size, fam = front(pb, meta_kind)
        if res & EMPTY:
            stop = E.UTX_STOP_EMPTY
            break
        if res & CORRUPT:
            stop = E.UTX_STOP_CORRUPT
            break
        ip_len = (20 if fam == 4 else 40) + 8 + size
        fl = E.UTX_PADDED if res & PADDED else 0
        if ip_len > mtu:
            fl |= E.UTX_OVERSIZE
            over += 1
            row = (min(nxt, 0xFFFFFFFF), ring_off, meta_idx, 0, fl)
        else:
            if nxt + io + ip_len > cap or (S and io + ip_len > S):
                stop = E.UTX_STOP_NOSPACE
                break
            fl |= E.UTX_SENT
            row = (nxt, ring_off, meta_idx, ip_len, fl)
            sends.append((nxt, ring_off, size, pb.meta[meta_idx][1]))
        take(pb, size)
        tx.append(row)
        if fl & E.UTX_SENT:
            sent += 1
            nxt = sent * S if S else nxt + io + ip_len
    out = np.zeros(1, E.UDPTXOUT_DTYPE)[0]
    out["payload_read"], out["payload_len"], out["meta_read"], out["meta_len"] = pb.state()
    out["sent"], out["oversize"], out["bytes"], out["stop"], out["valid"] = sent, over, min(nxt, 0xFFFFFFFF), stop, 1
    return tx, out, sends


def header(sock, entry, size) -> bytes:
    """The frame's head as the host builds it, checksums 0 (oracle.batch_emit fills them)."""
    fam = int(entry["family"])
    n = 4 if fam == 4 else 16
    src, dst = bytes(entry["local_addr"][:n]), bytes(entry["remote_addr"][:n])
    u = P.udp(int(sock["port"]), int(entry["src_port"]), b"")[:4] + P.be16(8 + size) + P.be16(0)
    hop = int(sock["hop_limit"])
    if fam == 4:
        ip = P.ipv4(src, dst, 17, u, ttl=hop, flags_frag=0x4000, ident=0, total_len=20 + 8 + size)
    else:
        ip = P.ipv6(src, dst, 17, u, hop=hop, payload_len=8 + size)
    if int(sock["flags"]) & E.UTXS_ETH:
        return bytes(sock["eth_dst"]) + bytes(sock["eth_src"]) + P.be16(0x0800 if fam == 4 else 0x86DD) + ip
    return ip


def expected(src, socks, meta, caps, frame_stride, dst_size, tx_size, sentinel=SENTINEL):
    """What the call leaves, as a dict:
      tx, tx_written: d_tx (zero where not written) and the mask of the entries written;
      outs: the group entries (all zero for an invalid group);
      arena: the sentinel-filled destination with every SENT frame at its place;
      frames: [(group, k, absolute offset in d_dst, frame bytes)] of the SENT frames."""
    tx = np.zeros(tx_size, E.UDPTX_DTYPE)
    tx_written = np.zeros(tx_size, bool)
    outs = np.zeros(len(socks), E.UDPTXOUT_DTYPE)
    arena = np.full(dst_size, sentinel, np.uint8)
    recs, where = [], []
    for gi, sock in enumerate(socks):
        if not group_valid(sock):
            continue
        rows, outs[gi], sends = walk(sock, meta, frame_stride)
        t0 = int(sock["tx_first"])
        for k, row in enumerate(rows):
            tx[t0 + k] = row + (0,)
            tx_written[t0 + k] = True
        s0, d0 = int(sock["src_offset"]), int(sock["dst_offset"])
        sent_k = [k for k, row in enumerate(rows) if row[4] & E.UTX_SENT]
        for k, (foff, ring_off, size, entry) in zip(sent_k, sends):
            recs.append(header(sock, entry, size) + bytes(src[s0 + ring_off:s0 + ring_off + size]))
            where.append((gi, k, d0 + foff, bool(int(sock["flags"]) & E.UTXS_ETH)))
    frames = []
    if recs:
        buf, offs, lens = P.pack(recs)
        kinds = np.array([E.KIND_ETH if w[3] else E.KIND_IP for w in where], np.uint8)
        st = oracle.batch_emit(buf, E.make_descriptors(offs, lens, kinds), len(recs), caps=tuple(caps))
        assert not np.any(st & (E.ST_MALFORMED | E.ST_UNSUPPORTED)), "the model built a frame emit does not take"
        for (gi, k, at, _), o, n in zip(where, offs, lens):
            f = buf[int(o):int(o) + int(n)]
            assert at + int(n) <= dst_size and np.all(arena[at:at + int(n)] == sentinel), "frames overlap or leave the arena"
            arena[at:at + int(n)] = f
            frames.append((gi, k, at, bytes(f)))
    return dict(tx=tx, tx_written=tx_written, outs=outs, arena=arena, frames=frames)
