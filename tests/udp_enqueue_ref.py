"""Pure-Python model of smol_csum_batch_verify_udp_enqueue's contract (include/smolcsum.h), for the CPU tests
(tests/test_udp_enqueue_cpu.py, tests/test_pktbuf_rule_cpu.py) and the GPU tests (tests/test_gpu_udp_enqueue*.py),
which take their expected record entries, group entries, metadata entries and ring bytes from `expected`.

`PacketBuffer` restates the reference's PacketBuffer (src/storage/packet_buffer.rs:80-118, 169-216) over its two
RingBuffers (src/storage/ring_buffer.rs:76-105, 181-268) with real modulo arithmetic: enqueue, and dequeue, which
skips padding entries, so that the reference's own tests replay against it (tests/golden/packet_buffer_kat.json).

No checksum is computed here: the status bytes are an input (oracle.batch_verify's)."""
import numpy as np

from smoltcp_amd import engine as E
from tests.test_verify_copy_cpu import expected_span

SENTINEL = 0xA5
OK, FULL, PADDED = 1, 2, 4  # PktBufStep.res of smoltcp_amd/csrc/csum_pktbuf.h


class PacketBuffer:
    """The two rings' state (P, M fixed; pr, pl, mr, ml) and, for the replay of the reference's tests, the
    metadata entries ((size, header) with header None for padding) and the payload storage."""

    def __init__(self, P, M, pr=0, pl=0, mr=0, ml=0):
        self.P, self.M, self.pr, self.pl, self.mr, self.ml = P, M, pr, pl, mr, ml
        self.meta = [None] * M
        self.store = bytearray(P)

    def state(self):
        return self.pr, self.pl, self.mr, self.ml

    def valid(self):
        return self.pl <= self.P and self.ml <= self.M and (self.pr < self.P if self.P else self.pr == 0) and \
            (self.mr < self.M if self.M else self.mr == 0)

    def enqueue(self, size, header=()):
        """PacketBuffer::enqueue.  Returns (res, ring_off, meta_idx, pad_idx, pad_size): res is OK or FULL, with
        PADDED when a padding entry was enqueued (which stays when the packet entry then finds no room)."""
        P, M = self.P, self.M
        if P < size or self.ml == M:
            return FULL, 0, 0, 0, 0
        if self.pl == 0:
            self.pr = 0
        window = P - self.pl
        widx = (self.pr + self.pl) % P if P else 0
        contig = min(window, P - widx)
        res = pad_idx = pad_size = 0
        if window < size:
            return FULL, 0, 0, 0, 0
        if contig < size:
            if window - contig < size:
                return FULL, 0, 0, 0, 0
            res, pad_idx, pad_size = PADDED, (self.mr + self.ml) % M, contig
            self.meta[pad_idx] = (contig, None)
            self.ml += 1
            self.pl += contig
        if self.ml == M:
            return res | FULL, 0, 0, pad_idx, pad_size
        meta_idx = (self.mr + self.ml) % M
        self.meta[meta_idx] = (size, header)
        self.ml += 1
        ring_off = (self.pr + self.pl) % P if P else 0
        self.pl += size
        return res | OK, ring_off, meta_idx, pad_idx, pad_size

    def _dequeue_payload(self, size):
        """RingBuffer::dequeue_many: at most the contiguous allocated bytes."""
        size = min(size, self.pl, self.P - self.pr)
        at = self.pr
        self.pr = (self.pr + size) % self.P if self.P else 0
        self.pl -= size
        return at, size

    def dequeue_padding(self):
        """PacketBuffer::dequeue_padding: a padding entry at the front is dequeued with its bytes."""
        if self.ml and self.meta[self.mr][1] is None:
            self._dequeue_payload(self.meta[self.mr][0])
            self.mr, self.ml = (self.mr + 1) % self.M, self.ml - 1

    def peek(self):
        """PacketBuffer::peek: the front packet's payload without removing it, or None for Err(Empty)."""
        self.dequeue_padding()
        if self.ml == 0:
            return None
        return bytes(self.store[self.pr:self.pr + self.meta[self.mr][0]])

    def write(self, ring_off, data):
        """copy_from_slice into the slice enqueue returned."""
        self.store[ring_off:ring_off + len(data)] = data

    def dequeue(self):
        """PacketBuffer::dequeue: padding is skipped.  Returns the payload bytes, or None for Err(Empty)."""
        self.dequeue_padding()
        if self.ml == 0:
            return None
        size = self.meta[self.mr][0]
        self.mr, self.ml = (self.mr + 1) % self.M, self.ml - 1
        at, got = self._dequeue_payload(size)
        assert got == size
        return bytes(self.store[at:at + size])


def group_valid(first, count, reserved, n, sock) -> bool:
    if first >= n or count == 0 or count > E.MAX_SOCKET_DGRAMS or count > n - first or reserved != 0:
        return False
    if np.any(sock["reserved"]):
        return False
    return PacketBuffer(int(sock["payload_cap"]), int(sock["meta_cap"]), int(sock["payload_read"]), int(sock["payload_len"]),
                        int(sock["meta_read"]), int(sock["meta_len"])).valid()


def udp_datagram(rec: bytes, kind: int, flags: int = 0):
    """(off, size, src_port, dst_port, family, src_addr, dst_addr) of a record with a UDP payload span under
    verify_copy's span rule, else None."""
    span = expected_span(rec, kind, flags)
    if span is None:
        return None
    ip = 14 if kind == E.KIND_ETH else 0
    if rec[ip] >> 4 == 4:
        proto, l4, fam, src, dst = rec[ip + 9], ip + (rec[ip] & 15) * 4, 4, rec[ip + 12:ip + 16], rec[ip + 16:ip + 20]
    else:
        proto, l4, fam, src, dst = rec[ip + 6], ip + 40, 6, rec[ip + 8:ip + 24], rec[ip + 24:ip + 40]
        if proto == 0:
            proto, l4 = rec[l4], l4 + (rec[l4 + 1] + 1) * 8
    if proto != 17:
        return None
    assert span[0] == l4 + 8
    return span[0], span[1], rec[l4] << 8 | rec[l4 + 1], rec[l4 + 2] << 8 | rec[l4 + 3], fam, bytes(src), bytes(dst)


def _layout(sock, sizes):
    """The rule over `sizes` (None: the record does not take part) from the socket's state: (steps, buffer)."""
    pb = PacketBuffer(int(sock["payload_cap"]), int(sock["meta_cap"]), int(sock["payload_read"]), int(sock["payload_len"]),
                      int(sock["meta_read"]), int(sock["meta_len"]))
    return [None if s is None else pb.enqueue(s) for s in sizes], pb


def enqueue_group(items, first, sock, arena, acc_mask, spec_arena, spec_mask, meta):
    """One valid group.  items[j]: None (no candidate) or (off, payload, src_port, family, src, dst, accept).
    Stores the accepted layout into `arena` / acc_mask, the speculative one into spec_arena / spec_mask, and the metadata
    entries into `meta` (a dict: index in d_meta -> entry).  Returns (rx, out)."""
    rx = np.zeros(len(items), E.UDPRX_DTYPE)
    base, mfirst = int(sock["dst_offset"]), int(sock["meta_first"])
    spec, _ = _layout(sock, [None if it is None else len(it[1]) for it in items])
    acc, pb = _layout(sock, [None if it is None or not it[6] else len(it[1]) for it in items])
    out = np.zeros(1, E.UDPSOCKOUT_DTYPE)[0]
    for j, it in enumerate(items):
        if it is None:
            continue
        off, payload, sport, fam, src, dst, _ = it
        data = np.frombuffer(payload, np.uint8)
        if spec[j][0] & OK:
            a = base + spec[j][1]
            spec_arena[a:a + len(payload)] = data
            spec_mask[a:a + len(payload)] = True
        fl, at, mi = E.URX_UDP, 0, 0
        if acc[j] is not None:
            res, at, mi, pad_idx, pad_size = acc[j]
            if res & PADDED:
                fl |= E.URX_PADDED
                e = np.zeros(1, E.UDPMETA_DTYPE)[0]
                e["size"], e["kind"] = pad_size, E.UMETA_PADDING
                meta[mfirst + pad_idx] = e
            if res & OK:
                fl |= E.URX_ENQUEUED
                out["enqueued"] += 1
                arena[base + at:base + at + len(payload)] = data
                acc_mask[base + at:base + at + len(payload)] = True
                e = np.zeros(1, E.UDPMETA_DTYPE)[0]
                e["size"], e["record"], e["src_port"], e["family"], e["kind"] = len(payload), first + j, sport, fam, E.UMETA_PACKET
                e["remote_addr"][:len(src)] = np.frombuffer(src, np.uint8)
                e["local_addr"][:len(dst)] = np.frombuffer(dst, np.uint8)
                meta[mfirst + mi] = e
                if len(payload) > 0 and not (spec[j][0] & OK and spec[j][1] == at):
                    fl |= E.URX_RESTORED
                    out["restored"] += 1
            else:
                fl |= E.URX_FULL
                out["full"] += 1
                at = mi = 0
        rx[j] = (at, len(payload), mi, off & 0xFFFF, fl, 0)
    out["payload_read"], out["payload_len"], out["meta_read"], out["meta_len"] = pb.state()
    out["valid"] = 1
    return rx, out


def expected(recs, kinds, flags, groups, socks, status, arena_size: int, meta_size: int, sentinel: int = SENTINEL):
    """What the call leaves, as a dict:
      rx, outs: the record and group entries (rx of records the call does not write stay zero);
      written[i]: record i belongs to a valid group (its status byte and entry are written);
      arena: the sentinel-filled arena with every ENQUEUED record's payload at its place;
      spec_arena, spec_only: the speculative layout's bytes, and the mask of the bytes that lie in a speculative
        range and in no accepted one (there the arena may hold the sentinel or spec_arena's byte);
      meta, meta_written: d_meta (zero where not written) and the mask of the entries written."""
    n = len(recs)
    rx = np.zeros(n, E.UDPRX_DTYPE)
    outs = np.zeros(len(groups), E.UDPSOCKOUT_DTYPE)
    arena = np.full(arena_size, sentinel, np.uint8)
    spec_arena = np.full(arena_size, sentinel, np.uint8)
    spec_mask, acc_mask = np.zeros(arena_size, bool), np.zeros(arena_size, bool)
    written = np.zeros(n, bool)
    entries = {}
    for gi, (first, count, reserved) in enumerate(groups):
        first, count = int(first), int(count)
        if not group_valid(first, count, int(reserved), n, socks[gi]):
            continue
        port = int(socks[gi]["port"])
        items = []
        for i in range(first, first + count):
            t = udp_datagram(recs[i], int(kinds[i]), int(flags[i]))
            if t is None or t[3] != port:
                items.append(None)
            else:
                items.append((t[0], recs[i][t[0]:t[0] + t[1]], t[2], t[4], t[5], t[6], bool(int(status[i]) & E.ST_ACCEPT)))
        rx[first:first + count], outs[gi] = enqueue_group(items, first, socks[gi], arena, acc_mask, spec_arena, spec_mask, entries)
        written[first:first + count] = True
    meta = np.zeros(meta_size, E.UDPMETA_DTYPE)
    meta_written = np.zeros(meta_size, bool)
    for i, e in entries.items():
        meta[i], meta_written[i] = e, True
    return dict(rx=rx, outs=outs, written=written, arena=arena, spec_arena=spec_arena,
                spec_only=spec_mask & ~acc_mask,
                meta=meta, meta_written=meta_written)


def check_arena(got, exp, sentinel: int = SENTINEL):
    """The three byte classes of the contract.  Returns the indices of the bytes that break it."""
    ok = np.where(exp["spec_only"], (got == sentinel) | (got == exp["spec_arena"]), got == exp["arena"])
    return np.nonzero(~ok)[0]
