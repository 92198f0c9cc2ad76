"""numpy restatement of smol_csum_batch_verify_tcp_assemble's contract (include/smolcsum.h), for the CPU
tests (tests/test_tcp_assemble_cpu.py, tests/test_tcpwin_rule_cpu.py) and the GPU tests
(tests/test_gpu_tcp_assemble.py), which take their expected segment entries, flow entries and ring bytes
from `expected`.

No checksum is computed here: which records verify accepts is an input (`accept`, from the status bytes
of oracle.batch_verify).  `sequential_socket` restates TcpSocket::process' receive path
(src/socket/tcp.rs:1705-1783, 2205-2241) fed one segment at a time: the moving window_start, the trim,
RingBuffer::write_unallocated and an Assembler (src/storage/assembler.rs) with a settable hole limit."""
import numpy as np

from smoltcp_amd import engine as E
from tests.test_verify_copy_cpu import expected_span

SENTINEL = 0xA5
MAX_FLOW_SEGMENTS = 256
SEG_TCP, SEG_IN_WINDOW, SEG_COPIED, SEG_REDELIVERED = 0x01, 0x02, 0x04, 0x08
TCPWIN_DTYPE = np.dtype([("dst_offset", "<u8"), ("ring_len", "<u4"), ("ring_pos", "<u4"), ("window_start", "<u4"),
                         ("window_len", "<u4"), ("reserved", "<u4", (2,))])
TCPSEG_DTYPE = np.dtype([("seq", "<u4"), ("win_off", "<u4"), ("len", "<u4"), ("off", "<u2"), ("flags", "u1"), ("reserved", "u1")])
TCPFLOW_DTYPE = np.dtype([("contig_len", "<u4"), ("counted", "<u4"), ("redelivered", "<u4"), ("valid", "u1"),
                          ("reserved", "u1", (3,))])


def seq_diff(seq, window_start):
    """TcpSeqNumber's subtraction: (int32)(seq - window_start), elementwise (int64 arrays)."""
    s = (np.asarray(seq, np.int64) - np.asarray(window_start, np.int64)) & 0xFFFFFFFF
    return np.where(s >= 1 << 31, s - (1 << 32), s)


def window_rule(seq, p, window_start, window_len):
    """The window rule, elementwise over arrays (or scalars): (in_window, win_off, len, trim) as int64
    arrays.  segment_in_window (tcp.rs:1719-1769) and the trim (:1771-1783)."""
    s = seq_diff(seq, window_start)
    p, W = np.asarray(p, np.int64), np.asarray(window_len, np.int64)
    e = s + p
    inside = (0 <= s) & (s < W)
    empty = (s != -1) & np.where(W == 0, s == 0, inside)
    data = (W != 0) & (inside | ((0 < e) & (e <= W)))
    inw = np.where(p == 0, empty, data)
    lo, hi = np.maximum(s, 0), np.minimum(e, W)
    z = np.zeros_like(lo)
    return inw.astype(np.int64), np.where(inw, lo, z), np.where(inw, hi - lo, z), np.where(inw, np.maximum(-s, 0), z)


def ring_split(win_off, length, ring_pos, ring_len):
    """The two pieces of window range [win_off, win_off + length) in the ring (write_unallocated's two
    get_unallocated slices): (pos0, len0, len1), len1 bytes at ring index 0.  Elementwise."""
    win_off, length = np.asarray(win_off, np.int64), np.asarray(length, np.int64)
    ring_pos, ring_len = np.asarray(ring_pos, np.int64), np.asarray(ring_len, np.int64)
    ok = (length > 0) & (ring_len > 0)
    pos0 = np.where(ok, (ring_pos + win_off) % np.where(ring_len > 0, ring_len, 1), 0)
    len0 = np.where(ok, np.minimum(length, ring_len - pos0), 0)
    return pos0, len0, np.where(ok, length - len0, 0)


def group_valid(first: int, count: int, reserved: int, n: int, win) -> bool:
    if first >= n or count == 0 or count > MAX_FLOW_SEGMENTS or count > n - first or reserved != 0:
        return False
    rl, rp = int(win["ring_len"]), int(win["ring_pos"])
    if win["reserved"].any() or int(win["window_len"]) > rl:
        return False
    return rp < rl if rl else rp == 0


def tcp_segment(rec: bytes, kind: int, flags: int = 0):
    """(off, p, seq, syn_or_rst) of a record with a TCP payload span under verify_copy's span rule, else
    None."""
    span = expected_span(rec, kind, flags)
    if span is None:
        return None
    ip = 14 if kind == E.KIND_ETH else 0
    if rec[ip] >> 4 == 4:
        proto, l4 = rec[ip + 9], ip + (rec[ip] & 15) * 4
    else:
        proto, l4 = rec[ip + 6], ip + 40
        if proto == 0:
            proto, l4 = rec[l4], l4 + (rec[l4 + 1] + 1) * 8
    if proto != 6:
        return None
    return span[0], span[1], int.from_bytes(rec[l4 + 4:l4 + 8], "big"), bool(rec[l4 + 13] & 0x06)


def contig_of(ranges) -> int:
    """The largest c such that the union of the [start, end) ranges covers [0, c)."""
    c = 0
    for a, b in sorted(ranges):
        if a > c:
            break
        c = max(c, b)
    return c


def assemble_group(items, win, arena):
    """One valid group.  items[j]: None (no TCP span) or (seq, payload, off, syn_or_rst, accept).  Stores
    into `arena` (None: no stores) the records that are not counted first, then the counted ones in arrival
    order.  Returns (segs, flow)."""
    segs = np.zeros(len(items), TCPSEG_DTYPE)
    ws, W = int(win["window_start"]), int(win["window_len"])
    rp, rl, base = int(win["ring_pos"]), int(win["ring_len"]), int(win["dst_offset"])
    todo = []  # (counted, j, win_off, bytes)
    for j, it in enumerate(items):
        if it is None:
            continue
        seq, payload, off, syn_rst, accept = it
        inw, wo, ln, trim = (int(x) for x in window_rule(seq, len(payload), ws, W))
        fl = SEG_TCP | (SEG_IN_WINDOW if inw else 0) | (SEG_COPIED if inw and not syn_rst else 0)
        segs[j] = (seq, wo, ln, off, fl, 0)
        if fl & SEG_COPIED and ln > 0:
            todo.append((bool(accept), j, wo, bytes(payload[trim:trim + ln])))
    lost = [(wo, wo + len(b)) for c, _, wo, b in todo if not c]
    redel = 0
    for c, j, wo, b in todo:
        if c and any(a < wo + len(b) and wo < e for a, e in lost):
            segs[j]["flags"] |= SEG_REDELIVERED
            redel += 1
    if arena is not None:
        for c, j, wo, b in sorted(todo, key=lambda t: (t[0], t[1])):
            pos0, len0, len1 = (int(x) for x in ring_split(wo, len(b), rp, rl))
            arena[base + pos0:base + pos0 + len0] = np.frombuffer(b[:len0], np.uint8)
            arena[base:base + len1] = np.frombuffer(b[len0:], np.uint8)
    flow = np.zeros(1, TCPFLOW_DTYPE)[0]
    flow["contig_len"] = contig_of([(wo, wo + len(b)) for c, _, wo, b in todo if c])
    flow["counted"] = sum(1 for t in todo if t[0])
    flow["redelivered"] = redel
    flow["valid"] = 1
    return segs, flow


def expected(recs, kinds, flags, groups, wins, accept, arena_size: int, sentinel: int = SENTINEL):
    """What the call leaves: (segs, flows, arena, written).  recs: the records' bytes; kinds / flags: per
    record; groups: (first, count, reserved) each; wins: TCPWIN_DTYPE, one per group; accept: per record,
    whether its status byte has ST_ACCEPT.  segs of records the call does not write stay zero; written[i]:
    record i belongs to a valid group (its status byte and segment entry are written)."""
    n = len(recs)
    segs = np.zeros(n, TCPSEG_DTYPE)
    flows = np.zeros(len(groups), TCPFLOW_DTYPE)
    arena = np.full(arena_size, sentinel, np.uint8)
    written = np.zeros(n, bool)
    for gi, (first, count, reserved) in enumerate(groups):
        first, count = int(first), int(count)
        if not group_valid(first, count, int(reserved), n, wins[gi]):
            continue
        items = []
        for i in range(first, first + count):
            t = tcp_segment(recs[i], int(kinds[i]), int(flags[i]))
            items.append(None if t is None else (t[2], recs[i][t[0]:t[0] + t[1]], t[0], t[3], bool(accept[i])))
        segs[first:first + count], flows[gi] = assemble_group(items, wins[gi], arena)
        written[first:first + count] = True
    return segs, flows, arena, written


class Assembler:
    """src/storage/assembler.rs on absolute offsets: disjoint data ranges behind `front`, at most `limit`
    of them (None: unbounded; the reference's ASSEMBLER_MAX_SEGMENT_COUNT is 4)."""

    def __init__(self, limit=None):
        self.front, self.ranges, self.limit = 0, [], limit

    def add_then_remove_front(self, offset: int, size: int):
        """Returns the bytes that became contiguous at the front, or None for TooManyHolesError (nothing
        changes)."""
        a, b = self.front + offset, self.front + offset + size
        if offset == 0 and (not self.ranges or b < self.ranges[0][0]):  # guaranteed to succeed (:307-310)
            self.front = b
            return size
        touch = [r for r in self.ranges if r[0] <= b and a <= r[1]]
        if not touch and self.limit is not None and len(self.ranges) >= self.limit:
            return None
        for r in touch:
            a, b = min(a, r[0]), max(b, r[1])
        self.ranges = sorted([r for r in self.ranges if r not in touch] + [(a, b)])
        if self.ranges[0][0] == self.front:
            self.front = self.ranges.pop(0)[1]
            return self.front - a
        return 0


def sequential_socket(segments, window_start: int, window_len: int, ring_pos: int, ring_len: int, hole_limit=None,
                      sentinel: int = SENTINEL):
    """TcpSocket::process' receive path over `segments` ((seq, payload) each), one at a time.  window_end
    stays where the last ACK put it; window_start moves with every enqueue.  Returns a dict: contig (bytes
    enqueued in total), ring (the ring's storage, sentinel-filled), in_window and stored (per segment)."""
    ring = np.full(ring_len, sentinel, np.uint8)
    asm = Assembler(hole_limit)
    in_window, stored = [], []
    for seq, payload in segments:
        f, p = asm.front, len(payload)
        s = int(seq_diff(seq, window_start))  # relative to the poll's first window_start; the window is [f, W)
        e, W = s + p, window_len
        if p == 0:
            inw = s != f - 1 and (s == f if f == W else f <= s < W)
        else:
            inw = f != W and (f <= s < W or f < e <= W)
        in_window.append(inw)
        stored.append(False)
        if not inw:
            continue
        lo, hi = max(s, f), min(e, W)
        if hi - lo == 0 or asm.add_then_remove_front(lo - f, hi - lo) is None:
            continue
        data = np.frombuffer(payload[lo - s:hi - s], np.uint8)
        idx = (ring_pos + lo + np.arange(hi - lo)) % ring_len
        ring[idx] = data
        stored[-1] = True
    return dict(contig=asm.front, ring=ring, in_window=in_window, stored=stored)
