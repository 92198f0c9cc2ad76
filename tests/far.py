"""The sparse-arena rig: batches whose 64-bit byte offsets lie at and past a seam (2^32 on the device).

Every batched call of include/smolcsum.h takes 64-bit byte offsets, and the kernels split them into 32-bit
halves by hand.  A case here is built compactly, the way the other modules build theirs (P.pack,
C.place_records, E.make_*), its reference runs on the compact buffers (oracle.batch_*, tests/*_ref.py), and a
placement map, a list of extents (compact_lo, compact_hi, far_lo), moves every object to its place in an
`Arena` of a little more than `seam` bytes and rewrites every offset that points at it.  What does not depend
on position (status bytes, entries) is compared as it is.

Three placements: NEAR (wholly below the seam: the control), STRADDLE (begins below the seam and ends above
it; one object per arena can) and FAR (wholly above it, FAR_LO with small low words from seam + 37 up, FAR_HI
with large ones down from the arena's end).  NEAR objects start at size - seam + 3, above every address a FAR
one has with its high word dropped, so a load that lost its high word reads the sentinel and a store that lost
it lands in bytes `Arena.check` scans.

The builders take the seam and the arena size as parameters: tests/test_far_rig_cpu.py runs them with seam
2^20 over host memory, the oracle standing in for the engine, and checks there that the rig sees a dropped
high word and a stray store; tests/test_gpu_far_offsets.py runs them with seam 2^32 on the device."""
from __future__ import annotations

import numpy as np

import oracle
from smoltcp_amd import engine as E
from tests import pktgen as P

DST_FILL = 0xA5   # arenas: a byte no call may change outside what it writes
PRE_FILL = 0x5A   # status and entry tensors: bytes the call must not write keep it
MARGIN = 256      # every expected extent is compared with this many bytes around it
SLICE = 256 << 20  # the sentinel scan's largest temporary
TAIL = 64         # bytes kept free at the arena's end (the suite's buffers all carry tail slack)
GPU_SEAM = 1 << 32
GPU_SIZE = (1 << 32) + (1 << 28)
NEAR, STRADDLE, FAR_LO, FAR_HI = 0, 1, 2, 3
FAR = (FAR_LO, FAR_HI)
NOCAPS = (0, 0, 0, 0, 0)


class Arena:
    """`size` bytes of `fill`, on the device (backend "torch") or on the host ("numpy")."""

    def __init__(self, size: int, seam: int, backend: str, fill: int = DST_FILL, slice_bytes: int = SLICE):
        assert backend in ("torch", "numpy") and 0 < seam < size
        self.size, self.seam, self.backend, self.fill, self.slice_bytes = size, seam, backend, fill, slice_bytes
        if backend == "torch":
            import torch

            self.buf = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
        else:
            self.buf = np.full(size, fill, np.uint8)

    def refill(self):
        if self.backend == "torch":
            self.buf.fill_(self.fill)
        else:
            self.buf[:] = self.fill

    def put(self, far_lo: int, data):
        """Upload one extent."""
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        assert 0 <= far_lo and far_lo + a.size <= self.size
        if a.size == 0:
            return
        if self.backend == "torch":
            import torch

            self.buf[far_lo:far_lo + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        else:
            self.buf[far_lo:far_lo + a.size] = a

    def get(self, lo: int, hi: int) -> np.ndarray:
        return self.buf[lo:hi].cpu().numpy() if self.backend == "torch" else self.buf[lo:hi].copy()

    def _stray(self, lo: int, hi: int):
        """The first byte of [lo, hi) that is not the fill, or None; no temporary above slice_bytes."""
        if self.backend == "numpy":
            for a in range(lo, hi, self.slice_bytes):
                bad = np.flatnonzero(self.buf[a:min(hi, a + self.slice_bytes)] != self.fill)
                if bad.size:
                    return a + int(bad[0])
            return None
        import torch

        dirty = torch.zeros((), dtype=torch.bool, device="cuda")
        for a in range(lo, hi, self.slice_bytes):
            dirty |= (self.buf[a:min(hi, a + self.slice_bytes)] != self.fill).any()
        if not bool(dirty):
            return None
        for a in range(lo, hi, self.slice_bytes):
            bad = torch.nonzero(self.buf[a:min(hi, a + self.slice_bytes)] != self.fill)
            if bad.numel():
                return a + int(bad[0])

    def check(self, expected):
        """expected: (far_lo, bytes) extents, all the arena holds.  Every extent, widened by MARGIN on each
        side, equals the expectation on the host; every byte outside the widened extents still equals the fill
        (a store whose high word was dropped lands at its offset mod the seam, which is there)."""
        ext = sorted(((int(lo), np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b)
                      for lo, b in expected), key=lambda e: e[0])
        wide = []
        for lo, b in ext:
            a, z = max(0, lo - MARGIN), min(self.size, lo + b.size + MARGIN)
            if wide and a <= wide[-1][1]:
                wide[-1][1] = max(wide[-1][1], z)
            else:
                wide.append([a, z])
        k = 0
        for a, z in wide:
            want = np.full(z - a, self.fill, np.uint8)
            while k < len(ext) and ext[k][0] < z:
                lo, b = ext[k]
                want[lo - a:lo - a + b.size] = b
                k += 1
            got = self.get(a, z)
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, f"arena bytes differ at {[hex(a + int(d)) for d in diff[:8]]}: got " \
                                   f"{got[diff[:8]]} want {want[diff[:8]]}"
        pos = 0
        for a, z in wide + [[self.size, self.size]]:
            stray = self._stray(pos, a)
            assert stray is None, f"a byte outside every expected extent was written: arena[{hex(stray)}]"
            pos = z


class Layout:
    """Hands out arena addresses by placement; the straddling object is placed first."""

    def __init__(self, seam: int, size: int, rng):
        self.seam, self.size, self.rng = seam, size, rng
        self.near, self.lo, self.hi, self.near_end = size - seam + 3, seam + 37, size - TAIL - 1, seam
        self.used = False  # whether anything has been placed

    def straddle(self, n: int, below: int) -> int:
        """An object of n bytes, `below` of them below the seam."""
        assert 0 < below < n and not self.used, "one straddling object, placed first"
        self.used = True
        self.near_end = self.seam - below
        self.lo = max(self.lo, self.near_end + n + 37)
        return self.near_end

    def place(self, where: int, n: int, gap: int | None = None) -> int:
        gap = int(self.rng.integers(0, 8)) if gap is None else gap
        self.used = True
        if where == NEAR:
            o = self.near + gap
            self.near = o + n
            assert self.near + MARGIN <= self.near_end
        elif where == FAR_LO:
            o = self.lo + gap
            self.lo = o + n
        else:
            assert where == FAR_HI
            o = self.hi - gap - n
            self.hi = o
        assert self.lo <= self.hi, "the arena's far part is full"
        return o


class Placement:
    """The map from compact offsets to arena offsets: extents (compact_lo, compact_hi, far_lo)."""

    def __init__(self, extents):
        self.ext = sorted((int(a), int(b), int(f)) for a, b, f in extents)
        for (a, b, _), (a2, _, _) in zip(self.ext, self.ext[1:]):
            assert a <= b <= a2, "compact extents overlap"
        far = sorted((f, f + b - a) for a, b, f in self.ext)
        for (_, z), (a2, _) in zip(far, far[1:]):
            assert z <= a2, "arena extents overlap"
        self.clo = np.array([e[0] for e in self.ext], np.int64)

    def far(self, off, length=0):
        """The arena offset of the object of `length` bytes at compact offset `off` (arrays broadcast)."""
        off, length = np.asarray(off, np.int64), np.asarray(length, np.int64)
        k = np.maximum(np.searchsorted(self.clo, off, "right") - 1, 0)
        chi = np.array([e[1] for e in self.ext], np.int64)[k]
        flo = np.array([e[2] for e in self.ext], np.int64)[k]
        assert ((self.clo[k] <= off) & (off + length <= chi)).all(), "an object lies outside every extent"
        return (off - self.clo[k] + flo).astype(np.uint64)

    def where(self, off, length, seam):
        """NEAR / STRADDLE / FAR_LO (any wholly-far object) of the objects at compact offsets `off`."""
        f = self.far(off, length).astype(np.int64)
        return np.where(f + np.asarray(length, np.int64) <= seam, NEAR, np.where(f >= seam, FAR_LO, STRADDLE))

    def upload(self, arena: Arena, compact: np.ndarray):
        """Every extent of `compact` to its place; neighbours less than 4 KiB apart travel as one piece, the
        bytes between them as the arena's fill."""
        far = sorted((f, a, b) for a, b, f in self.ext if b > a)
        k = 0
        while k < len(far):
            j, end = k, far[k][0] + far[k][2] - far[k][1]
            while j + 1 < len(far) and far[j + 1][0] - end < 4096:
                j += 1
                end = far[j][0] + far[j][2] - far[j][1]
            piece = np.full(end - far[k][0], arena.fill, np.uint8)
            for f, a, b in far[k:j + 1]:
                piece[f - far[k][0]:f - far[k][0] + b - a] = compact[a:b]
            arena.put(far[k][0], piece)
            k = j + 1

    def expected(self, compact: np.ndarray):
        """The extents of `compact` (the reference's buffer after the call) where the arena holds them."""
        return [(f, compact[a:b]) for a, b, f in self.ext]


def accepted_enough(where, ok, what=""):
    """The rig's condition: at least half of the STRADDLE objects and at least half of the FAR ones are accepted
    by the reference (a dropped high word reads the sentinel; an object the reference rejects anyway would
    not show it).  where: placement per object (FAR_LO / FAR_HI both count as FAR); ok: bool per object."""
    where, ok = np.asarray(where), np.asarray(ok, bool)
    for name, m in (("STRADDLE", where == STRADDLE), ("FAR", (where == FAR_LO) | (where == FAR_HI))):
        if m.any():
            assert 2 * int(ok[m].sum()) >= int(m.sum()), f"{what}: {int(ok[m].sum())} of {int(m.sum())} {name} objects accepted"


# ---- descriptor batches: verify / emit / data -------------------------------------------------------------

class DescCase:
    """One descriptor batch in its compact and its far form.

    compact: the batch buffer with every checksum filled (verify's input); raw: the same before the oracle
    filled them (emit's input); offs / lens / kinds: the descriptors in batch order (compact
    offsets); where: their placements; place: the Placement; desc_far: smol_csum_desc_t with arena offsets."""

    def __init__(self, compact, offs, lens, kinds, where, place, raw=None):
        self.raw = compact if raw is None else raw
        self.compact, self.offs, self.lens, self.where, self.place = compact, offs, lens, np.asarray(where), place
        self.kinds = np.broadcast_to(np.asarray(kinds, np.uint8), (len(offs),)).copy()
        self.n = len(offs)
        self.desc = E.make_descriptors(offs, lens, self.kinds)
        self.desc_far = E.make_descriptors(place.far(offs, lens), lens, self.kinds)

    def fill(self, arena: Arena, compact=None):
        arena.refill()
        self.place.upload(arena, self.compact if compact is None else compact)

    def batch_of(self):
        """The device batch of the far descriptors (made on first use; the GPU module's)."""
        if getattr(self, "batch", None) is None:
            import torch

            self.batch = E.Batch(n=self.n, desc=torch.from_numpy(self.desc_far.view(np.uint8).copy()).cuda())
        return self.batch

    def ref_verify(self, caps=NOCAPS, compact=None):
        return oracle.batch_verify((self.compact if compact is None else compact).copy(), self.desc, self.n, caps=caps)

    def ref_emit(self, caps=NOCAPS):
        """(status bytes, the compact buffer after emit) of emit over `raw`."""
        after = self.raw.copy()
        return oracle.batch_emit(after, self.desc, self.n, caps=caps), after

    def ref_data(self):
        return oracle.batch_data(self.compact, self.desc, self.n)


def eth_frame(rec: bytes) -> bytes:
    """An IP record behind an Ethernet header of its own version's ethertype (IPv4's for anything else)."""
    return P.eth(rec, 0x86DD if rec[:1] and rec[0] >> 4 == 6 else 0x0800)


def tcp_run(rng, count: int, lo: int, hi: int):
    """`count` IPv4 / TCP records of lo..hi-1 bytes (checksums 0), to be packed back to back."""
    recs = []
    for _ in range(count):
        n = int(rng.integers(lo, hi))
        recs.append(P.ipv4(P.rand_bytes(rng, 4), P.rand_bytes(rng, 4), 6, P.tcp(7, 9, P.rand_bytes(rng, n - 40))))
    return recs


def desc_case(seam: int, size: int, recs, kind: int, seed: int, placements=(NEAR, STRADDLE, FAR_LO, FAR_HI), *,
              straddle_below: int = 21, straddle_index: int | None = None, shuffle: bool = True, lay: Layout | None = None,
              run=None, run_seam_record: int = 35, flip_every: int = 0):
    """`recs` (bytes each, any checksums) as a descriptor batch.

    placements: record i gets placements[i mod len].  One STRADDLE record straddles the seam with
    straddle_below bytes below it: record straddle_index, or the first STRADDLE one of at least 64 bytes; the
    other STRADDLE ones take the next placement.
    shuffle: the descriptors are listed in shuffled order, so that 8 consecutive ones, one wavefront of the
    descriptor walk, hold near and far records; False keeps the records' order, for calls whose groups name
    runs of records.
    lay: a Layout shared with something else in the arena that straddles already.
    flip_every: the oracle's emit (default caps) fills every checksum first; one bit is then flipped in every
    flip_every-th record but the straddling one, so that verify has something to reject.
    run: records packed back to back, listed in order after the others from a descriptor index that is a
    multiple of 8.  The seam falls inside run[run_seam_record], whose index mod 8 is neither 0 nor 7: the carry
    into the high word happens inside one wavefront's 8 records.  The run is the arena's straddling object, so
    no single record straddles then."""
    rng = np.random.default_rng(seed)
    recs = list(recs)
    while run is not None and len(recs) % 8:
        recs.append(recs[len(recs) // 2])
    buf, offs, lens = P.pack(recs, gap_rng=rng)
    n = len(recs)
    lay = Layout(seam, size, rng) if lay is None else lay  # (a shared one: something else straddles already)
    ext, where = [], np.zeros(n, np.int64)
    cand = [p for p in placements if p != STRADDLE] or [NEAR]
    want = [placements[i % len(placements)] for i in range(n)]
    if run is not None:
        assert 0 < run_seam_record % 8 < 7 and run_seam_record < len(run)
        rbuf, roffs, rlens = P.pack(run)
        rbuf = rbuf[:int(roffs[-1] + rlens[-1])]
        below = int(roffs[run_seam_record]) + int(rlens[run_seam_record]) // 2
        base = lay.straddle(rbuf.size, below)
        ext.append((buf.size, buf.size + rbuf.size, base))
        roffs = roffs + np.uint64(buf.size)
        buf = np.concatenate([buf, rbuf, np.zeros(16, np.uint8)])
    elif STRADDLE in placements:
        k = next(i for i in range(n) if want[i] == STRADDLE and lens[i] >= 64) if straddle_index is None else straddle_index
        below = min(straddle_below, int(lens[k]) - 1)
        ext.append((int(offs[k]), int(offs[k] + lens[k]), lay.straddle(int(lens[k]), below)))
        where[k] = STRADDLE
        want[k] = None
    for i in range(n):
        if want[i] is None:
            continue
        w = want[i] if want[i] != STRADDLE else cand[i % len(cand)]
        ext.append((int(offs[i]), int(offs[i] + lens[i]), lay.place(w, int(lens[i]))))
        where[i] = w
    order = rng.permutation(n) if shuffle else np.arange(n)
    offs, lens, where = offs[order], lens[order], where[order]
    if run is not None:
        offs, lens = np.concatenate([offs, roffs]), np.concatenate([lens, rlens])
        f = base + (roffs - roffs[0]).astype(np.int64)
        where = np.concatenate([where, np.where(f + rlens <= seam, NEAR, np.where(f >= seam, FAR_LO, STRADDLE))])
    raw = buf.copy()
    oracle.batch_emit(buf, E.make_descriptors(offs, lens, kind), len(offs))
    if flip_every:
        for i in range(0, len(offs), flip_every):
            if lens[i] and where[i] != STRADDLE:
                buf[int(offs[i]) + int(lens[i]) - 1] ^= 0x10
    case = DescCase(buf, offs, lens, kind, where, Placement(ext), raw)
    if run is not None:  # the run's records end where the next begins, across the seam, inside one wavefront
        d = case.desc_far[n:]
        assert n % 8 == 0 and (d["offset"][1:] == d["offset"][:-1] + d["len"][:-1]).all()
        s = n + run_seam_record
        assert case.desc_far["offset"][s] < seam < case.desc_far["offset"][s] + case.desc_far["len"][s]
    return case


def data_case(seam: int, size: int, seed: int, lengths=(1, 2, 63, 64, 1500, 131075)):
    """Raw spans for data(): for every length, spans that begin at each byte of the 16-byte window
    [seam - 8, seam + 8) and spans that end at each of them, over one region of random bytes that holds 0xFF
    bytes around the seam (never the arena's fill throughout); plus the same lengths NEAR and FAR.  The spans
    overlap: data() only reads."""
    rng = np.random.default_rng(seed)
    big = max(lengths)
    region = rng.integers(0, 256, 2 * (big + 16), dtype=np.uint8)
    mid = big + 16  # the region's byte that lies at the seam
    region[mid - 40:mid + 40] = 0xFF
    lay = Layout(seam, size, rng)
    ext = [(0, region.size, lay.straddle(region.size, mid))]
    offs, lens = [], []
    for ln in lengths:
        for p in range(-8, 8):
            offs += [mid + p, mid + p - ln]
            lens += [ln, ln]
    chunks, pos = [region], region.size
    for where in (NEAR, FAR_LO, FAR_HI):
        for ln in lengths:
            b = rng.integers(0, 256, ln, dtype=np.uint8) if ln % 2 else np.full(ln, 0xFF, np.uint8)
            ext.append((pos, pos + ln, lay.place(where, ln)))
            offs.append(pos)
            lens.append(ln)
            chunks.append(b)
            pos += ln
    place = Placement(ext)
    offs, lens = np.array(offs, np.uint64), np.array(lens, np.uint32)
    order = rng.permutation(len(offs))
    offs, lens = offs[order], lens[order]
    return DescCase(np.concatenate(chunks + [np.zeros(16, np.uint8)]), offs, lens, E.KIND_RAW,
                    place.where(offs, lens, seam), place)


# ---- sparse fixed stride ------------------------------------------------------------------------------------

class FixedCase:
    """n records of L bytes, `stride` apart from arena offset `base`: record r at base + r * stride.  The
    compact buffer holds them back to back.  base is chosen so that one record straddles the seam."""

    def __init__(self, seam: int, size: int, stride: int, L: int, below: int | None = None):
        self.seam, self.stride, self.L = seam, stride, L
        r = seam // stride  # the record that is to straddle: base + r * stride = seam - below
        below = L // 3 + 1 if below is None else below
        assert 0 < below < L and L <= stride
        self.base = (seam - below) - r * stride
        while self.base < 0:
            r -= 1
            self.base += stride
        self.n = (size - TAIL - self.base - L) // stride + 1
        self.far = self.base + np.arange(self.n, dtype=np.int64) * stride
        self.where = np.where(self.far + L <= seam, NEAR, np.where(self.far >= seam, FAR_LO, STRADDLE))
        self.place = Placement([(i * L, (i + 1) * L, int(f)) for i, f in enumerate(self.far)])
        assert int((self.far >= seam).sum()) >= 8 and (self.where == STRADDLE).sum() == 1

    def fill(self, arena: Arena, compact: np.ndarray):
        arena.refill()
        self.place.upload(arena, compact)


# ---- the engine's stand-ins on the host (tests/test_far_rig_cpu.py) ---------------------------------------

def _oracle_op(op, buf, desc, caps):
    n = len(desc)
    if op == "verify":
        return oracle.batch_verify(buf, desc, n, caps=caps)
    if op == "emit":
        return oracle.batch_emit(buf, desc, n, caps=caps)
    assert op == "data"
    return oracle.batch_data(buf, desc, n)


def standin(arena: Arena, desc_far, op: str, caps=NOCAPS):
    """The oracle on the sparse buffer itself: what a correct engine does."""
    return _oracle_op(op, arena.buf, np.ascontiguousarray(desc_far), caps)


def standin_dropped_high_word(arena: Arena, desc_far, op: str, caps=NOCAPS):
    """An engine that drops the high word of every byte address: address a becomes a mod seam (the seam is a
    power of two), for loads and stores alike."""
    seam = arena.seam
    assert seam & (seam - 1) == 0
    out = []
    for d in desc_far:
        idx = (int(d["offset"]) + np.arange(int(d["len"]), dtype=np.int64)) & (seam - 1)
        rec = np.concatenate([arena.buf[idx], np.zeros(16, np.uint8)])
        one = E.make_descriptors([0], [int(d["len"])], int(d["kind"]), int(d["flags"]))
        out.append(_oracle_op(op, rec, one, caps)[0])
        if op == "emit":
            arena.buf[idx] = rec[:idx.size]
    return np.array(out, np.uint16 if op == "data" else np.uint8)


def standin_stray_store(arena: Arena, desc_far, op: str, caps=NOCAPS):
    """A correct engine but for one extra byte stored at far_lo - seam of the first far record."""
    out = standin(arena, desc_far, op, caps)
    far = desc_far["offset"][desc_far["offset"] >= arena.seam]
    arena.buf[int(far[0]) - arena.seam] ^= 0xFF
    return out


# ---- destinations of the calls with a second buffer -------------------------------------------------------

def chain_slots(seam: int, size: int, caps, pivot: int, seam_at, rng, lay: Layout | None = None):
    """Slots of caps[i] bytes each, back to back in shuffled order, in three pieces: the first third NEAR, the
    last third FAR_HI, the middle third one chain across the seam with slot `pivot` at it: seam_at "inside"
    puts the seam inside that slot (it straddles), "end" right after its last byte (it ends at seam - 1 and
    the next slot begins at the seam), "start" at its first byte.  Returns (arena offset per slot, placement
    per slot: NEAR / STRADDLE / FAR_LO / FAR_HI)."""
    caps = np.asarray(caps, np.int64)
    n = len(caps)
    assert n >= 9 and caps[pivot] >= 2
    order = [int(i) for i in rng.permutation(n) if i != pivot]
    order.insert(n // 2, pivot)
    pos = np.zeros(n + 1, np.int64)
    pos[1:] = np.cumsum(caps[order])
    a, b, k = n // 3, 2 * n // 3, n // 2
    inside = {"inside": caps[pivot] // 2, "end": caps[pivot], "start": 0}.get(seam_at, seam_at)
    p = pos[k] + int(inside)
    lay = Layout(seam, size, rng) if lay is None else lay
    mid = lay.straddle(int(pos[b] - pos[a]), int(p - pos[a]))
    near, hi = lay.place(NEAR, int(pos[a])), lay.place(FAR_HI, int(pos[n] - pos[b]))
    far, where = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j, i in enumerate(order):
        far[i] = near + pos[j] if j < a else mid + pos[j] - pos[a] if j < b else hi + pos[j] - pos[b]
        where[i] = NEAR if far[i] + caps[i] <= seam else (FAR_HI if j >= b else FAR_LO) if far[i] >= seam else STRADDLE
    assert far[pivot] + int(inside) == seam
    if 0 < inside < caps[pivot]:
        assert where[pivot] == STRADDLE
    else:
        assert (far + caps == seam).any() and (far == seam).any()
    return far.astype(np.uint64), where


def chain_slots_compact(seam: int, size: int, caps, pivot: int, seam_at, rng, lay: Layout | None = None):
    """chain_slots for a reference that fills a compact arena: (compact offset per slot, arena offset per slot,
    placement per slot, the Placement of the compact arena's three pieces, the compact arena's size)."""
    state = rng.bit_generator.state
    far, where = chain_slots(seam, size, caps, pivot, seam_at, rng, lay)
    rng.bit_generator.state = state  # the same shuffle again
    caps = np.asarray(caps, np.int64)
    n = len(caps)
    order = [int(i) for i in rng.permutation(n) if i != pivot]
    order.insert(n // 2, pivot)
    pos = np.zeros(n + 1, np.int64)
    pos[1:] = np.cumsum(caps[order])
    compact = np.zeros(n, np.int64)
    compact[order] = pos[:-1]
    a, b = n // 3, 2 * n // 3
    ext = [(int(pos[lo]), int(pos[hi]), int(far[order[lo]])) for lo, hi in ((0, a), (a, b), (b, n)) if pos[hi] > pos[lo]]
    place = Placement(ext)
    assert (place.far(compact, caps).astype(np.int64) == far.astype(np.int64))[caps > 0].all()
    return compact.astype(np.uint64), far, where, place, int(pos[n])


def pairs_present(rec_where, dst_where):
    """Every (record placement x destination placement) pair occurs (FAR_LO / FAR_HI: FAR)."""
    fold = lambda w: np.where(np.asarray(w) == FAR_HI, FAR_LO, np.asarray(w))
    return {(int(a), int(b)) for a, b in zip(fold(rec_where), fold(dst_where))}


# ---- the cases of the calls with a second buffer -------------------------------------------------------------
# Each builder takes the seam and the arena size, answers with the references on compact host buffers, asserts
# the rig's condition (accepted_enough) and the (record placement x destination placement) pairs it promises,
# and returns what the device call needs.  tests/test_far_rig_cpu.py runs every one at the small seam.

V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
V6A, V6B = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
BASE_PAIRS = {(a, b) for a in (NEAR, FAR_LO) for b in (NEAR, FAR_LO)}
SEAM_IN_RUN = {"between": lambda S, fl: 2 * S, "inside": lambda S, fl: 2 * S + fl // 2}


def _placed(case, buf=None):
    buf = case.raw if buf is None else buf
    return [bytes(buf[int(o):int(o + ln)]) for o, ln in zip(case.offs, case.lens)]


def _changed(case, before, after):
    return np.array([not np.array_equal(after[int(o):int(o + ln)], before[int(o):int(o + ln)])
                     for o, ln in zip(case.offs, case.lens)])


def payload_records(rng, n: int, long=(20000, 60000)):
    """Records that mostly carry a UDP / TCP payload, IPv4 and IPv6; every 37th a TCP segment of long[0] ..
    long[1] bytes, every 41st 0-40 random bytes."""
    recs = []
    for i in range(n):
        pl = P.rand_bytes(rng, int(rng.integers(1, 1473)))
        s4, d4, s6, d6 = P.rand_bytes(rng, 4), P.rand_bytes(rng, 4), P.rand_bytes(rng, 16), P.rand_bytes(rng, 16)
        recs.append([P.ipv4(s4, d4, 17, P.udp(7, 9, pl)), P.ipv4(s4, d4, 6, P.tcp(7, 9, pl)), P.ipv6(s6, d6, 17, P.udp(7, 9, pl)),
                     P.ipv6(s6, d6, 6, P.tcp(7, 9, pl)), P.ipv4(s4, d4, 1, P.icmp_echo(8, pl))][i % 5])
    for i in range(0, n, 37):
        recs[i] = P.ipv4(V4A, V4B, 6, P.tcp(1, 2, P.rand_bytes(rng, int(rng.integers(*long)))))
    for i in range(5, n, 41):
        recs[i] = P.rand_bytes(rng, int(rng.integers(0, 40)))
    return recs


def vcopy_case(seam, size, kind, seam_at, n=400, long=(20000, 60000)):
    """verify_copy: records NEAR / STRADDLE / FAR, slots back to back across the seam in shuffled record order;
    the straddling record's slot straddles ("inside"), ends at seam - 1 ("end") or begins at the seam ("start")."""
    from types import SimpleNamespace

    from tests.test_verify_copy_cpu import expected_span

    rng = np.random.default_rng(len(seam_at) + kind)
    recs = payload_records(np.random.default_rng(31), n, long)
    case = desc_case(seam, size, [eth_frame(r) for r in recs] if kind == E.KIND_ETH else recs, kind, 32, flip_every=5,
                     straddle_index=37, straddle_below=long[0] // 2)
    placed = _placed(case, case.compact)
    spans = [expected_span(r, kind, 0) for r in placed]
    caps = np.array([sp[1] if sp else 7 for sp in spans], np.int64)
    caps[3::11] = np.maximum(caps[3::11] - 1, 0)  # too small by one byte: reported, not delivered
    caps[4::13] += 5                               # roomy: the slot's last 5 bytes keep the fill
    pivot = int(np.flatnonzero(case.where == STRADDLE)[0])
    caps[pivot] = spans[pivot][1]
    far, dwhere = chain_slots(seam, size, caps, pivot, seam_at, rng)
    ref_sp, expected = np.zeros(case.n, E.SPAN_DTYPE), []
    for i, sp in enumerate(spans):
        if sp is None:
            continue
        ref_sp[i]["off"], ref_sp[i]["len"] = sp
        if sp[1] <= caps[i]:
            ref_sp[i]["copied"] = 1
            expected.append((int(far[i]), np.frombuffer(placed[i][sp[0]:sp[0] + sp[1]], np.uint8)))
    delivered = (ref_sp["copied"] == 1) & (ref_sp["len"] > 0)
    accepted_enough(case.where, delivered, "verify_copy records")
    accepted_enough(dwhere, delivered, "verify_copy slots")
    pairs = pairs_present(case.where[delivered], dwhere[delivered])
    want = BASE_PAIRS | {(STRADDLE, {"inside": STRADDLE, "end": NEAR, "start": FAR_LO}[seam_at])}
    assert want <= pairs, want - pairs
    return SimpleNamespace(case=case, ref_st=case.ref_verify(), ref_sp=ref_sp, slots=E.make_slots(far, caps), dwhere=dwhere,
                           expected=expected, pairs=pairs)


def copy_emit_case(seam, size, seam_at):
    """copy_emit: records NEAR / STRADDLE / FAR, payload sources of 0, 1, 15, 16, 17 and 1460 bytes back to back
    across the seam in the second arena: a FAR record's 1460-byte source crosses it ("inside"), or the straddling
    record's ends at seam - 1 and the next begins at the seam ("end")."""
    from types import SimpleNamespace

    rng = np.random.default_rng(60 + len(seam_at))
    recs, spec = [], []
    for i in range(240):
        ln = (0, 1, 15, 16, 17, 1460)[i % 6]
        s4, d4, s6, d6 = P.rand_bytes(rng, 4), P.rand_bytes(rng, 4), P.rand_bytes(rng, 16), P.rand_bytes(rng, 16)
        r, hdr = [(P.ipv4(s4, d4, 17, P.udp(7, 9, bytes(ln))), 28), (P.ipv4(s4, d4, 6, P.tcp(7, 9, bytes(ln))), 40),
                  (P.ipv6(s6, d6, 17, P.udp(7, 9, bytes(ln))), 48), (P.ipv6(s6, d6, 6, P.tcp(7, 9, bytes(ln))), 60)][(i // 6) % 4]
        recs.append(r)
        spec.append((hdr, ln))
    case = desc_case(seam, size, recs, E.KIND_IP, 61, shuffle=False, straddle_index=5, straddle_below=500)
    lens, dst0 = np.array([c[1] for c in spec], np.int64), [c[0] for c in spec]
    pivot = 11 if seam_at == "inside" else 5
    assert lens[pivot] == 1460 and case.where[5] == STRADDLE and case.where[11] in FAR
    s_compact, s_far, swhere, splace, total = chain_slots_compact(seam, size, lens, pivot, seam_at, rng)
    src = rng.integers(0, 256, total + 16, dtype=np.uint8)
    after = case.raw.copy()
    ref_st = oracle.batch_copy_emit(after, case.desc, case.n, src, E.make_copies(s_compact, dst0, lens))
    assert not (ref_st & E.ST_MALFORMED).any()
    changed = _changed(case, case.raw, after)
    accepted_enough(case.where, changed, "copy_emit records")
    accepted_enough(swhere, changed & (lens > 0), "copy_emit sources")
    pairs = pairs_present(case.where[lens > 0], swhere[lens > 0])
    assert BASE_PAIRS | {(FAR_LO, STRADDLE) if seam_at == "inside" else (STRADDLE, NEAR)} <= pairs
    return SimpleNamespace(case=case, after=after, ref_st=ref_st, copies=E.make_copies(s_far, dst0, lens), src=src[:total],
                           splace=splace, pairs=pairs)


def tcp_frame(seq, payload, sport=1000, dport=80):
    """One Ethernet / IPv4 / TCP frame, checksums 0 (the oracle's emit fills them)."""
    return P.eth(P.ipv4(V4A, V4B, 6, P.tcp(sport, dport, payload, seq=seq & 0xFFFFFFFF)))


def tcpasm_case(seam, size, rot):
    """verify_tcp_assemble: four flows whose frames lie NEAR, STRADDLE and FAR in each flow; one ring straddles
    the seam at ring offset 3000 with ring_pos 6500 of 8000, so that the 6000-byte window wraps around the
    ring's end while a segment's piece crosses the seam; the other rings NEAR, FAR_LO, FAR_HI.  rot moves the
    flow that holds the straddling frame to the straddling / the FAR / the NEAR ring."""
    from types import SimpleNamespace

    from tests import tcp_assemble_ref as R

    rng = np.random.default_rng(40 + rot)
    pay, W, RL, RP = 1460, 6000, 8000, 6500
    recs, groups, starts = [], [], [0xFFFFF000, 77, 0x7FFFFF00, 0x12345678]
    for ws in starts:
        stream = P.rand_bytes(rng, W + pay)
        first = len(recs)
        for j in (1, 0, 3, 2, 1, 4):  # out of order, one duplicate, the last one trimmed at the window's end
            recs.append(tcp_frame(ws + j * pay, stream[j * pay:(j + 1) * pay]))
        groups.append((first, len(recs) - first))
    n = len(recs)
    case = desc_case(seam, size, recs, E.KIND_ETH, 41 + rot, shuffle=False, straddle_below=700)
    assert int(np.flatnonzero(case.where == STRADDLE)[0]) < groups[0][1]  # the straddling frame is flow 0's
    ref_st = case.ref_verify()
    wins = E.make_tcpwins([3 + g * (RL + 11) for g in range(4)], RL, RP, starts, W)
    ref_segs, ref_flows, ref_arena, written = R.expected(_placed(case, case.compact), case.kinds, np.zeros(n, np.uint8),
                                                         [g + (0,) for g in groups], wins, (ref_st & E.ST_ACCEPT) != 0,
                                                         3 + 4 * (RL + 11) + 19)
    assert written.all() and (ref_flows["valid"] == 1).all() and (ref_flows["contig_len"] == W).all()
    lay = Layout(seam, size, rng)
    ring_far = {0: lay.straddle(RL, 3000)}
    ring_far.update({1: lay.place(NEAR, RL), 2: lay.place(FAR_LO, RL), 3: lay.place(FAR_HI, RL)})
    ring_of = [(g - rot) % 3 if g < 3 else 3 for g in range(4)]  # flow g's ring: 0 straddles, 1 NEAR, 2 / 3 FAR
    far = [ring_far[ring_of[g]] for g in range(4)]
    dplace = Placement([(int(wins["dst_offset"][g]), int(wins["dst_offset"][g]) + RL, far[g]) for g in range(4)])
    delivered = ref_segs["len"] > 0
    accepted_enough(case.where, delivered, "tcp_assemble frames")
    dwhere = np.repeat([(STRADDLE, NEAR, FAR_LO, FAR_HI)[ring_of[g]] for g in range(4)], [g[1] for g in groups])
    pairs = pairs_present(case.where[delivered], dwhere[delivered])
    assert {(a, b) for a in (NEAR, FAR_LO) for b in (NEAR, STRADDLE, FAR_LO)} <= pairs
    assert (STRADDLE, (STRADDLE, NEAR, FAR_LO)[ring_of[0]]) in pairs
    # a piece crosses the seam while the window wraps: the straddling ring holds bytes at both ends and on both sides
    o = int(wins["dst_offset"][ring_of.index(0)])
    ring = ref_arena[o:o + RL]
    assert (ring[[0, 2999, 3000, RL - 1]] != DST_FILL).all() and (ring[4600:6400] == DST_FILL).all()
    wins_far = wins.copy()
    wins_far["dst_offset"] = far
    return SimpleNamespace(case=case, ref_st=ref_st, ref_segs=ref_segs, ref_flows=ref_flows, ref_arena=ref_arena, dplace=dplace,
                           wins=wins_far, groups=E.make_groups([g[0] for g in groups], [g[1] for g in groups]), ring_of=ring_of,
                           pairs=pairs)


def echo_case(seam, size, kind, seam_at):
    """verify_echo_reply: ICMPv4 / ICMPv6 echo requests, two in three FAR, reply slots back to back across the
    seam: the straddling request's reply straddles ("inside") or ends at seam - 1 ("end"), or a FAR request's
    reply straddles ("far-inside")."""
    from types import SimpleNamespace

    from tests import echo_ref as R

    rng = np.random.default_rng(50 + kind + len(seam_at))
    recs = []
    for i in range(180):
        data = P.rand_bytes(rng, int(rng.choice([0, 1, 15, 16, 17, 56, 111, 113, 600, 1472])))
        recs.append(P.ipv4(V4A, V4B, 1, P.icmp_echo(8, data)) if i % 3 else P.ipv6(V6A, V6B, 58, P.icmp_echo(128, data)))
    for i in range(7, 180, 17):  # not a request: nothing written
        recs[i] = P.ipv4(V4A, V4B, 17, P.udp(7, 9, P.rand_bytes(rng, 50)))
    recs[13] = P.ipv4(V4A, V4B, 1, P.icmp_echo(8, P.rand_bytes(rng, 600)))  # the one that straddles, cut in its IP header
    if kind == E.KIND_ETH:
        recs = [eth_frame(r) for r in recs]
    case = desc_case(seam, size, recs, kind, 51, (FAR_LO, STRADDLE, FAR_HI, NEAR, FAR_LO, FAR_HI), flip_every=9,
                     straddle_index=13, straddle_below=30)
    placed, flags = _placed(case, case.compact), np.zeros(case.n, np.uint8)
    need = np.asarray(R.frame_lens(placed, case.kinds, flags, None), np.int64)
    pivot = int(np.flatnonzero(case.where == (FAR_HI if seam_at == "far-inside" else STRADDLE))[0])
    assert need[pivot] >= 2
    compact, far, dwhere, dplace, total = chain_slots_compact(seam, size, need, pivot, seam_at.split("-")[-1], rng)
    ref_st, ref_ent, ref_arena = R.expected(placed, case.kinds, flags, NOCAPS, None, E.make_slots(compact, need), total + 16)
    assert np.array_equal(ref_st, case.ref_verify())
    written = (ref_ent["flags"] & R.WRITTEN) != 0
    accepted_enough(case.where, written, "echo requests")
    accepted_enough(dwhere, written, "echo slots")
    pairs = pairs_present(case.where[written], dwhere[written])
    assert {"inside": (STRADDLE, STRADDLE), "end": (STRADDLE, NEAR), "far-inside": (FAR_LO, STRADDLE)}[seam_at] in pairs
    assert BASE_PAIRS <= pairs
    return SimpleNamespace(case=case, ref_st=ref_st, ref_ent=ref_ent, ref_arena=ref_arena[:total], dplace=dplace,
                           slots=E.make_slots(far, need), dwhere=dwhere, pairs=pairs)


def _cut_layout(seam, size, rng, first_pass, make_plans, expected, stride, pick, seam_at, lay=None):
    """The destination of a cut call: a first pass of the reference says what each record's frames need, the
    slots lie back to back across the seam, SEAM_IN_RUN[seam_at] bytes into the run of record pick(sizes); the
    reference then fills a compact arena."""
    sz = first_pass()
    S = np.where(stride, stride, sz["frame_len"]).astype(np.int64)
    need = np.where(sz["count"] > 0, (sz["count"].astype(np.int64) - 1) * S + sz["last_len"], 0)
    pivot = pick(sz)
    at = SEAM_IN_RUN[seam_at](int(S[pivot]), int(sz["frame_len"][pivot]))
    assert 0 < at < need[pivot]
    compact, far, dwhere, dplace, total = chain_slots_compact(seam, size, need, pivot, at, rng, lay)
    ref_out, ref_arena = expected(make_plans(compact, need), total + 16)
    return far, need, dwhere, dplace, ref_out, ref_arena[:total], pivot


def fragcut_case(seam, size, seam_at, strided):
    """fragment_emit: IPv4 datagrams NEAR / STRADDLE / FAR cut at MTU 576 into frame runs dst_offset + k * S NEAR,
    FAR and across the seam: the seam between two frames of a FAR datagram's run, or inside a frame; frames back
    to back or frame length + 5 apart."""
    from types import SimpleNamespace

    from tests import fragment_ref as C
    from tests import test_frag_cpu as FC

    rng = np.random.default_rng(70 + strided + 2 * len(seam_at))
    recs = FC.datagrams(rng, 120, 8, 5000)
    recs[5] = P.ipv4(FC.A, FC.B, 17, P.udp(4000, 53, P.rand_bytes(rng, 3992)), flags_frag=0x4000)
    case = desc_case(seam, size, recs, E.KIND_IP, 71, straddle_index=5, straddle_below=1000)
    n = case.n
    placed, flags, mtus, idents = _placed(case), np.zeros(n, np.uint8), np.full(n, 576, np.uint16), 0x4000 + np.arange(n)
    stride = 581 if strided else 0
    make = lambda o, c: E.make_fragplans(o, c, mtus, idents)
    exp = lambda pl, sz: C.expected(placed, case.kinds, flags, pl, stride, NOCAPS, sz)
    far, need, dwhere, dplace, ref_out, ref_arena, pivot = _cut_layout(
        seam, size, rng, lambda: exp(make(np.zeros(n), 0), 1)[0], make, exp, stride,
        lambda sz: int(np.flatnonzero((sz["count"] >= 4) & (case.where != NEAR))[0]), seam_at)
    written = ref_out["written"] == 1
    accepted_enough(case.where, written, "fragment_emit datagrams")
    accepted_enough(dwhere, written, "fragment_emit runs")
    pairs = pairs_present(case.where[written], dwhere[written])
    assert BASE_PAIRS <= pairs and dwhere[pivot] == STRADDLE and written[pivot] and case.where[pivot] != NEAR
    return SimpleNamespace(case=case, plans=make(far, need), stride=stride, ref_out=ref_out, ref_arena=ref_arena, dplace=dplace,
                           dwhere=dwhere, pairs=pairs)


def tcpcut_case(seam, size, seam_at, strided):
    """tcp_segment_emit: header templates NEAR and FAR, the payload sources back to back across the seam in the
    same arena (send 7's crosses it), the frame runs NEAR, FAR and across the seam in the other (send 8's, the
    seam between two frames or inside one); MSS 1460, frames back to back or 1565 bytes apart."""
    from types import SimpleNamespace

    from tests import tcp_segment_ref as T

    rng = np.random.default_rng(80 + strided + 2 * len(seam_at))
    n = 96
    recs = [T.template(rng, v6=bool(i & 1), doff=(5, 8, 15)[i % 3], flags=0x19, seq=int(rng.integers(0, 1 << 32))) for i in range(n)]
    lens_p = np.array([int(rng.choice([0, 1, 1459, 1460, 1461, 4000, 7300, 9000])) for _ in range(n)], np.int64)
    lens_p[7] = lens_p[8] = 7300
    lay = Layout(seam, size, rng)
    s_compact, s_far, swhere, splace, s_total = chain_slots_compact(seam, size, lens_p, 7, "inside", rng, lay)
    case = desc_case(seam, size, recs, E.KIND_IP, 81, (NEAR, FAR_LO, FAR_HI), lay=lay)
    src = rng.integers(0, 256, s_total + 16, dtype=np.uint8)
    placed, flags = _placed(case), np.zeros(n, np.uint8)  # (shuffled: send i is the batch's template i, payload range i)
    stride = 1565 if strided else 0
    make = lambda o, c, so=s_compact: E.make_tcpplans(so, lens_p, 1460, o, c)
    exp = lambda pl, sz: T.expected(placed, case.kinds, flags, pl, src, stride, NOCAPS, sz)
    far, need, dwhere, dplace, ref_out, ref_arena, _ = _cut_layout(
        seam, size, rng, lambda: exp(make(np.zeros(n), 0), 1)[0], make, exp, stride, lambda sz: 8, seam_at)
    assert (ref_out["written"] == 1).all() and swhere[7] == STRADDLE and dwhere[8] == STRADDLE
    pairs = pairs_present(swhere[lens_p > 0], dwhere[lens_p > 0])
    assert BASE_PAIRS <= pairs_present(case.where, dwhere) and BASE_PAIRS <= pairs
    return SimpleNamespace(case=case, plans=make(far, need, s_far), stride=stride, ref_out=ref_out, ref_arena=ref_arena,
                           dplace=dplace, src=src[:s_total], splace=splace, pairs=pairs)


def fraggroups_case(seam, size, seam_at, ng=12, lo=2300, hi=4000):
    """The drop-in route of tests/test_gpu_fragments.py on the sparse layout: test_frag_cpu.tx_pair cuts ng
    datagrams (UDP, TCP, ICMP echo, ICMP error; five fragments and more) at MTU 576 into offloaded fragments (no checksum filled) and
    the reference's emit-whole-then-fragment; each group's fragments, shuffled, lie NEAR, STRADDLE and FAR at
    once.  emit_frag over the offloaded records must give the reference fragments, verify_frag accept them
    all, and verify_reassemble deliver every datagram into slots back to back across the seam: the straddling
    fragment's group's slot straddles ("inside") or ends at seam - 1 ("end")."""
    from types import SimpleNamespace

    from tests import reassemble_ref as R
    from tests import test_frag_cpu as FC

    rng = np.random.default_rng(90 + len(seam_at))
    off, ref, groups = FC.tx_pair(FC.datagrams(rng, ng, lo, hi), 576, shuffle_rng=rng)
    case = desc_case(seam, size, off, E.KIND_IP, 91, shuffle=False, straddle_below=300)
    n = case.n
    assert int(np.flatnonzero(case.where == STRADDLE)[0]) < groups[0][1]
    for f, c in groups:  # every group mixes the placements
        assert {NEAR, FAR_LO, FAR_HI} <= set(case.where[f:f + c].tolist())
    gh = E.make_groups([g[0] for g in groups], [g[1] for g in groups])
    emitted = case.raw.copy()  # the reference's fragments where the offloaded ones stand
    for o, r in zip(case.offs, ref):
        emitted[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    after = case.raw.copy()
    ref_est = oracle.batch_emit_frag(after, case.desc, n, gh)
    assert np.array_equal(after, emitted) and not ref_est.any(), "the oracle's group emit is emit-whole-then-fragment"
    accepted_enough(case.where, _changed(case, case.raw, emitted), "emit_frag")
    ref_st = oracle.batch_verify_frag(emitted.copy(), case.desc, n, gh)
    assert (ref_st & E.ST_ACCEPT).all()
    placed, flags, g3 = _placed(case, emitted), np.zeros(n, np.uint8), [g + (0,) for g in groups]
    slot_caps = R.expected(placed, case.kinds, flags, g3, np.zeros(ng, np.uint64), np.zeros(ng, np.int64), 1)[0]["len"].astype(np.int64)
    compact, far, dwhere, dplace, total = chain_slots_compact(seam, size, slot_caps, 0, seam_at, rng)
    ref_dg, ref_arena = R.expected(placed, case.kinds, flags, g3, compact, slot_caps, total + 16)
    assert (ref_dg["copied"] == 1).all() and {NEAR, FAR_LO} <= set(np.where(dwhere == FAR_HI, FAR_LO, dwhere).tolist())
    assert dwhere[0] == (STRADDLE if seam_at == "inside" else NEAR)
    return SimpleNamespace(case=case, groups=gh, emitted=emitted, ref_est=ref_est, ref_st=ref_st, ref_dg=ref_dg,
                           ref_arena=ref_arena[:total], dplace=dplace, slots=E.make_slots(far, slot_caps), dwhere=dwhere)


def nhc_case(seam, size, kat: bytes, kat_addrs):
    """nhc_udp_verify / nhc_udp_emit: the reference's own datagram across the seam and FAR with small and with
    large low words, random datagrams of every port mode in the three placements."""
    from types import SimpleNamespace

    rng = np.random.default_rng(95)
    recs = [P.nhc_udp(rng, i % 4, bool((i >> 2) & 1), int(rng.integers(0, 2000))) for i in range(200)]
    addrs = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    for i in (1, 2, 3):
        recs[i], addrs[i] = kat, np.frombuffer(kat_addrs, np.uint8)
    case = desc_case(seam, size, recs, E.KIND_RAW, 96, shuffle=False, straddle_index=1, straddle_below=len(kat) // 2)
    n = case.n
    assert case.where[:4].tolist() == [NEAR, STRADDLE, FAR_LO, FAR_HI]
    pre = case.raw.copy()  # emit's input: the KAT's inline checksum (bytes 5 and 6) zeroed
    for i in (1, 2, 3):
        pre[int(case.offs[i]) + 5:int(case.offs[i]) + 7] = 0
    after = pre.copy()
    ref_est = oracle.batch_nhc_udp_emit(after, case.desc, n, addrs)
    assert all(bytes(after[int(case.offs[i]):int(case.offs[i]) + len(kat)]) == kat for i in (1, 2, 3))
    accepted_enough(case.where, _changed(case, pre, after), "nhc_udp_emit")
    bad = after.copy()  # verify's input: every fifth record but the KATs with one bit flipped
    for i in range(4, n, 5):
        if case.lens[i]:
            bad[int(case.offs[i]) + int(case.lens[i]) - 1] ^= 0x10
    ref_st = oracle.batch_nhc_udp_verify(bad.copy(), case.desc, n, addrs)
    accepted_enough(case.where, (ref_st & E.ST_ACCEPT) != 0, "nhc_udp_verify")
    assert ((ref_st & E.ST_ACCEPT) == 0).any() and (ref_st[1:4] & E.ST_ACCEPT).all()
    return SimpleNamespace(case=case, addrs=addrs, pre=pre, after=after, ref_est=ref_est, bad=bad, ref_st=ref_st)
