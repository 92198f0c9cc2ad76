"""What the cut calls (smol_csum_batch_fragment_emit, smol_csum_batch_tcp_segment_emit) share: the part of the
expected results that does not depend on which frames a record makes (tests/fragment_ref.py and
tests/tcp_segment_ref.py say that), and the GPU tests' rig around one call.  No checksum is computed here."""
from __future__ import annotations

import numpy as np

import oracle
from tests import pktgen as P

SENTINEL = 0xA5

# smol_csum_fragout_t and smol_csum_tcpout_t
OUT_DTYPE = np.dtype([("count", "<u4"), ("frame_len", "<u4"), ("last_len", "<u4"), ("status", "u1"), ("written", "u1"),
                      ("reserved", "<u2")])


def emit_record(rec: bytes, kind: int, flags: int, caps):
    """(status byte, record bytes) after smol_csum_batch_emit's oracle on a copy of the record."""
    a = np.frombuffer(rec, np.uint8).copy()
    if a.size == 0:
        return int(oracle.batch_emit(np.zeros(1, np.uint8), None, 1, 0, 0, oracle.kind_flags(kind, flags), caps)[0]), b""
    st = oracle.batch_emit(a, None, 1, a.size, a.size, oracle.kind_flags(kind, flags), caps)
    return int(st[0]), a.tobytes()


def new_results(n: int, arena_size: int, sentinel: int = SENTINEL):
    """(out entries, arena) before the first record: zero, and a sentinel fill that shows a stray store."""
    return np.zeros(n, OUT_DTYPE), np.full(arena_size, sentinel, np.uint8)


def place(out, arena, i: int, status: int, frames, plan, frame_stride: int):
    """Record i's entry and, when they fit, its frames in the arena.  frames: the frames the record makes
    (bytes each), None for a record that is not cut; plan: its plan entry (dst_offset, cap).  The frames lie
    frame_stride apart (0: back to back) and are stored only when all of them lie inside the cap and the
    stride is not below the frame length."""
    out[i]["status"] = status
    if frames is None:
        return
    count, frame_len, last_len = len(frames), len(frames[0]), len(frames[-1])
    assert all(len(f) == frame_len for f in frames[:-1])
    out[i]["count"], out[i]["frame_len"], out[i]["last_len"] = count, frame_len, last_len
    S = frame_stride or frame_len
    if (count - 1) * S + last_len > int(plan["cap"]) or S < frame_len:
        return
    out[i]["written"] = 1
    o = int(plan["dst_offset"])
    for k, f in enumerate(frames):
        assert o + k * S + len(f) <= arena.size
        arena[o + k * S:o + k * S + len(f)] = np.frombuffer(f, np.uint8)


# ---- the GPU tests' rig ----------------------------------------------------------------------------

def place_records(recs, kinds, flags, fixed, rng):
    """The batch buffer of a test: fixed = (record stride, base offset) puts the records at a fixed stride
    over random bytes (one kind and one flags value), None packs them for a descriptor batch with random
    gaps (odd offsets).  Returns (buf, offs, lens, placed): placed are the records as they stand in the
    batch, a fixed-stride one's trailing bytes included."""
    n = len(recs)
    if fixed is not None:
        rstride, base = fixed
        buf = rng.integers(0, 256, base + n * rstride + 64, dtype=np.uint8)
        offs = base + np.arange(n, dtype=np.uint64) * rstride
        for o, r in zip(offs, recs):
            assert len(r) <= rstride
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
        lens = np.full(n, rstride, np.uint32)
        assert (kinds == kinds[0]).all() and (flags == flags[0]).all()
    else:
        buf, offs, lens = P.pack(recs, gap_rng=rng)
    return buf, offs, lens, [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]


def plan_slots(n: int, make_plans, expected, stride: int, start: int, cap_adj):
    """Slots back to back from `start`, each as large as its record's frames need (a first pass of
    expected(plans, arena_size) over make_plans(dst_offsets, caps) with caps of 0 reports it); cap = that +
    cap_adj, one for all or one per record.  Returns (plans, slot offsets, reference entries, reference arena)."""
    size = expected(make_plans(np.zeros(n), 0), 1)[0]
    need = np.where(size["count"] > 0, (size["count"].astype(np.int64) - 1) *
                    np.where(stride, stride, size["frame_len"]).astype(np.int64) + size["last_len"], 0)
    slot = np.concatenate([[start], start + np.cumsum(need)]).astype(np.int64)
    plans = make_plans(slot[:-1], np.maximum(need + cap_adj, 0))
    return (plans, slot[:-1]) + expected(plans, int(slot[-1]) + 21)


def upload(E, buf, offs, lens, kinds, flags, fixed, plans, arena_size: int):
    """(batch, device copy of buf, the view of it the batch starts at, sentinel-filled arena, device plans)."""
    import torch

    if fixed is not None:
        batch = E.Batch.fixed(len(offs), fixed[0], fixed[0], int(kinds[0]), flags=int(flags[0]))
    else:
        batch = E.Batch.from_records(offs, lens, kinds, "cuda:0", flags=flags)
    d = torch.from_numpy(buf.copy()).cuda()
    dst = torch.full((arena_size,), SENTINEL, dtype=torch.uint8, device="cuda")
    pd = torch.from_numpy(plans.view(np.uint8).copy()).cuda()
    return batch, d, d[fixed[1]:] if fixed is not None else d, dst, pd


def compare(eng, kernel: str, out, dst, ref_out, ref_arena, read_only):
    """The assertions of every case: the launch recorded is `kernel`, every (device tensor, host array, name)
    of read_only is unchanged, the entries and the WHOLE arena equal the reference's.  Returns both, on the host."""
    launched = eng.last_launch()
    got_out = out.cpu().numpy().reshape(-1).view(OUT_DTYPE)
    got_dst = dst.cpu().numpy()
    assert launched["kernel"] == kernel, launched
    for dev, host, name in read_only:
        assert np.array_equal(dev.cpu().numpy(), host), f"{name} is only read"
    bad = np.nonzero(got_out != ref_out)[0]
    assert bad.size == 0, f"entries differ at {bad[:8]}: got {got_out[bad[:4]]} want {ref_out[bad[:4]]}"
    diff = np.nonzero(got_dst != ref_arena)[0]
    assert diff.size == 0, f"destination bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {ref_arena[diff[:8]]})"
    return got_out, got_dst
