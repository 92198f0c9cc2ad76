"""GPU parity of tcp_segment_emit (smol_csum_batch_tcp_segment_emit): TCP sends cut into MSS-sized segments
behind their header template, every checksum filled, in one pass over the payload.

Every case compares, exactly:
  1. the smol_csum_tcpout_t entries with tests/tcp_segment_ref.py (oracle.batch_emit's status byte included);
  2. the WHOLE destination arena, filled with the sentinel 0xA5 beforehand, with the helper's: a stray store
     or a missing byte anywhere fails;
  3. the batch buffer and the payload source with what was uploaded: they are only read;
and checks that the launch recorded is tcpcut_kernel.
"""
import numpy as np
import pytest

from tests import cut_ref as R
from tests import pktgen as P
from tests import tcp_segment_ref as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def _run(eng, sends, stride=0, caps=NOCAPS, fixed=None, start=3, cap_adj=0, src_mod=None, seed=0):
    """One tcp_segment_emit call, compared exactly.  sends: (record, kind, flags, mss, len) each; fixed:
    (record stride, base offset) for a fixed-stride batch, else a descriptor batch with random gaps (odd
    offsets).  The payload ranges lie back to back in d_src, the first at its first byte and the last ending
    at its last (src_mod: each range's offset mod 16 instead, gaps as needed).  Slots lie back to back from
    `start`, each as large as its send needs; cap = that + cap_adj (one for all or one per send).  Returns
    (out entries, arena, slot offsets, plans)."""
    n = len(sends)
    recs = [s[0] for s in sends]
    kinds = np.array([s[1] for s in sends], np.uint8)
    flags_a = np.array([s[2] for s in sends], np.uint8)
    msss = np.array([s[3] for s in sends], np.uint16)
    lens_p = np.array([s[4] for s in sends], np.int64)
    rng = np.random.default_rng(seed)
    buf, offs, lens, placed = R.place_records(recs, kinds, flags_a, fixed, rng)
    so, pos = [], 0
    for i in range(n):
        if src_mod is not None:
            pos += (int(src_mod[i]) - pos) % 16
        so.append(pos)
        pos += int(lens_p[i])
    src = rng.integers(0, 256, max(pos, 1), dtype=np.uint8)

    def make_plans(dst_offsets, dst_caps):
        plans = E.make_tcpplans(so, lens_p, msss, dst_offsets, dst_caps)
        plans["reserved"], plans["reserved2"] = 0xDEAD, 0xDEADBEEF  # the kernel ignores them
        return plans

    plans, slots, ref_out, ref_arena = R.plan_slots(
        n, make_plans, lambda pl, size: T.expected(placed, kinds, flags_a, pl, src, stride, caps, size), stride, start, cap_adj)
    batch, d, dv, dst, pd = R.upload(E, buf, offs, lens, kinds, flags_a, fixed, plans, ref_arena.size)
    ds = torch.from_numpy(src.copy()).cuda()
    out = eng.tcp_segment_emit(dv, batch, ds, dst, pd, frame_stride=stride, caps=caps)
    got_out, got_dst = R.compare(eng, "tcpcut_kernel", out, dst, ref_out, ref_arena,
                                 [(d, buf, "the batch buffer"), (ds, src, "the payload source")])
    return got_out, got_dst, slots, plans


# ---- 1. the size sweep ---------------------------------------------------------------------------

def _sweep_lens(mss):
    ls = [0, 1, mss - 1, mss, mss + 1, 2 * mss, 5 * mss + 3]
    return [x for x in ls if mss != 1 or x <= 40]


@pytest.mark.parametrize("stride", [0, 1601, 1600])
@pytest.mark.parametrize("form", ["desc", "fixed"])
def test_size_sweep(eng, form, stride):
    """mss in {1, 7, 16, 536, 1460} x the payload lengths around 0, 1, 2 and 5 segments, IPv4 and IPv6, with
    and without Ethernet, data offset 5, 8 and 15; frames back to back (frame_stride 0), at an odd stride
    above every frame length here and at a multiple of 64."""
    rng = np.random.default_rng(stride + (form == "fixed"))
    for eth in (False, True):
        kind = E.KIND_ETH if eth else E.KIND_IP
        sends = [(T.template(rng, v6=v6, eth=eth, doff=doff, flags=0x19, seq=int(rng.integers(0, 1 << 32))), kind, 0, mss, ln)
                 for mss in (1, 7, 16, 536, 1460) for ln in _sweep_lens(mss) for v6 in (False, True) for doff in (5, 8, 15)]
        out, _, _, _ = _run(eng, sends, stride=stride, fixed=(117, 5) if form == "fixed" else None, seed=stride + eth)
        assert (out["written"] == 1).all() and (out["status"] == 0).all()
        assert out["count"].tolist() == [max(1, -(-s[4] // s[3])) for s in sends]


# ---- 2. every alignment --------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [0, 79])
def test_every_source_and_destination_alignment(eng, stride):
    """256 sends: the source offsets take every value mod 16 against every destination offset mod 16 (slots
    back to back whose sizes are 1 mod 16); mss 37 is odd, so the slices' source parity alternates, and with
    frames of 77 bytes so do the frames' alignments."""
    rng = np.random.default_rng(5)
    ln = 129 if stride == 0 else 123  # 4 frames: 4 * 40 + 129 = 289, 3 * 79 + 40 + 12 = 289
    sends = [(T.template(rng, seq=int(rng.integers(0, 1 << 32))), E.KIND_IP, 0, 37, ln) for _ in range(256)]
    out, _, slots, plans = _run(eng, sends, stride=stride, start=0, src_mod=[i // 16 for i in range(256)])
    assert {(int(p["src_offset"]) % 16, int(p["dst_offset"]) % 16) for p in plans} == {(a, b) for a in range(16) for b in range(16)}
    assert (out["count"] == 4).all() and (out["written"] == 1).all()


# ---- 3. values -----------------------------------------------------------------------------------

def test_sequence_wrap(eng):
    rng = np.random.default_rng(6)
    sends = [(T.template(rng, v6=v6, seq=0xFFFFFF00), E.KIND_IP, 0, 100, 1000) for v6 in (False, True)]
    _, arena, slots, _ = _run(eng, sends)
    seqs = [int.from_bytes(arena[int(slots[0]) + 140 * k + 24:int(slots[0]) + 140 * k + 28].tobytes(), "big") for k in range(10)]
    assert seqs == [(0xFFFFFF00 + 100 * k) & 0xFFFFFFFF for k in range(10)] and seqs[3] == 0x2C


def test_flags(eng):
    """FIN / PSH only on the last frame, every other flag bit (NS in the data offset byte included) on all."""
    rng = np.random.default_rng(7)
    cases = [(0x10, False), (0x18, False), (0x19, False), (0xF9, True)]
    sends = [(T.template(rng, flags=fl, ns=ns), E.KIND_IP, 0, 64, 64 * 3 + 1) for fl, ns in cases]
    _, arena, slots, _ = _run(eng, sends)
    for (fl, ns), s in zip(cases, slots):
        for k in range(4):
            f = arena[int(s) + 104 * k:]
            assert f[33] == (fl if k == 3 else fl & ~0x09) and f[32] == (0x51 if ns else 0x50)


@pytest.mark.parametrize("ipv4_caps", [0, 1, 2, 3])
def test_every_caps_combination(eng, ipv4_caps):
    """caps.ipv4 x caps.tcp over {Both, Rx, Tx, None}."""
    rng = np.random.default_rng(10 + ipv4_caps)
    sends = [(T.template(rng, v6=v6, eth=eth, doff=7), E.KIND_ETH if eth else E.KIND_IP, 0, 536, ln)
             for v6 in (False, True) for eth in (False, True) for ln in (0, 1300)]
    for tcp in range(4):
        _run(eng, sends, caps=(ipv4_caps, 3 - tcp, tcp, 0, 0), seed=tcp)


# ---- 4. records that are not cut -----------------------------------------------------------------

def test_records_not_cut_neighbours_served(eng):
    rng = np.random.default_rng(12)
    sends = []
    cases = T.not_cut_cases(rng)
    for _, rec, kind, flags, mss, ln in cases:
        sends += [(T.template(rng), E.KIND_IP, 0, 536, 1000), (rec, kind, flags, mss, ln),
                  (T.template(rng, v6=True, eth=True, doff=6), E.KIND_ETH, 0, 1460, 1461)]
    out, _, _, _ = _run(eng, sends, cap_adj=np.where(np.arange(len(sends)) % 3 == 1, 1 << 20, 0))
    assert (out["count"][1::3] == 0).all() and (out["written"][1::3] == 0).all() and (out["frame_len"][1::3] == 0).all()
    assert (out["count"][0::3] == 2).all() and (out["written"][0::3] == 1).all() and (out["written"][2::3] == 1).all()
    assert {int(s) for s in out["status"][1::3]} == {0, E.ST_MALFORMED, E.ST_UNSUPPORTED}
    # the same kinds in a fixed-stride batch of their own kind and flags
    for k, f in ((E.KIND_IP, 0), (E.KIND_ETH, 0), (E.KIND_RAW, 0), (E.KIND_IP, E.REC_IPHDR_ONLY)):
        sub = [(T.template(rng, eth=k == E.KIND_ETH), k, f, 536, 600)] + [c[1:] for c in cases if c[2] == k and c[3] == f]
        _run(eng, sub, fixed=(128, 1))


# ---- 5. cap and stride ---------------------------------------------------------------------------

def test_cap_one_byte_short_and_stride_below_frame_len(eng):
    rng = np.random.default_rng(13)
    lens = (1000, 3000, 536, 537, 100, 0, 5000, 540, 1072, 1073, 2000, 500)
    sends = [(T.template(rng, v6=bool(i % 2), doff=5 + i % 3), E.KIND_IP, 0, 536, ln) for i, ln in enumerate(lens)]
    short = np.where(np.arange(len(sends)) % 2 == 0, -1, 0)
    out, arena, _, _ = _run(eng, sends, cap_adj=short)
    assert out["written"].tolist() == [0, 1] * 6 and (out["count"] > 0).all()
    out, arena, _, _ = _run(eng, sends, cap_adj=-1)
    assert (out["written"] == 0).all() and (arena == T.SENTINEL).all() and (out["frame_len"] > 0).all()
    # a stride of 575 is below the frame length of every send with a full first segment (at least 40 + 536)
    out, arena, _, _ = _run(eng, sends, stride=575, cap_adj=10000)
    assert out["written"].tolist() == [int(fl) <= 575 for fl in out["frame_len"]] and out["written"].sum() == 3
    # 599: between the IPv6 frame lengths 596 (data offset 5) and 600 (6); gaps keep the sentinel
    out, _, _, _ = _run(eng, sends, stride=599, cap_adj=short)
    assert out["written"].tolist() == [int(fl) <= 599 and i % 2 == 1 for i, fl in enumerate(out["frame_len"])]
    assert out["written"].sum() == 4


# ---- 6. sizes ------------------------------------------------------------------------------------

def test_largest_frame(eng):
    """mss 65495 behind IPv4 and a 20-byte TCP header: total length 65535; three frames."""
    rng = np.random.default_rng(14)
    sends = [(T.template(rng), E.KIND_IP, 0, 536, 700), (T.template(rng), E.KIND_IP, 0, 65495, 2 * 65495 + 1),
             (T.template(rng, v6=True, eth=True), E.KIND_ETH, 0, 1460, 99)]
    out, _, _, _ = _run(eng, sends)
    assert out["count"].tolist() == [2, 3, 1] and int(out[1]["frame_len"]) == 65535 and (out["written"] == 1).all()


def test_slices_around_one_step_of_128_chunks(eng):
    """Slices of 2016 to 2049 bytes at every source alignment: 126 to 130 source chunks, around what one
    step of the kernel holds (64 lanes x 2 chunks, with and without the extra leading slot of a destination
    shift): where a frame starts to take a second step."""
    rng = np.random.default_rng(17)
    sends = [(T.template(rng, v6=bool(a & 1), seq=int(rng.integers(0, 1 << 32))), E.KIND_IP, 0, mss, 2 * mss + 1)
             for mss in (2016, 2017, 2018, 2031, 2032, 2033, 2048, 2049) for a in range(16)]
    out, _, _, _ = _run(eng, sends, src_mod=[i % 16 for i in range(len(sends))])
    assert (out["count"] == 3).all() and (out["written"] == 1).all()


def test_many_sends_grid_stride(eng):
    """More sends than one workgroup holds, count not a multiple of 4, 1 to 3 segments each."""
    rng = np.random.default_rng(15)
    sends = []
    for i in range(203):
        eth, v6 = bool(i & 1), bool(i & 2)
        mss = (536, 1460, 89)[i % 3]
        sends.append((T.template(rng, v6=v6, eth=eth, doff=5 + i % 11, seq=int(rng.integers(0, 1 << 32))),
                      E.KIND_ETH if eth else E.KIND_IP, 0, mss, 1 + (i * 37) % (3 * mss)))
    out, _, _, _ = _run(eng, sends)
    assert set(out["count"].tolist()) == {1, 2, 3} and (out["written"] == 1).all()


# ---- 7. against the calls that exist -------------------------------------------------------------

def test_cross_check_copy_emit_and_verify(eng):
    """64 sends at mss 1460 into a dense fixed-stride arena (frame_stride = hl + mss): the frames equal what
    copy_emit writes from host-built headers plus the same payload, and verify accepts every frame."""
    rng = np.random.default_rng(16)
    n, mss, hl = 64, 1460, 14 + 20 + 32
    S = hl + mss
    recs = [T.template(rng, eth=True, doff=8, flags=0x19, seq=int(rng.integers(0, 1 << 32))) for _ in range(n)]
    lens_p = rng.integers(1, 4 * mss + 1, n)
    counts = -(-lens_p // mss)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    nf = int(counts.sum())
    so = np.concatenate([[0], np.cumsum(lens_p)[:-1]])
    src = rng.integers(0, 256, int(lens_p.sum()), dtype=np.uint8)
    buf, offs, lens = P.pack(recs, gap_rng=rng)
    plans = E.make_tcpplans(so, lens_p, mss, firsts * S, counts * S)
    ds = torch.from_numpy(src).cuda()
    dst = torch.zeros(nf * S, dtype=torch.uint8, device="cuda")
    out = eng.tcp_segment_emit(torch.from_numpy(buf).cuda(), E.Batch.from_records(offs, lens, E.KIND_ETH, "cuda:0"), ds, dst,
                               torch.from_numpy(plans.view(np.uint8).copy()).cuda(), frame_stride=S)
    assert eng.last_launch()["kernel"] == "tcpcut_kernel"
    out = out.cpu().numpy().reshape(-1).view(E.TCPOUT_DTYPE)
    assert out["count"].tolist() == counts.tolist() and (out["written"] == 1).all() and (out["status"] == 0).all()
    # the caller's route without the call: headers built on the host, one copy descriptor per segment
    host = np.zeros(nf * S, np.uint8)
    c_src, c_len = [], []
    for i in range(n):
        seq0 = int.from_bytes(recs[i][38:42], "big")
        for k in range(int(counts[i])):
            pk = min(mss, int(lens_p[i]) - k * mss)
            h = bytearray(recs[i][:hl])
            h[16:18] = (20 + 32 + pk).to_bytes(2, "big")
            h[38:42] = ((seq0 + k * mss) & 0xFFFFFFFF).to_bytes(4, "big")
            if k + 1 < counts[i]:
                h[47] &= ~0x09 & 0xFF
            o = (int(firsts[i]) + k) * S
            host[o:o + hl] = np.frombuffer(bytes(h), np.uint8)
            c_src.append(int(so[i]) + k * mss)
            c_len.append(pk)
    frames = E.Batch.from_records(np.arange(nf, dtype=np.uint64) * S, hl + np.array(c_len, np.uint32), E.KIND_ETH, "cuda:0")
    dst2 = torch.from_numpy(host).cuda()
    eng.copy_emit(dst2, frames, ds, torch.from_numpy(E.make_copies(c_src, hl, c_len).view(np.uint8).copy()).cuda())
    assert torch.equal(dst, dst2)
    st = eng.verify(dst, E.Batch.fixed(nf, S, S, E.KIND_ETH))
    assert bool((st & E.ST_ACCEPT).all())


def test_no_records_launches_nothing(eng):
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    eng.emit(buf, E.Batch.fixed(2, 64, 64, E.KIND_IP))
    before = eng.last_launch()
    assert before["kernel"] != "tcpcut_kernel"
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    out = eng.tcp_segment_emit(buf, E.Batch.fixed(0, 64, 64, E.KIND_IP), buf, buf, empty)
    assert out.numel() == 0 and eng.last_launch() == before
