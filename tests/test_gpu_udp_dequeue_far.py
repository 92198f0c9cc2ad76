"""udp_dequeue_emit with 64-bit offsets at and past 4 GiB, on the sparse arenas of tests/far.py: the sockets' payload
rings NEAR, across, exactly at and past 2^32 in the first arena, which is also d_meta (meta_first * 48 passes 2^32);
their frame areas NEAR, across, exactly at and past it in the second arena, which is also d_tx (tx_first * 16 passes
2^32).  The case is built compactly (tests/test_gpu_udp_dequeue.py's Tx), answered by tests/udp_dequeue_ref.py
there, and moved: d_tx entries and group entries do not depend on position and are compared as they are, both
arenas are scanned for strays.  The module skips only when the device has less than 12 GiB free."""
import numpy as np
import pytest

from tests import far as F
from tests import udp_dequeue_ref as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.test_gpu_far_offsets import SEAM, SIZE, _dev, _pre, rig  # noqa: E402,F401  (rig: this module's own)
from tests.test_gpu_udp_dequeue import ETH, Tx, rnd, v6  # noqa: E402

SIZES = (1472, 33, 700, 0, 1)
P_, M, PR = 4096, 6, 100


def _compact():
    """Four sockets of five datagrams each, IPv4 and IPv6, two with an Ethernet header: (Tx, built arrays, model)."""
    tx = Tx()
    for g in range(4):
        pay = rnd(60 + g, *SIZES)
        tx.add([p if (g + j) % 2 else v6(p) for j, p in enumerate(pay)], P_=P_, M=M, pr=PR, mr=g, mtu=1520,
               eth=ETH if g % 2 else None)
    built = tx.build()
    src, socks, meta, dst_size, tx_size = built
    return tx, built, D.expected(src, socks, meta, (0, 0, 0, 0, 0), 0, dst_size, tx_size)


def _aligned(lay, where, n, unit):
    """An object of n bytes at a multiple of `unit` bytes."""
    o = lay.place(where, n + unit)
    return (o + unit - 1) // unit * unit


@pytest.mark.parametrize("seam_at", ["payload", "at", "head"])
def test_udp_dequeue_rings_and_frames_across_the_seam(rig, seam_at):  # noqa: F811
    """payload: 2^32 falls inside a payload of socket 1's ring and inside a frame's payload of socket 2's area;
    at: socket 1's src_offset and dst_offset are 2^32 exactly, socket 3's ring and frames end at 2^32 - 1;
    head: 2^32 falls between two payloads of socket 1's ring and inside a frame's head of socket 2's area."""
    eng = rig.eng.prod
    tx, (src, socks, meta, _, _), exp = _compact()
    rng = np.random.default_rng(7)
    need = [int(s["dst_cap"]) for s in socks]
    flen = [[len(f[3]) for f in exp["frames"] if f[0] == g] for g in range(4)]
    layA, layB = F.Layout(SEAM, SIZE, rng), F.Layout(SEAM, SIZE, rng)
    src_far, dst_far = [0] * 4, [0] * 4
    if seam_at == "at":
        base = layA.straddle(2 * P_, P_)
        src_far[3], src_far[1] = base, base + P_
        base = layB.straddle(need[3] + need[1], need[3])
        dst_far[3], dst_far[1] = base, base + need[3]
        assert src_far[1] == SEAM == dst_far[1]
        rest = {0: F.NEAR, 2: F.FAR_HI}
    else:
        src_far[1] = layA.straddle(P_, PR + (700 if seam_at == "payload" else SIZES[0]))
        dst_far[2] = layB.straddle(need[2], flen[2][0] + (flen[2][1] - 10 if seam_at == "payload" else 20))
        rest = {0: F.NEAR, 3: F.FAR_HI}
    for g, w in rest.items():
        src_far[g], dst_far[g] = layA.place(w, P_), layB.place(w, need[g])
    for g in range(4):
        if not src_far[g]:
            src_far[g] = layA.place(F.FAR_LO, P_)
        if not dst_far[g]:
            dst_far[g] = layB.place(F.FAR_LO, need[g])
    meta_far = [_aligned(layA, w, 48 * M, 48) // 48 for w in (F.NEAR, F.FAR_LO, F.FAR_HI, F.FAR_LO)]
    tx_far = [_aligned(layB, w, 16 * 5, 16) // 16 for w in (F.NEAR, F.FAR_HI, F.FAR_LO, F.FAR_HI)]
    assert max(meta_far) > SEAM // 48 and max(tx_far) > SEAM // 16

    far = socks.copy()
    far["src_offset"], far["dst_offset"], far["meta_first"], far["tx_first"] = src_far, dst_far, meta_far, tx_far
    a_ext, b_ext = [], []
    for g in range(4):
        so, mf = int(socks[g]["src_offset"]), int(socks[g]["meta_first"])
        a_ext.append((src_far[g], src[so:so + P_].copy()))
        a_ext.append((48 * meta_far[g], meta[mf:mf + M].view(np.uint8).copy()))
        t0 = int(socks[g]["tx_first"])
        b_ext.append((16 * tx_far[g], exp["tx"][t0:t0 + 5].view(np.uint8).copy()))
        do = int(socks[g]["dst_offset"])
        b_ext += [(dst_far[g] + f[2] - do, np.frombuffer(f[3], np.uint8)) for f in exp["frames"] if f[0] == g]
    rig.a.refill()
    rig.b.refill()
    for lo, data in a_ext:
        rig.a.put(lo, data)
    assert rig.a.buf.data_ptr() % 16 == 0 and rig.b.buf.data_ptr() % 16 == 0
    far_dev = _dev(far)
    _, out = eng.udp_dequeue_emit(rig.a.buf, far_dev, rig.a.buf, rig.b.buf, 0, tx=rig.b.buf, out=_pre(4, 32))
    launched = eng.last_launch()
    assert launched["kernel"] == "udptx_kernel", launched
    got_out = out.cpu().numpy().reshape(-1).view(E.UDPTXOUT_DTYPE)
    assert np.array_equal(got_out, exp["outs"]), (got_out, exp["outs"])
    assert got_out["sent"].tolist() == [5] * 4
    assert np.array_equal(far_dev.cpu().numpy(), far.view(np.uint8)), "d_socks is only read"
    rig.b.check(b_ext)
    rig.a.check(a_ext)  # d_src and d_meta, which is this arena: only read
    print(f"far udp_dequeue_emit {seam_at}: src {[hex(x) for x in src_far]}, dst {[hex(x) for x in dst_far]}")
