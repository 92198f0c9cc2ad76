"""The sparse-arena case of verify_unreach_reply: tests/far.py's rig (imported, not restated) with refused
datagrams NEAR, across and past the seam and their error frames' slots back to back across it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import unreach_ref as R
from tests.far import (BASE_PAIRS, FAR_HI, FAR_LO, NEAR, NOCAPS, STRADDLE, V4A, V4B, V6A, V6B, Layout, _placed,
                       accepted_enough, chain_slots_compact, desc_case, eth_frame, pairs_present)

OPEN, CLOSED = 53, 4000
PORTS = E.make_port_map([OPEN])


def unreach_case(seam, size, kind, seam_at):
    """verify_unreach_reply: UDP datagrams to a closed port and packets of an unhandled protocol / next header,
    IPv4 and IPv6, P around both cuts, two in three FAR; every 17th a datagram to an open port (nothing written).
    The error frames' slots lie back to back across the seam: the straddling datagram's frame straddles
    ("inside") or ends at seam - 1 ("end"), or a FAR datagram's frame straddles ("far-inside").  The port map
    lies in the records' arena past the seam, at map_far."""
    rng = np.random.default_rng(150 + kind + len(seam_at))
    recs = []
    for i in range(180):
        plen = int(rng.choice([8, 9, 23, 24, 25, 64, 527, 528, 529, 1191, 1192, 1193, 1472]))
        port = bool(i % 4)
        pay = P.udp(int(rng.integers(1, 65536)), CLOSED, P.rand_bytes(rng, plen - 8)) if port else P.rand_bytes(rng, plen)
        proto = 17 if port else 47
        recs.append(P.ipv4(V4A, V4B, proto, pay, ttl=1 + i) if i % 3 else P.ipv6(V6A, V6B, proto, pay, hop=1 + i))
    for i in range(7, 180, 17):  # an open port: nothing written
        recs[i] = P.ipv4(V4A, V4B, 17, P.udp(7, OPEN, P.rand_bytes(rng, 50)))
    recs[13] = P.ipv4(V4A, V4B, 17, P.udp(9, CLOSED, P.rand_bytes(rng, 600)))  # the one that straddles, cut in its IP header
    if kind == E.KIND_ETH:
        recs = [eth_frame(r) for r in recs]
    lay = Layout(seam, size, np.random.default_rng(152))  # shared: the port map lies in the records' arena, FAR
    case = desc_case(seam, size, recs, kind, 151, (FAR_LO, STRADDLE, FAR_HI, NEAR, FAR_LO, FAR_HI), flip_every=9,
                     straddle_index=13, straddle_below=30, lay=lay)
    map_far = lay.place(FAR_HI, 8192, gap=5)
    assert map_far >= seam
    placed, flags = _placed(case, case.compact), np.zeros(case.n, np.uint8)
    need = np.asarray(R.frame_lens(placed, case.kinds, flags, PORTS, None), np.int64)
    pivot = int(np.flatnonzero(case.where == (FAR_HI if seam_at == "far-inside" else STRADDLE))[0])
    assert need[pivot] >= 2
    compact, far, dwhere, dplace, total = chain_slots_compact(seam, size, need, pivot, seam_at.split("-")[-1], rng)
    ref_st, ref_ent, ref_arena = R.expected(placed, case.kinds, flags, NOCAPS, None, PORTS, E.make_slots(compact, need), total + 16)
    assert np.array_equal(ref_st, case.ref_verify())
    written = (ref_ent["flags"] & R.WRITTEN) != 0
    accepted_enough(case.where, written, "refused datagrams")
    accepted_enough(dwhere, written, "error frame slots")
    pairs = pairs_present(case.where[written], dwhere[written])
    assert {"inside": (STRADDLE, STRADDLE), "end": (STRADDLE, NEAR), "far-inside": (FAR_LO, STRADDLE)}[seam_at] in pairs
    assert BASE_PAIRS <= pairs
    assert ((ref_ent["flags"] & R.SEND) != 0).sum() >= 100 and (written & ((ref_ent["flags"] & R.SEND) == 0)).any()
    assert (ref_ent["flags"] == 0).any() and ((ref_ent["flags"] & R.PORT) != 0).any() and (ref_ent["flags"] == R.REFUSED | R.ANSWERED | R.WRITTEN | R.SEND).any()
    return SimpleNamespace(case=case, ref_st=ref_st, ref_ent=ref_ent, ref_arena=ref_arena[:total], dplace=dplace,
                           slots=E.make_slots(far, need), dwhere=dwhere, pairs=pairs, ports=PORTS, map_far=map_far)
