"""The sparse-arena case of verify_udp_enqueue: tests/far.py's rig (imported, not restated) with the sockets'
frames NEAR, across and past the seam, their payload rings NEAR, across and past it, and their metadata rings
in the rings' arena on both sides of it (d_meta is the arena's base: meta_first * 48 passes the seam)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import udp_enqueue_ref as R
from tests.far import (DST_FILL, FAR_HI, FAR_LO, NEAR, STRADDLE, V4A, V4B, V6A, V6B, Layout, Placement, _placed,
                       accepted_enough, desc_case, pairs_present)

PORT, RL, M, CUT = 5000, 8000, 8, 3000  # the straddling ring has CUT of its RL bytes below the seam
SIZES = (1472, 700, 1, 1472, 333, 1472)
# (payload_read, payload_len, meta_read, meta_len) of the four sockets: each puts a payload across ring offset CUT
STATES = ((2000, 350, 0, 0), (7000, 500, 6, 1), (0, 2500, 3, 2), (2990, 0, 7, 0))


def udp_frame(payload, sport, v6=False):
    """One Ethernet / IP / UDP frame to PORT, checksums 0 (the oracle's emit fills them)."""
    u = P.udp(sport, PORT, payload)
    return P.eth(P.ipv6(V6A, V6B, 17, u), 0x86DD) if v6 else P.eth(P.ipv4(V4A, V4B, 17, u))


def udprx_case(seam, size, rot):
    """verify_udp_enqueue: four sockets of six datagrams whose frames lie NEAR, STRADDLE and FAR in each group,
    every seventh record corrupted (one per group, at another position in each: its followers are RESTORED).  One
    payload ring straddles the seam at ring offset CUT, the others lie NEAR, FAR_LO and FAR_HI; rot moves the
    socket that holds the straddling frame to the straddling / the FAR / the NEAR ring.  Every socket's state
    puts a payload across ring offset CUT, so on the straddling ring a payload's range straddles the seam."""
    rng = np.random.default_rng(170 + rot)
    recs, groups = [], []
    for g in range(4):
        first = len(recs)
        recs.extend(udp_frame(P.rand_bytes(rng, s), 4000 + len(recs), v6=bool((g + j) & 1)) for j, s in enumerate(SIZES))
        groups.append((first, len(SIZES)))
    n = len(recs)
    case = desc_case(seam, size, recs, E.KIND_ETH, 171 + rot, shuffle=False, straddle_below=700, flip_every=7)
    assert int(np.flatnonzero(case.where == STRADDLE)[0]) < groups[0][1]  # the straddling frame is socket 0's
    ref_st = case.ref_verify()
    assert ((ref_st & E.ST_ACCEPT) == 0).sum() == 4
    dst0 = [3 + g * (RL + 11) for g in range(4)]
    socks = E.make_udpsocks(dst0, [1 + g * (M + 1) for g in range(4)], RL, [s[0] for s in STATES], [s[1] for s in STATES], M,
                            [s[2] for s in STATES], [s[3] for s in STATES], PORT)
    exp = R.expected(_placed(case, case.compact), case.kinds, np.zeros(n, np.uint8), [g + (0,) for g in groups], socks, ref_st,
                     3 + 4 * (RL + 11) + 19, 1 + 4 * (M + 1))
    rx, outs = exp["rx"], exp["outs"]
    assert exp["written"].all() and (outs["valid"] == 1).all() and (outs["enqueued"] == 5).all() and outs["restored"].sum() >= 6
    assert ((rx["flags"] & E.URX_PADDED) != 0).any()
    lay = Layout(seam, size, rng)
    ring_far = {0: lay.straddle(RL, CUT)}
    ring_far.update({1: lay.place(NEAR, RL), 2: lay.place(FAR_LO, RL), 3: lay.place(FAR_HI, RL)})
    ring_of = [(g - rot) % 3 if g < 3 else 3 for g in range(4)]  # socket g's ring: 0 straddles, 1 NEAR, 2 / 3 FAR
    far = [ring_far[ring_of[g]] for g in range(4)]
    # the metadata rings: 48-byte entries at multiples of 48 from the arena's base, sockets 0 and 2 past the seam
    meta_far = []
    for g in range(4):
        a = lay.place((FAR_HI, NEAR, FAR_LO, NEAR)[g], 48 * (M + 1))
        meta_far.append(-(-a // 48))
    assert 48 * meta_far[0] >= seam and 48 * meta_far[2] >= seam and 48 * meta_far[1] + 48 * M < seam
    dplace = Placement([(dst0[g], dst0[g] + RL, far[g]) for g in range(4)])
    delivered = ((rx["flags"] & E.URX_ENQUEUED) != 0) & (rx["len"] > 0)
    accepted_enough(case.where, delivered, "udp_enqueue frames")
    dwhere = np.repeat([(STRADDLE, NEAR, FAR_LO, FAR_HI)[ring_of[g]] for g in range(4)], [g[1] for g in groups])
    pairs = pairs_present(case.where[delivered], dwhere[delivered])
    assert {(a, b) for a in (NEAR, FAR_LO) for b in (NEAR, STRADDLE, FAR_LO)} <= pairs
    # a payload's range straddles the seam: the straddling ring holds payload bytes on both sides of the cut, of one record
    gs = ring_of.index(0)
    cross = [e for e in rx[groups[gs][0]:groups[gs][0] + 6] if e["flags"] & E.URX_ENQUEUED and e["ring_off"] < CUT < e["ring_off"] + e["len"]]
    assert len(cross) == 1
    socks_far = socks.copy()
    socks_far["dst_offset"] = far
    socks_far["meta_first"] = meta_far
    # the metadata entries where the arena holds them
    meta_ext = []
    for g in range(4):
        for k in range(M):
            i = 1 + g * (M + 1) + k
            if exp["meta_written"][i]:
                meta_ext.append((48 * (meta_far[g] + k), exp["meta"][i:i + 1].view(np.uint8).copy()))
    assert len(meta_ext) == int(outs["meta_len"].sum()) - sum(s[3] for s in STATES)
    return SimpleNamespace(case=case, ref_st=ref_st, exp=exp, dplace=dplace, socks=socks_far, meta_ext=meta_ext,
                           groups=E.make_groups([g[0] for g in groups], [g[1] for g in groups]), ring_of=ring_of, pairs=pairs,
                           fill=DST_FILL)


def ring_extents(c, get):
    """The rings' expected bytes where the arena holds them.  get(lo, hi) reads the arena: a byte that lies in a
    speculative range and in no accepted one may hold the speculative byte instead of the fill, and is expected
    as it is found when it holds that byte (any third value fails the arena's check)."""
    out = []
    for a, b, f in c.dplace.ext:
        want = c.exp["arena"][a:b].copy()
        only = c.exp["spec_only"][a:b]
        if only.any():
            got, spec = get(f, f + b - a), c.exp["spec_arena"][a:b]
            take = only & (got == spec)
            want[take] = spec[take]
        out.append((f, want))
    return out
