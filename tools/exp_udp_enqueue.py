#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_udp_enqueue (a batch of received frames verified, every UDP
datagram's payload put where its socket's PacketBuffer::enqueue places it, metadata entries written, in the
same pass) next to what a caller could do before it, on device-resident data: 2^14 sockets of 45 datagrams,
2^16 sockets of 6 and 2^18 sockets of 1.  Frames are Ethernet + IPv4 + UDP with 1472-byte payloads at a fixed
stride of 1514; every socket's payload ring holds the poll, count * 1472 bytes, empty at the start, the rings
back to back; its metadata ring has count entries.

Lines per shape:
  (a) verify_copy              smol_csum_batch_verify_copy over the same records, slots precomputed by the host
                               at the same places: the second half of the route the call replaces (verify, the
                               status bytes to the host, PacketBuffer::enqueue walked there, the slots back)
  (b) verify                   smol_csum_batch_verify alone: the first half of that route, and the read floor
  (c) verify_udp_enqueue       the fused call, every datagram accepted: the layouts are equal, nothing is stored
                               twice
  (d) verify_udp_enqueue_bad   the fused call over the same frames with one corrupted datagram in the middle of
                               every group: its followers move and are stored again (the restore pass's cost)

Two more lines split (c) into its parts, on the same frames:
  (e) verify_udp_enqueue_noport  the fused call with the sockets bound to another port: no record is a candidate,
                               so the header pre-pass, the stream and the sums run, the rule and the stores do not
  (f) verify_tcp_assemble      smol_csum_batch_verify_tcp_assemble over the same groups: no record is a TCP segment,
                               so it streams and sums each record in the same workgroup-per-group shape with no
                               pre-pass and no store: the shape's floor
(e) - (f) is the header pre-pass, (c) - (e) the rule's two serial loops, the stores and the entries.

The route the call replaces costs (a) + (b) in kernel time plus a device-host-device round trip and the host's
walk, which this tool does not charge.  Every line is timed with device events around `--launches` back-to-back
launches over `--batches` frame buffers taken in turn, `--rounds` times, the lines interleaved round by round on
one box; reported per launch: the median round, the fastest and the slowest.  Ratios are medians'.  Before the
timing the fused call's arena is compared with (a)'s on the first batch.

    python tools/exp_udp_enqueue.py [--configs 45,6,1] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

CONFIGS = {"45": (1 << 14, 45), "6": (1 << 16, 6), "1": (1 << 18, 1)}
HL, PAY, PORT = 42, 1472, 5000
STRIDE = HL + PAY


def headers(nsocks: int, count: int, seed: int):
    """The (nsocks * count, HL) frame headers (Ethernet, IPv4 with DF, UDP to PORT, checksum fields 0: emit fills
    them), the source port and address varying per datagram."""
    rng = np.random.default_rng(seed)
    h = np.zeros((nsocks * count, HL), np.uint8)
    h[:, 0:14] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 0x08, 0x00)
    tl = 28 + PAY
    h[:, 14:26] = (0x45, 0, tl >> 8, tl & 0xFF, 0, 0, 0x40, 0, 64, 17, 0, 0)
    h[:, 26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    h[:, 28:30] = rng.integers(0, 256, (nsocks * count, 2), dtype=np.uint8)
    h[:, 34:36] = rng.integers(1, 256, (nsocks * count, 2), dtype=np.uint8)
    h[:, 36:42] = (PORT >> 8, PORT & 0xFF, (8 + PAY) >> 8, (8 + PAY) & 0xFF, 0, 0)
    return h


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nsocks, count = CONFIGS[cfg]
    nf = nsocks * count
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0600)
    hdr_d = torch.from_numpy(headers(nsocks, count, 0x5EED0601)).to(dev)
    batch = E.Batch.fixed(nf, STRIDE, STRIDE, E.KIND_ETH)
    bufs, bad = [], []
    mid = count // 2
    for _ in range(batches):
        b = torch.randint(0, 256, (nf, STRIDE), dtype=torch.uint8, device=dev, generator=gen)
        b[:, :HL] = hdr_d
        b = b.reshape(-1)
        eng.emit(b, batch)  # the checksums a sender fills
        bufs.append(b)
        c = b.clone()
        c.view(nsocks, count, STRIDE)[:, mid, HL + 700] ^= 0x10  # one payload bit of the middle datagram of every group
        bad.append(c)
    del hdr_d
    ring = count * PAY
    groups = torch.from_numpy(E.make_groups(np.arange(nsocks, dtype=np.uint64) * count, count).view(np.uint8).copy()).to(dev)
    socks = torch.from_numpy(E.make_udpsocks(np.arange(nsocks, dtype=np.uint64) * ring, np.arange(nsocks, dtype=np.uint64) * count,
                                             ring, 0, 0, count, 0, 0, PORT).view(np.uint8).copy()).to(dev)
    slots = torch.from_numpy(E.make_slots(np.arange(nf, dtype=np.uint64) * PAY, PAY).view(np.uint8).copy()).to(dev)
    arena_a = torch.zeros(nf * PAY, dtype=torch.uint8, device=dev)
    arena_c = torch.zeros(nf * PAY, dtype=torch.uint8, device=dev)
    meta = torch.zeros((nf, 48), dtype=torch.uint8, device=dev)
    st = torch.empty(nf, dtype=torch.uint8, device=dev)
    spans = torch.empty((nf, 8), dtype=torch.uint8, device=dev)
    rx = torch.empty((nf, 16), dtype=torch.uint8, device=dev)
    out = torch.empty((nsocks, 32), dtype=torch.uint8, device=dev)

    noport = torch.from_numpy(E.make_udpsocks(np.arange(nsocks, dtype=np.uint64) * ring, np.arange(nsocks, dtype=np.uint64) * count,
                                              ring, 0, 0, count, 0, 0, PORT + 1).view(np.uint8).copy()).to(dev)
    wins = torch.from_numpy(E.make_tcpwins(np.arange(nsocks, dtype=np.uint64) * ring, ring, 0, 0, ring).view(np.uint8).copy()).to(dev)
    flows = torch.empty((nsocks, 16), dtype=torch.uint8, device=dev)
    fused = lambda b: eng.verify_udp_enqueue(b, batch, groups, arena_c, socks, meta, status=st, rx=rx, out=out)
    ops = {
        "verify_copy": lambda i: eng.verify_copy(bufs[i], batch, arena_a, slots, status=st, spans=spans),
        "verify": lambda i: eng.verify(bufs[i], batch, status=st),
        "verify_udp_enqueue": lambda i: fused(bufs[i]),
        "verify_udp_enqueue_bad": lambda i: fused(bad[i]),
        "verify_udp_enqueue_noport": lambda i: eng.verify_udp_enqueue(bufs[i], batch, groups, arena_c, noport, meta, status=st, rx=rx,
                                                                      out=out),
        "verify_tcp_assemble": lambda i: eng.verify_tcp_assemble(bufs[i], batch, groups, arena_c, wins, status=st, segs=rx, flows=flows),
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call's arena against verify_copy's, on the first batch
    arena_a.zero_()
    arena_c.zero_()
    st_a, _ = eng.verify_copy(bufs[0], batch, arena_a, slots, status=torch.empty_like(st), spans=spans)
    route = eng.last_launch()
    st_c, _, _ = eng.verify_udp_enqueue(bufs[0], batch, groups, arena_c, socks, meta, status=torch.empty_like(st), rx=rx, out=out)
    launched = eng.last_launch()
    oe = out.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE)
    re_ = rx.cpu().numpy().reshape(-1).view(E.UDPRX_DTYPE)
    me = meta.cpu().numpy().reshape(-1).view(E.UDPMETA_DTYPE)
    check = {"arena_equals_verify_copy": bool(torch.equal(arena_c, arena_a)), "status_equals_verify_copy": bool(torch.equal(st_c, st_a)),
             "accepts_all": bool((st_c & E.ST_ACCEPT).all()), "sockets": nsocks,
             "enqueued_all": bool((re_["flags"] == (E.URX_UDP | E.URX_ENQUEUED)).all()) and bool((oe["enqueued"] == count).all()),
             "state_out": bool((oe["payload_len"] == ring).all() and (oe["meta_len"] == count).all()),
             "metadata": bool((me["size"] == PAY).all() and (me["record"] == np.arange(nf)).all() and (me["kind"] == E.UMETA_PACKET).all()),
             "restored": int(oe["restored"].astype(np.uint64).sum())}
    # the corrupted line: the followers of every group's middle datagram move down by one payload
    arena_c.zero_()
    eng.verify_udp_enqueue(bad[0], batch, groups, arena_c, socks, meta, status=st, rx=rx, out=out)
    oe = out.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE)
    keep = np.ones((nsocks, count), bool)
    keep[:, mid] = False
    want = bufs[0].view(nf, STRIDE)[torch.from_numpy(keep.reshape(-1)).to(dev)][:, HL:].reshape(nsocks, (count - 1) * PAY)
    check["bad_enqueued"] = int(oe["enqueued"].astype(np.uint64).sum())
    check["bad_restored"] = int(oe["restored"].astype(np.uint64).sum())
    check["bad_restored_expected"] = nsocks * (count - 1 - mid)
    check["bad_arena"] = bool(torch.equal(arena_c.view(nsocks, ring)[:, :(count - 1) * PAY], want))
    del want

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    payload = nf * PAY
    res = {"config": cfg, "sockets": nsocks, "datagrams_per_socket": count, "frames": nf, "frame_bytes": STRIDE, "payload": PAY,
           "payload_bytes": payload, "batches": len(bufs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "verify_copy_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check}
    X.summarize(res, times, payload)
    X.over(res, "verify_udp_enqueue", ("verify_copy", "verify"))
    a, b, c, d = (res[k]["ms"] for k in ("verify_copy", "verify", "verify_udp_enqueue", "verify_udp_enqueue_bad"))
    res["c_over_a"], res["c_over_a_plus_b"], res["d_over_c"] = round(c / a, 3), round(c / (a + b), 3), round(d / c, 3)
    e, f = res["verify_udp_enqueue_noport"]["ms"], res["verify_tcp_assemble"]["ms"]
    res["parts_ms"] = {"shape_floor_f": f, "header_prepass_e_minus_f": round(e - f, 4), "rule_stores_entries_c_minus_e": round(c - e, 4)}
    eng.close()
    return res


def main():
    args = X.parser("45,6,1", batches=2, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
