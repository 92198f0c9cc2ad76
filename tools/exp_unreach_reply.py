#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_unreach_reply (a batch of received frames verified, the ICMP error for
every UDP datagram to a closed port written to its slot in the same pass) next to what a caller could do before
it, on device-resident data.  Every record is a UDP datagram in an Ethernet frame, checksums filled; 2^16 records
per config, fixed stride:

  70    70-byte Ethernet / IPv4 probes (a port scan's), all to closed ports: 98-byte error frames
  590   590-byte Ethernet / IPv4 datagrams to closed ports: 590-byte error frames, the data cut at 528 bytes
  1514  1514-byte Ethernet / IPv4 datagrams to closed ports: the same frames, 944 payload bytes behind the cut
  1294  1294-byte Ethernet / IPv6 datagrams to closed ports: 1294-byte error frames, the data cut at 1192 bytes
  mix   70-byte probes, nine in ten to open ports: the call mostly verifies

Lines per config, on the same batches:
  (a) verify_unreach_reply   the fused call, error frames back to back in an arena
  (b) verify                 smol_csum_batch_verify alone: the floor of any route that reads each datagram once
  (c) verify_then_copy_emit  what a caller can do without the call: verify, then smol_csum_batch_copy_emit over a
                             second batch whose frame heads (Ethernet, IP, ICMP, the quoted header) were prepared
                             beforehand, the quoted data copied from the datagrams.  THIS LINE LEAVES OUT the
                             host's work between the two calls (downloading the headers to learn the ports,
                             building every head, uploading heads and copy descriptors), so it flatters the
                             route without the fused call.

Every line is timed with device events around `--launches` back-to-back launches over `--batches` frame
buffers taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch:
the median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's arena
is compared with (c)'s frame batch on the first buffer, byte for byte.

    python tools/exp_unreach_reply.py [--configs 70,590,1514,1294,mix] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

N = 1 << 16
# config -> (IP version, frame length, share of datagrams to open ports in tenths)
CONFIGS = {"70": (4, 70, 0), "590": (4, 590, 0), "1514": (4, 1514, 0), "1294": (6, 1294, 0), "mix": (4, 70, 9)}
MAC_A, MAC_B = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2)
OPEN_PORT = 53


def heads(ver: int, plen: int, open_tenths: int, seed: int):
    """(request heads, error-frame heads, closed): the requests' Ethernet, IP and UDP headers, n x (14 + 20 | 40 + 8),
    and what a host would build in front of the quoted data for each (MACs and addresses swapped, a fresh IP
    header, Destination Unreachable / Port Unreachable, the request's header emitted again), every checksum field
    zero; closed[i]: the request goes to a closed port."""
    rng = np.random.default_rng(seed)
    n, iph = N, 20 if ver == 4 else 40
    dlen = min(plen, 528 if ver == 4 else 1192)
    rq, rp = np.zeros((n, 14 + iph + 8), np.uint8), np.zeros((n, 14 + 2 * iph + 8), np.uint8)
    et = (0x08, 0x00) if ver == 4 else (0x86, 0xDD)
    rq[:, 0:14] = MAC_A + MAC_B + et
    rp[:, 0:14] = MAC_B + MAC_A + et
    ttl = rng.integers(1, 256, n, dtype=np.uint8)
    q = 14 + iph + 8  # the quoted header's place in the frame
    if ver == 4:
        src = np.array((10, 0, 0, 1), np.uint8)[None, :].repeat(n, 0)
        src[:, 2:4] = rng.integers(1, 255, (n, 2), dtype=np.uint8)
        dst = (10, 9, 0, 2)
        for h, o, tl, s, d in ((rq, 14, 20 + plen, src, dst), (rp, 14, 48 + dlen, dst, src), (rp, q, 20 + plen, src, dst)):
            h[:, o:o + 4] = (0x45, 0, tl >> 8, tl & 0xFF)
            h[:, o + 6] = 0x40
            h[:, o + 12:o + 16], h[:, o + 16:o + 20] = s, d
        rq[:, 14 + 4:14 + 6] = rng.integers(0, 256, (n, 2), dtype=np.uint8)  # the request's ident; the others' are 0
        rq[:, 14 + 8], rq[:, 14 + 9] = ttl, 17
        rp[:, 14 + 8:14 + 10] = (64, 1)
        rp[:, q + 8], rp[:, q + 9] = ttl, 17
        rp[:, 34:36] = (3, 3)
    else:
        src = np.frombuffer(bytes.fromhex("20010db8000000000000000000000001"), np.uint8)[None, :].repeat(n, 0)
        src[:, 12:16] = rng.integers(1, 255, (n, 4), dtype=np.uint8)
        dst = np.frombuffer(bytes.fromhex("20010db8000100000000000000000002"), np.uint8)
        for h, o, pl, s, d in ((rq, 14, plen, src, dst), (rp, 14, 48 + dlen, dst, src), (rp, q, plen, src, dst)):
            h[:, o] = 0x60
            h[:, o + 4:o + 6] = (pl >> 8, pl & 0xFF)
            h[:, o + 8:o + 24], h[:, o + 24:o + 40] = s, d
        rq[:, 14 + 6], rq[:, 14 + 7] = 17, ttl
        rp[:, 14 + 6:14 + 8] = (58, 64)
        rp[:, q + 6], rp[:, q + 7] = 17, ttl
        rp[:, 54:56] = (1, 4)
    closed = (np.arange(n) % 10) >= open_tenths
    port = np.where(closed, rng.integers(1024, 65536, n), OPEN_PORT)
    u = 14 + iph
    rq[:, u:u + 2] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    rq[:, u + 2], rq[:, u + 3] = port >> 8, port & 0xFF
    rq[:, u + 4:u + 6] = (plen >> 8, plen & 0xFF)
    return rq, rp, closed


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    ver, flen, open_tenths = CONFIGS[cfg]
    n, iph = N, 20 if ver == 4 else 40
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0700)
    plen = flen - 14 - iph
    dlen = min(plen, 528 if ver == 4 else 1192)
    hl, rl = 14 + iph + 8, 14 + 2 * iph + 8   # the request's head, the error frame's
    out_len = rl + dlen
    rq, rp, closed = heads(ver, plen, open_tenths, 0x5EED0702)
    offs = np.arange(n, dtype=np.int64) * flen
    total = n * flen
    batch = E.Batch.fixed(n, flen, flen, E.KIND_ETH)
    idx = (torch.from_numpy(offs).to(dev)[:, None] + torch.arange(hl, device=dev)[None, :]).reshape(-1)
    rq_d = torch.from_numpy(rq).to(dev).reshape(-1)
    bufs = []
    for _ in range(batches):
        b = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=dev, generator=gen)
        b[idx] = rq_d
        eng.emit(b, batch)  # the checksums a sender fills
        bufs.append(b)
    del idx, rq_d
    # the route without the call: a batch of the error frames with their heads in place, back to back, and one copy
    # per frame for the quoted data
    who = np.flatnonzero(closed)
    m = who.size
    foffs = np.arange(m, dtype=np.int64) * out_len
    frames = torch.zeros(m * out_len + 16, dtype=torch.uint8, device=dev)
    fidx = (torch.from_numpy(foffs).to(dev)[:, None] + torch.arange(rl, device=dev)[None, :]).reshape(-1)
    frames[fidx] = torch.from_numpy(rp[who]).to(dev).reshape(-1)
    del fidx
    fbatch = E.Batch.fixed(m, out_len, out_len, E.KIND_ETH)
    copies = torch.from_numpy(E.make_copies(offs[who] + 14 + iph, rl, dlen).view(np.uint8).copy()).to(dev)
    soffs = np.zeros(n, np.int64)
    soffs[who] = foffs
    slots = torch.from_numpy(E.make_slots(soffs, np.where(closed, out_len, 0)).view(np.uint8).copy()).to(dev)
    pmap = torch.from_numpy(E.make_port_map([OPEN_PORT])).to(dev)
    arena = torch.zeros(m * out_len + 16, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    ent = torch.empty((n, 8), dtype=torch.uint8, device=dev)

    def two_calls(i):
        eng.verify(bufs[i], batch, status=st)
        eng.copy_emit(frames, fbatch, bufs[i], copies)

    ops = {
        "verify_unreach_reply": lambda i: eng.verify_unreach_reply(bufs[i], batch, arena, slots, pmap, status=st, unr=ent),
        "verify": lambda i: eng.verify(bufs[i], batch, status=st),
        "verify_then_copy_emit": two_calls,
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call's arena against the two calls' frame batch, on the first buffer
    arena.zero_()
    st_a, _ = eng.verify_unreach_reply(bufs[0], batch, arena, slots, pmap, status=torch.empty_like(st), unr=ent)
    launched = eng.last_launch()
    two_calls(0)
    route = eng.last_launch()
    fl = ent.cpu().numpy().reshape(-1).view(E.UNR_DTYPE)["flags"]
    full = E.UNR_REFUSED | E.UNR_PORT | E.UNR_ANSWERED | E.UNR_WRITTEN | E.UNR_SEND
    check = {"arena_equals_copy_emit": bool(torch.equal(arena, frames)), "status_equals_verify": bool(torch.equal(st_a, st)),
             "send_all_closed": bool((fl[closed] == full).all()), "open_untouched": bool((fl[~closed] == 0).all())}

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    res = {"config": cfg, "records": n, "ip_version": ver, "frame_bytes": flen, "closed_share": round(m / n, 3),
           "error_frame_bytes": out_len, "batch_bytes": total, "batches": len(bufs), "launches_per_round": launches,
           "rounds": rounds, "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "copy_emit_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check,
           "note": "verify_then_copy_emit leaves out the host's header download, head building and upload between its two calls"}
    X.summarize(res, times, total, "frame_GBs")
    X.over(res, "verify_unreach_reply", ("verify", "verify_then_copy_emit"))
    eng.close()
    return res


def main():
    args = X.parser("70,590,1514,1294,mix", batches=2, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
