#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_echo_reply (a batch of received frames verified, the reply to every
ICMP echo request written to its slot in the same pass) next to what a caller could do before it, on
device-resident data.  Every record is an answerable echo request in an Ethernet frame, checksums filled:

  98    2^20 x 98-byte Ethernet / IPv4 requests (ping's default: 56 data bytes), fixed stride
  1514  2^20 x 1514-byte Ethernet / IPv4 requests (1472 data bytes), fixed stride
  1294  2^20 x 1294-byte Ethernet / IPv6 requests (1232 data bytes), fixed stride
  mix   2^18 Ethernet / IPv4 requests of U[64, 9000] bytes, a descriptor batch (2^18: a buffer of 1.2 GB)

Lines per config, on the same batches:
  (a) verify_echo_reply    the fused call, replies back to back in an arena
  (b) verify               smol_csum_batch_verify alone: the floor of any route that reads each request once
  (c) verify_then_copy_emit  what a caller can do without the call: verify, then smol_csum_batch_copy_emit over a
                           second batch whose reply heads were prepared beforehand, the echo data copied from
                           the requests.  THIS LINE LEAVES OUT the host's work between the two calls (reading
                           the status, building every reply head, uploading heads and copy descriptors), so it
                           flatters the route without the fused call.
  (d) verify_echo_reply_cap0  the fused call with every slot's cap 0: every request is answered and none
                           written, so the call streams, sums twice, applies the rule and writes status bytes
                           and entries, and stores no frame.  (a) - (d) is what the frames' stores cost.

Every line is timed with device events around `--launches` back-to-back launches over `--batches` frame
buffers taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch:
the median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's arena
is compared with (c)'s reply batch on the first buffer, byte for byte.

    python tools/exp_echo_reply.py [--configs 98,1514,1294,mix] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

# config -> (records, IP version, frame length or None for U[64, 9000] over descriptors)
CONFIGS = {"98": (1 << 20, 4, 98), "1514": (1 << 20, 4, 1514), "1294": (1 << 20, 6, 1294), "mix": (1 << 18, 4, None)}
MAC_A, MAC_B = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2)


def heads(ver: int, dlen: np.ndarray, seed: int):
    """(request heads, reply heads), n x head_len each, every checksum field zero: Ethernet, IP and the first 8
    bytes of the ICMP message, for requests carrying dlen[i] data bytes; the reply heads are what a host would
    build (MACs and addresses swapped, a fresh IP header, type 0 / 129, the same ident and sequence number)."""
    rng = np.random.default_rng(seed)
    n = dlen.size
    hl = 14 + (20 if ver == 4 else 40) + 8
    rq, rp = np.zeros((n, hl), np.uint8), np.zeros((n, hl), np.uint8)
    et = (0x08, 0x00) if ver == 4 else (0x86, 0xDD)
    rq[:, 0:14] = MAC_A + MAC_B + et
    rp[:, 0:14] = MAC_B + MAC_A + et
    idseq = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if ver == 4:
        src = np.array((10, 0, 0, 1), np.uint8)[None, :].repeat(n, 0)
        src[:, 2:4] = rng.integers(1, 255, (n, 2), dtype=np.uint8)
        dst = (10, 9, 0, 2)
        tl = (28 + dlen).astype(np.uint32)
        for h, s, d, ttl in ((rq, src, dst, 57), (rp, dst, src, 64)):
            h[:, 14:16] = (0x45, 0)
            h[:, 16], h[:, 17] = tl >> 8, tl & 0xFF
            h[:, 20:24] = (0x40, 0, ttl, 1)
            h[:, 26:30], h[:, 30:34] = s, d
        rq[:, 18:20] = rng.integers(0, 256, (n, 2), dtype=np.uint8)  # the request's ident; the reply's is 0
        l4 = 34
    else:
        src = np.frombuffer(bytes.fromhex("20010db8000000000000000000000001"), np.uint8)[None, :].repeat(n, 0)
        src[:, 12:16] = rng.integers(1, 255, (n, 4), dtype=np.uint8)
        dst = np.frombuffer(bytes.fromhex("20010db8000100000000000000000002"), np.uint8)
        pl = (8 + dlen).astype(np.uint32)
        for h, s, d, hop in ((rq, src, dst, 57), (rp, dst, src, 64)):
            h[:, 14] = 0x60
            h[:, 18], h[:, 19] = pl >> 8, pl & 0xFF
            h[:, 20:22] = (58, hop)
            h[:, 22:38], h[:, 38:54] = s, d
        l4 = 54
    rq[:, l4], rp[:, l4] = (8, 0) if ver == 4 else (128, 129)
    rq[:, l4 + 4:l4 + 8] = rp[:, l4 + 4:l4 + 8] = idseq
    return rq, rp


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    n, ver, flen = CONFIGS[cfg]
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0600)
    rng = np.random.default_rng(0x5EED0601)
    lens = np.full(n, flen, np.int64) if flen is not None else rng.integers(64, 9001, n).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    hl = 14 + (20 if ver == 4 else 40) + 8
    rq, rp = heads(ver, lens - hl, 0x5EED0602)
    if flen is not None:
        batch = E.Batch.fixed(n, flen, flen, E.KIND_ETH)
    else:
        batch = E.Batch.from_records(offs, lens, E.KIND_ETH, dev)
    idx = (torch.from_numpy(offs).to(dev)[:, None] + torch.arange(hl, device=dev)[None, :]).reshape(-1)
    rq_d = torch.from_numpy(rq).to(dev).reshape(-1)
    bufs = []
    for _ in range(batches):
        b = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=dev, generator=gen)
        b[idx] = rq_d
        eng.emit(b, batch)  # the checksums a sender fills
        bufs.append(b)
    # the route without the call: a second batch of the same geometry with the reply heads in place, and one
    # copy per record for the echo data
    replies = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    replies[idx] = torch.from_numpy(rp).to(dev).reshape(-1)
    del idx, rq_d
    copies = torch.from_numpy(E.make_copies(offs + hl, hl, lens - hl).view(np.uint8).copy()).to(dev)
    slots = torch.from_numpy(E.make_slots(offs, lens).view(np.uint8).copy()).to(dev)
    slots0 = torch.from_numpy(E.make_slots(offs, 0).view(np.uint8).copy()).to(dev)
    arena = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    ent = torch.empty((n, 8), dtype=torch.uint8, device=dev)

    def two_calls(i):
        eng.verify(bufs[i], batch, status=st)
        eng.copy_emit(replies, batch, bufs[i], copies)

    ops = {
        "verify_echo_reply": lambda i: eng.verify_echo_reply(bufs[i], batch, arena, slots, status=st, echo=ent),
        "verify": lambda i: eng.verify(bufs[i], batch, status=st),
        "verify_then_copy_emit": two_calls,
        "verify_echo_reply_cap0": lambda i: eng.verify_echo_reply(bufs[i], batch, arena, slots0, status=st, echo=ent),
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call's arena against the two calls' reply batch, on the first buffer
    arena.zero_()
    st_a, _ = eng.verify_echo_reply(bufs[0], batch, arena, slots, status=torch.empty_like(st), echo=ent)
    launched = eng.last_launch()
    two_calls(0)
    route = eng.last_launch()
    fl = ent.cpu().numpy().reshape(-1).view(E.ECHO_DTYPE)["flags"]
    full = E.ECHO_REQUEST | E.ECHO_ANSWERED | E.ECHO_WRITTEN | E.ECHO_SEND
    check = {"arena_equals_copy_emit": bool(torch.equal(arena[:total], replies[:total])),
             "status_equals_verify": bool(torch.equal(st_a, st)), "send_all": bool((fl == full).all())}

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    res = {"config": cfg, "records": n, "ip_version": ver, "frame_bytes": flen if flen is not None else "U[64, 9000]",
           "batch_bytes": total, "batches": len(bufs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "copy_emit_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check,
           "note": "verify_then_copy_emit leaves out the host's head building and upload between its two calls"}
    X.summarize(res, times, total, "frame_GBs")
    X.over(res, "verify_echo_reply", ("verify", "verify_then_copy_emit", "verify_echo_reply_cap0"))
    eng.close()
    return res


def main():
    args = X.parser("98,1514,1294,mix", batches=2, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
