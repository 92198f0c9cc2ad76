#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_tcp_assemble (a batch of received frames verified, every TCP
segment's payload put at its sequence number's place in its connection's receive ring in the same pass) next
to what a caller could do before it, on device-resident data: 2^14 flows of 45 segments, 2^16 flows of 6 and
2^18 flows of 1.  Frames are Ethernet + IPv4 + a 20-byte TCP header with 1460-byte payloads at a fixed stride
of 1514 (what tcp_segment_emit leaves in a TX ring), in order, nothing trimmed, nothing wrapping; every
flow's ring is its window, count * 1460 bytes, the rings back to back.

Lines per shape:
  (a) verify_copy          smol_csum_batch_verify_copy over the same records, slots precomputed by the host at
                           the same places: the route that exists when the host already has the sequence
                           numbers
  (b) verify               smol_csum_batch_verify alone: the read floor
  (c) verify_tcp_assemble  the fused call

Every line is timed with device events around `--launches` back-to-back launches over `--batches` frame
buffers taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch:
the median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's arena
is compared with (a)'s on the first batch.

    python tools/exp_tcp_assemble.py [--configs 45,6,1] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

CONFIGS = {"45": (1 << 14, 45), "6": (1 << 16, 6), "1": (1 << 18, 1)}
HL, MSS = 54, 1460
STRIDE = HL + MSS


def headers(nflows: int, count: int, seed: int):
    """The (nflows * count, HL) frame headers (Ethernet, IPv4 with DF, TCP with ACK | PSH, checksum fields 0:
    emit fills them) and every flow's first sequence number."""
    rng = np.random.default_rng(seed)
    h = np.zeros((nflows, count, HL), np.uint8)
    h[:, :, 0:14] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 0x08, 0x00)
    tl = 40 + MSS
    h[:, :, 14:26] = (0x45, 0, tl >> 8, tl & 0xFF, 0, 0, 0x40, 0, 64, 6, 0, 0)
    h[:, :, 26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    h[:, :, 34:38] = (0x0F, 0xA1, 0x00, 0x50)  # ports 4001 -> 80
    seq0 = rng.integers(0, 1 << 32, nflows, dtype=np.uint64).astype(np.uint32)
    seq = seq0[:, None] + (np.arange(count, dtype=np.uint32) * np.uint32(MSS))[None, :]
    for b in range(4):
        h[:, :, 38 + b] = (seq >> (24 - 8 * b)).astype(np.uint8)
    h[:, :, 42:46] = rng.integers(0, 256, (nflows, 1, 4), dtype=np.uint8)  # ack number
    h[:, :, 46:50] = (0x50, 0x18, 0x20, 0x00)
    return h.reshape(-1, HL), seq0


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nflows, count = CONFIGS[cfg]
    nf = nflows * count
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0500)
    hdr, seq0 = headers(nflows, count, 0x5EED0501)
    hdr_d = torch.from_numpy(hdr).to(dev)
    batch = E.Batch.fixed(nf, STRIDE, STRIDE, E.KIND_ETH)
    bufs = []
    for _ in range(batches):
        b = torch.randint(0, 256, (nf, STRIDE), dtype=torch.uint8, device=dev, generator=gen)
        b[:, :HL] = hdr_d
        b = b.reshape(-1)
        eng.emit(b, batch)  # the checksums a sender fills
        bufs.append(b)
    del hdr_d, hdr
    ring = count * MSS
    groups = torch.from_numpy(E.make_groups(np.arange(nflows, dtype=np.uint64) * count, count).view(np.uint8).copy()).to(dev)
    wins = torch.from_numpy(E.make_tcpwins(np.arange(nflows, dtype=np.uint64) * ring, ring, 0, seq0, ring).view(np.uint8).copy()).to(dev)
    slots = torch.from_numpy(E.make_slots(np.arange(nf, dtype=np.uint64) * MSS, MSS).view(np.uint8).copy()).to(dev)
    arena_a = torch.zeros(nf * MSS, dtype=torch.uint8, device=dev)
    arena_c = torch.zeros(nf * MSS, dtype=torch.uint8, device=dev)
    st = torch.empty(nf, dtype=torch.uint8, device=dev)
    spans = torch.empty((nf, 8), dtype=torch.uint8, device=dev)
    segs = torch.empty((nf, 16), dtype=torch.uint8, device=dev)
    flows = torch.empty((nflows, 16), dtype=torch.uint8, device=dev)

    ops = {
        "verify_copy": lambda i: eng.verify_copy(bufs[i], batch, arena_a, slots, status=st, spans=spans),
        "verify": lambda i: eng.verify(bufs[i], batch, status=st),
        "verify_tcp_assemble": lambda i: eng.verify_tcp_assemble(bufs[i], batch, groups, arena_c, wins, status=st, segs=segs,
                                                                 flows=flows),
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call's arena against verify_copy's, on the first batch
    arena_a.zero_()
    arena_c.zero_()
    st_a, _ = eng.verify_copy(bufs[0], batch, arena_a, slots, status=torch.empty_like(st), spans=spans)
    route = eng.last_launch()
    st_c, _, _ = eng.verify_tcp_assemble(bufs[0], batch, groups, arena_c, wins, status=torch.empty_like(st), segs=segs, flows=flows)
    launched = eng.last_launch()
    fe = flows.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE)
    se = segs.cpu().numpy().reshape(-1).view(E.TCPSEG_DTYPE)
    check = {"arena_equals_verify_copy": bool(torch.equal(arena_c, arena_a)), "status_equals_verify_copy": bool(torch.equal(st_c, st_a)),
             "accepts_all": bool((st_c & E.ST_ACCEPT).all()), "flows": nflows,
             "contig_all": bool((fe["contig_len"] == ring).all()), "counted_all": bool((fe["counted"] == count).all()),
             "redelivered": int(fe["redelivered"].astype(np.uint64).sum()),
             "copied_all": bool((se["flags"] == (E.SEG_TCP | E.SEG_IN_WINDOW | E.SEG_COPIED)).all())}

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    payload = nf * MSS
    res = {"config": cfg, "flows": nflows, "segments_per_flow": count, "frames": nf, "frame_bytes": STRIDE, "mss": MSS,
           "payload_bytes": payload, "batches": len(bufs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "verify_copy_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check}
    X.summarize(res, times, payload)
    X.over(res, "verify_tcp_assemble", ("verify_copy", "verify"))
    eng.close()
    return res


def main():
    args = X.parser("45,6,1", batches=2, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
