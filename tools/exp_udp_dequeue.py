#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_udp_dequeue_emit (every socket's transmit PacketBuffer dequeued on the device,
each datagram written out as a whole frame, headers built there, checksums filled in the pass that copies the
payload) next to the route a caller had before it, on device-resident data: 1024 sockets of 64 datagrams and
65536 sockets of 1.  Datagrams are 1472 bytes, IPv4 over Ethernet (frames of 1514 bytes, back to back); every
socket's payload ring holds its datagrams back to back from ring offset 0, the rings back to back; its metadata
ring has one entry per datagram, the destination address and port varying per datagram.

Lines per shape:
  (a) copy_emit         smol_csum_batch_copy_emit over the same frames with the HOST-BUILT headers already resident
                        in the frame buffer: the route before this call, less its host walk of the metadata rings,
                        its header build and the upload of 42 bytes a frame, which this tool does not charge
  (b) udp_dequeue_emit  the fused call: the rings' walk, the headers and the frames on the device
  (c) udp_dequeue_walk_only  the fused call over the same sockets with ip_mtu 100: every datagram is dequeued as
                        OVERSIZE, so the socket entry, the metadata loads, the serial rule, the d_tx and group
                        entries run and no payload byte moves: (b) - (c) is the frames

Every line is timed with device events around `--launches` back-to-back launches over `--batches` payload arenas
taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch: the median
round, the fastest and the slowest.  The ratio is the medians'.  Before the timing the fused call's frames are
compared with (a)'s byte for byte on the first batch, and checked by verify.

The kernel time by trace comes from runs of their own under the profiler, one per shape and set of lines
(`--lines` names the lines a run launches, so that a kernel's dispatches in the trace are one line's), and is
merged into the event run's file: `--kernel-trace CSV --config 64 --out FILE` runs nothing on the device, reads
rocprofv3's per-dispatch kernel_trace CSV and adds the median, fastest and slowest dispatch of udptx_kernel and of
copy-emit's kernel (copy_kernel on these shapes) under "kernel_trace" to FILE's entry of that shape, the first
16 dispatches of each (warm-up and check) left out:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/exp_udp_dequeue.py --configs 64 \
        --lines copy_emit,udp_dequeue_emit --rounds 3
    python tools/exp_udp_dequeue.py --kernel-trace DIR/.../*_kernel_trace.csv --config 64 --out FILE

    python tools/exp_udp_dequeue.py [--configs 64,1] [--lines a,b] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

CONFIGS = {"64": (1 << 10, 64), "1": (1 << 16, 1)}
HL, PAY, PORT, HOP = 42, 1472, 5000, 64
FRAME = HL + PAY
ETH_DST, ETH_SRC = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2)
LOCAL = (10, 0, 0, 2)


def metadata(nsocks: int, count: int, seed: int):
    """The nsocks * count metadata entries (send-side meaning: where to send and what to send from) and the
    (nsocks * count, HL) headers a host builds from them, checksum fields 0."""
    from smoltcp_amd import engine as E

    rng = np.random.default_rng(seed)
    n = nsocks * count
    m = np.zeros(n, E.UDPMETA_DTYPE)
    m["size"], m["family"], m["kind"] = PAY, 4, E.UMETA_PACKET
    m["src_port"] = rng.integers(1, 65536, n)
    m["remote_addr"][:, :4] = (10, 0, 0, 1)
    m["remote_addr"][:, 2:4] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    m["local_addr"][:, :4] = LOCAL
    h = np.zeros((n, HL), np.uint8)
    h[:, 0:14] = ETH_DST + ETH_SRC + (0x08, 0x00)
    tl = 28 + PAY
    h[:, 14:26] = (0x45, 0, tl >> 8, tl & 0xFF, 0, 0, 0x40, 0, HOP, 17, 0, 0)
    h[:, 26:30] = LOCAL
    h[:, 30:34] = m["remote_addr"][:, :4]
    h[:, 34:36] = (PORT >> 8, PORT & 0xFF)
    h[:, 36] = m["src_port"] >> 8
    h[:, 37] = m["src_port"] & 0xFF
    h[:, 38:42] = ((8 + PAY) >> 8, (8 + PAY) & 0xFF, 0, 0)
    return m, h


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0, lines=None) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nsocks, count = CONFIGS[cfg]
    nf = nsocks * count
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0700)
    srcs = [torch.randint(0, 256, (nf * PAY,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(batches)]
    m, h = metadata(nsocks, count, 0x5EED0701)
    meta = torch.from_numpy(m.view(np.uint8).copy()).to(dev)
    ring = count * PAY
    k = np.arange(nsocks, dtype=np.uint64)
    socks = torch.from_numpy(E.make_udptxsocks(k * ring, k * count, k * (count * FRAME), k * count, ring, 0, ring, count, 0, count,
                                               count * FRAME, count, PORT, 1500, HOP,
                                               eth=(bytes(ETH_DST), bytes(ETH_SRC))).view(np.uint8).copy()).to(dev)
    arena_b = torch.zeros(nf * FRAME, dtype=torch.uint8, device=dev)
    tx = torch.empty((nf, 16), dtype=torch.uint8, device=dev)
    out = torch.empty((nsocks, 32), dtype=torch.uint8, device=dev)
    # route (a): the frames with the host's headers in place, the payloads copied in from the rings
    arena_a = torch.zeros((nf, FRAME), dtype=torch.uint8, device=dev)
    arena_a[:, :HL] = torch.from_numpy(h).to(dev)
    arena_a = arena_a.reshape(-1)
    batch = E.Batch.fixed(nf, FRAME, FRAME, E.KIND_ETH)
    copies = torch.from_numpy(E.make_copies(np.arange(nf, dtype=np.uint64) * PAY, HL, PAY).view(np.uint8).copy()).to(dev)
    # (c): the same sockets under ip_mtu 100: every datagram is dequeued OVERSIZE, nothing is streamed
    walk = socks.clone()
    walk.view(nsocks, 96)[:, 66:68] = torch.tensor([100, 0], dtype=torch.uint8, device=dev)
    ops = {
        "copy_emit": lambda i: eng.copy_emit(arena_a, batch, srcs[i], copies),
        "udp_dequeue_emit": lambda i: eng.udp_dequeue_emit(srcs[i], socks, meta, arena_b, 0, tx=tx, out=out),
        "udp_dequeue_walk_only": lambda i: eng.udp_dequeue_emit(srcs[i], walk, meta, arena_b, 0, tx=tx, out=out),
    }
    if lines:
        ops = {k: ops[k] for k in lines}
    X.warm_up(ops, len(srcs))

    # results must not change: the fused call's frames against copy_emit's, on the first batch
    arena_b.zero_()
    eng.copy_emit(arena_a, batch, srcs[0], copies)
    route = eng.last_launch()
    eng.udp_dequeue_emit(srcs[0], socks, meta, arena_b, 0, tx=tx, out=out)
    launched = eng.last_launch()
    oe = out.cpu().numpy().reshape(-1).view(E.UDPTXOUT_DTYPE)
    te = tx.cpu().numpy().reshape(-1).view(E.UDPTX_DTYPE)
    check = {"frames_equal_copy_emit": bool(torch.equal(arena_b, arena_a)),
             "frames_verify": bool((eng.verify(arena_b, batch) & E.ST_ACCEPT).bool().all()), "sockets": nsocks,
             "sent_all": bool((oe["sent"] == count).all()) and bool((te["flags"] == E.UTX_SENT).all()),
             "state_out": bool((oe["payload_len"] == 0).all() and (oe["meta_len"] == 0).all() and (oe["bytes"] == count * FRAME).all()),
             "stop": sorted(set(oe["stop"].tolist()))}

    times = X.time_interleaved(ops, len(srcs), launches, rounds)
    payload = nf * PAY
    res = {"config": cfg, "sockets": nsocks, "datagrams_per_socket": count, "frames": nf, "frame_bytes": FRAME, "payload": PAY,
           "payload_bytes": payload, "batches": len(srcs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "copy_emit_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check}
    X.summarize(res, times, payload)
    if "udp_dequeue_emit" in res and "copy_emit" in res:
        X.over(res, "udp_dequeue_emit", ("copy_emit",))
    eng.close()
    return res


def merge_trace(csv_path: str, cfg: str, out: str, key: str, skip: int = 16) -> None:
    """The per-dispatch times of rocprofv3's kernel_trace CSV into out's entry of shape cfg, under
    "kernel_trace"[key]: per kernel the dispatches timed, the median, the fastest and the slowest in ms."""
    import csv
    import json
    import statistics

    rows = {}
    with open(csv_path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            short = "udptx_kernel" if "udptx_kernel" in name else "copy_kernel" if "smolcsum::copy_kernel" in name else \
                "xcopy_kernel" if "smolcsum::xcopy_kernel" in name else None
            if short:
                rows.setdefault(short, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    with open(out) as fh:
        res = json.load(fh)
    entry = next(e for e in res if e["config"] == cfg)
    got = {}
    for short, tt in rows.items():
        d = [(b - a) / 1e6 for a, b in sorted(tt)][skip:]
        if d:
            got[short] = {"dispatches": len(d), "ms": round(statistics.median(d), 4), "min_ms": round(min(d), 4),
                          "max_ms": round(max(d), 4)}
    entry.setdefault("kernel_trace", {})[key] = got
    with open(out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(cfg, key, got)


def main():
    ap = X.parser("64,1", batches=2, launches=32)
    ap.add_argument("--lines", default=None, help="the lines to launch (default: all)")
    ap.add_argument("--kernel-trace", default=None, help="merge this kernel_trace CSV into --out instead of running")
    ap.add_argument("--config", default="64", help="with --kernel-trace: the shape the traced run launched")
    ap.add_argument("--trace-key", default="copy_emit,udp_dequeue_emit", help="with --kernel-trace: the traced run's --lines")
    args = ap.parse_args()
    if args.kernel_trace:
        merge_trace(args.kernel_trace, args.config, args.out, args.trace_key)
        return
    lines = args.lines.split(",") if args.lines else None
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds, lines=lines))


if __name__ == "__main__":
    main()
