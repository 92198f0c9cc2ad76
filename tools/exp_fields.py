#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_emit_fields' three forms next to the in-place emit and verify, on
bench.py's device-resident shapes: C2 (2^20 x 1500 B IPv4/UDP, fixed stride), C4 (2^20 x 1320 B IPv6
mix, fixed stride) and C3 (2^20 IPv4/TCP segments of U[64, 9000] B, packed, descriptors).

Every operation is timed with device events around `--launches` back-to-back launches over `--batches`
batches taken in turn (as bench.py's steps do: an emit that rewrites the batch it just wrote finds its
field segments in the Infinity Cache), `--rounds` times, the operations interleaved round by round on
one box; reported per launch: the median round, and the fastest and slowest.  Ratios are medians'.

    python tools/exp_fields.py [--configs c2,c4,c3] [--records N] [--out FILE]
    python tools/exp_fields.py --sweep 1024,1320,...   # walk form against transposed form per record length
                                                        # (packed and with 64-B gaps, ~1.5 GB per batch): pick_fields' rule
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)


def make_batches(E, eng, cfg: str, n: int, dev, count: int):
    import torch

    if cfg == "c3":
        rng = np.random.default_rng(0x5EED0002)
        lens = rng.integers(64, 9001, n).astype(np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        batch = E.Batch.from_records(offs, lens, E.KIND_IP, dev)
        total, profile = int(offs[-1] + lens[-1]) + 16, E.SYNTH_TCP4
        read = int(lens.astype(np.uint64).sum())
    else:
        L, profile = (1500, E.SYNTH_UDP4) if cfg == "c2" else (1320, E.SYNTH_V6MIX)
        batch = E.Batch.fixed(n, L, L, E.KIND_IP)
        total = read = n * L
    bufs = []
    for j in range(count):
        b = torch.empty(total, dtype=torch.uint8, device=dev)
        eng.synth(b, batch, profile, 0x5EED0100 + j)
        bufs.append(b)
    return batch, bufs, read


def run(cfg: str, n: int, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    batch, bufs, read = make_batches(E, eng, cfg, n, dev, batches)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    fields = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    launched = {}

    def fields_op(form):
        def op(i):
            eng.set_fields_kernel(form)
            eng.emit_fields(bufs[i], batch, fields=fields)
            eng.set_fields_kernel(0)
        return op

    def note(name):
        ll = eng.last_launch()
        launched[name] = f'{ll["kernel"]}/{ll["variant"]} {ll["G"]}x{ll["U"]}'

    ops = {"emit_in_place": lambda i: eng.emit(bufs[i], batch),
           "verify": lambda i: eng.verify(bufs[i], batch, status=status),
           "fields_auto": fields_op(0), "fields_walk": fields_op(1)}
    ops["fields_dwalk" if cfg == "c3" else "fields_xwalk"] = fields_op(3 if cfg == "c3" else 2)
    X.warm_up(ops, len(bufs), after=note)
    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    # the entries are the in-place emit's fields: checked once here, on the last batch
    eng.set_fields_kernel(0)
    eng.emit_fields(bufs[-1], batch, fields=fields)
    f = fields.cpu().numpy().reshape(-1).view(E.FIELDS_DTYPE)
    res = {"config": cfg, "records": n, "read_bytes": read, "entry_bytes": 16 * n, "batches": len(bufs),
           "launches_per_round": launches, "rounds": rounds, "kernels": launched,
           "entries_with_a_field": int((f["off"] != 0xFFFF).any(axis=1).sum())}
    X.summarize(res, times, read, "read_GBs")
    res["fields_auto_over_emit"] = round(res["fields_auto"]["ms"] / res["emit_in_place"]["ms"], 3)
    res["fields_auto_over_verify"] = round(res["fields_auto"]["ms"] / res["verify"]["ms"], 3)
    eng.close()
    return res


def sweep(lengths, batches: int, launches: int, rounds: int, device: int = 0):
    """The walk form against the transposed form over fixed-stride IPv4/UDP records of each length."""
    import torch

    from smoltcp_amd import engine as E

    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    out = []
    for L in lengths:
        for stride in (L, L + 64):
            n = max(1024, (3 << 29) // stride)
            batch = E.Batch.fixed(n, stride, L, E.KIND_IP)
            bufs = []
            for j in range(batches):
                b = torch.zeros(n * stride + 16, dtype=torch.uint8, device=dev)
                eng.synth(b, batch, E.SYNTH_UDP4, 0x5EED0200 + j)
                bufs.append(b)
            fields = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)

            def fields_op(form):
                def op(i):
                    eng.set_fields_kernel(form)
                    eng.emit_fields(bufs[i], batch, fields=fields)
                    eng.set_fields_kernel(0)
                return op

            ops = {"walk": fields_op(1), "xwalk": fields_op(2), "verify": lambda i: eng.verify(bufs[i], batch, status=status)}
            X.warm_up(ops, len(bufs))
            med = X.summarize({}, X.time_interleaved(ops, len(bufs), launches, rounds), n * L)
            row = {"len": L, "stride": stride, "records": n}
            row.update({k + "_ms": v["ms"] for k, v in med.items()})
            row["xwalk_over_walk"] = round(row["xwalk_ms"] / row["walk_ms"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            del bufs, fields, status
    eng.close()
    return out


def main():
    ap = X.parser("c2,c4,c3", batches=4, launches=16)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--sweep", default=None, help="comma-separated record lengths (1024 .. 16257)")
    args = ap.parse_args()
    if args.sweep:
        rows = sweep([int(x) for x in args.sweep.split(",")], min(args.batches, 2), args.launches, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("".join(json.dumps(r) + "\n" for r in rows))
        return
    X.run_configs(args, lambda c: run(c, args.records, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
