"""The dispatch decision (smol_csum_tool_pick: family, variant, shape) over a grid of contexts and
batches, as text lines: what tests/data/dispatch_dump_parent.txt records (run-length coded) and
tests/test_capi_cpu.py::test_dispatch_matches_recorded_dump replays.  Needs no GPU."""
import ctypes
import itertools

from smoltcp_amd import _lib

FIELD_STORES, IPHDR_ONLY = 0x80, 0x01
FORCED_SHAPE = 2  # CFG_G16U6
FORMS = ("packed", "gap1", "gap64", "desc")
ALL_LENGTHS = (64, 97, 1000, 1023, 1024, 1088, 1320, 1409, 1410, 1500, 1520, 1521, 1536, 1921, 1922, 3969,
               3970, 8065, 8066, 9000, 9023, 9024, 16257, 16258, 20000)
RECORDED_LENGTHS = (64, 1500, 1922, 9024)


def _cases():
    """The grid under one variant, in dump order."""
    return itertools.product((0, 1), (-1, FORCED_SHAPE), range(4), FORMS, (0, 1), (0, 1), (0, 1))


def _key(name, v, case):
    ds, shape, op, form, fs, ih, nhc = case
    return f"{name} v{v} ds{ds} sh{shape} op{op} {form} fs{fs} ih{ih} nhc{nhc}: "


def recorded_lines(path):
    """The lines of a recorded dump.  The file lists the distinct pick strings ("V<i> <picks>") and, per
    library and variant ("@ <library> v<variant> <count>x<i> ..."), the run-length coded indices of the
    picks over the grid in dump order."""
    values = {}
    with open(path) as f:
        for line in f:
            w = line.split()
            if line.startswith("V"):
                values[int(w[0][1:])] = " ".join(w[1:])
            elif line.startswith("@"):
                idx = [int(r.split("x")[1]) for r in w[3:] for _ in range(int(r.split("x")[0]))]
                cases = list(_cases())
                assert len(idx) == len(cases), line[:40]
                for case, i in zip(cases, idx):
                    yield _key(w[1], int(w[2][1:]), case) + values[i]


def dump_lines(L, name, lengths):
    """One line per (variant built in L, desc_staged, forced shape, op, batch form, field stores,
    header only, NHC): the picks at each of `lengths`."""
    out3 = (ctypes.c_int * 3)()
    b = _lib.BatchC()
    b.n = 4096
    b.kind = 1
    marker = ctypes.c_void_p(ctypes.addressof(out3))  # never dereferenced: marks a descriptor batch
    for v in range(-1, 128):
        if not L.smol_csum_tool_variant_built(v):
            continue
        for case in _cases():
            ds, shape, op, form, fs, ih, nhc = case
            b.flags = (FIELD_STORES if fs else 0) | (IPHDR_ONLY if ih else 0)
            b.desc = marker if form == "desc" else None
            picks = []
            for ln in lengths:
                b.len = ln
                b.stride = ln + {"packed": 0, "gap1": 1, "gap64": 64, "desc": 0}[form]
                rc = L.smol_csum_tool_pick(v, shape, ds, op, ctypes.byref(b), nhc, out3)
                assert rc == 0, (name, v, rc)
                picks.append("%d/%d/%d" % tuple(out3))
            yield _key(name, v, case) + " ".join(picks)
