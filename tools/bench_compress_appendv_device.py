"""What appending a table of tensors costs: a seeded state-dict-like list of tensors in device memory (about 2 000 entries, lengths
log-uniform from 4 bytes to 64 MiB, scaled to --bytes of the silesia mix, zxc_amd/corpus.py; every entry a tensor of its own)
compressed at level 3 into one archive by
  (a) compress_device on a concatenated copy, timed with and without the device copies that concatenate,
  (b) one append session with one append per entry,
  (c) one append session with one appendv over the table,
alternating in one process, at 64 KiB and 512 KiB blocks, max_piece 256 MiB. Wall-clock from the first enqueue to the stream's
end; warm-up runs, then --runs timed repetitions; medians and p10 / p90. Every archive is compared with (a)'s before and after the
timed runs. One JSON line per (block size, variant), printed and appended to --out. --skip-appends leaves (b) out, for tables of
so many small entries that one append each takes minutes (--entries 65536 --bytes 268435456: the gather alone).

    python tools/bench_compress_appendv_device.py [--bytes 1073741824] [--entries 2000] [--blocks 65536,524288] [--level 3]
                                                  [--max-piece 268435456] [--runs 7] [--warmup 2] [--skip-appends]
                                                  [--out profiles/compress_appendv_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from devbench import lengths_log as lengths, pct  # noqa: E402
from zxc_amd import corpus  # noqa: E402

CORPUS_BYTES = 64 << 20  # generated once; a larger source repeats it


def alternating(fns, runs, warmup, stream):
    """-> per function the wall ms of every run, from the first enqueue to the end of the stream"""
    return devbench.alternating(fns, runs, warmup, stream, "wall")


def case(entries, lens, total, bs, a, stream):
    sp = stream.cuda_stream
    n = len(lens)
    cap = int(zxc_amd.lib().zxc_compress_bound(total))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    out_1 = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_s = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    cat = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    ws_1 = zxc_amd.compress_device_work_size(total, a.level, bs, True, False)
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    ws = zxc_amd.compress_append_device_work_size(total, a.max_piece, a.level, bs, True, False)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    ss = zxc_amd.compress_appendv_device_scratch_size(n, a.max_piece, a.level, bs, True, False)
    scratch = torch.empty(ss, dtype=torch.uint8, device="cuda")
    table = np.zeros(n, dtype=zxc_amd.IOV_DTYPE)
    table["base"], table["len"] = [e.data_ptr() for e in entries], lens
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    offs = np.concatenate(([0], np.cumsum(lens))).tolist()
    views = [cat[offs[k]: offs[k + 1]] for k in range(n)]
    ptrs = [e.data_ptr() for e in entries]

    def concat():
        for v, e in zip(views, entries):
            v.copy_(e, non_blocking=True)

    def whole():
        zxc_amd.compress_device(cat.data_ptr(), total, out_1.data_ptr(), cap, work_1.data_ptr(), ws_1, res.data_ptr(), a.level, bs, True, False, sp)

    def whole_with_copies():
        concat()
        whole()

    def appends():
        s = zxc_amd.compress_begin_device(out_s.data_ptr(), cap, total, a.max_piece, work.data_ptr(), ws, a.level, bs, True, False, sp)
        for p, m in zip(ptrs, lens):
            s.append(p, m, sp)
        s.end(res.data_ptr(), sp)

    def appendv():
        s = zxc_amd.compress_begin_device(out_s.data_ptr(), cap, total, a.max_piece, work.data_ptr(), ws, a.level, bs, True, False, sp)
        s.appendv(d_table.data_ptr(), n, total, scratch.data_ptr(), ss, sp)
        s.end(res.data_ptr(), sp)

    def same(what):
        """both sessions' archives against compress_device's for the concatenated copy"""
        whole_with_copies()
        stream.synchronize()
        size = int(res.item())
        assert size > 0, size
        for name, fn in ((("append per entry", appends),) if not a.skip_appends else ()) + (("appendv", appendv),):
            out_s.zero_()
            fn()
            stream.synchronize()
            assert int(res.item()) == size, (what, name, int(res.item()), size)
            assert torch.equal(out_s[:size], out_1[:size]), "%s: the archive of %s differs from compress_device's" % (what, name)
        return size

    size = same("before timing")
    variants = [("compress_device, concatenated before", whole, ws_1), ("compress_device with the concatenating copies", whole_with_copies, ws_1),
                ("session, one append per entry", appends, ws), ("session, one appendv", appendv, ws + ss)]
    if a.skip_appends:
        del variants[2]
    ms = alternating([fn for _, fn, _ in variants], a.runs, a.warmup, stream)
    assert same("after timing") == size
    lines = []
    for (call, _, wbytes), m in zip(variants, ms):
        walls = sorted(m)
        wall = statistics.median(walls)
        lines.append({"call": call, "entries": n, "corpus": "silesia mix", "level": a.level, "block_size": bs, "max_piece": a.max_piece,
                      "source_bytes": total, "archive_bytes": size, "work_bytes": wbytes, "runs": a.runs, "wall_ms": round(wall, 3),
                      "wall_ms_p10": round(pct(walls, 0.1), 3), "wall_ms_p90": round(pct(walls, 0.9), 3),
                      "source_gbps": round(total / wall / 1e6, 2)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--blocks", default="65536,524288", help="comma-separated block sizes")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--max-piece", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-appends", action="store_true", help="leave variant (b) out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_appendv_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    L.zxc_compress_bound.restype = ctypes.c_uint64
    L.zxc_compress_bound.argtypes = [ctypes.c_size_t]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    total = a.bytes
    gen = min(total, CORPUS_BYTES)
    part = torch.frombuffer(bytearray(corpus.synth_silesia(gen, seed=3)), dtype=torch.uint8).to("cuda")
    lens = lengths(a.entries, total, a.seed)
    entries, at = [], 0
    for m in lens:  # every entry a tensor of its own; their concatenation is the corpus, repeated
        e = torch.empty(m, dtype=torch.uint8, device="cuda")
        done = 0
        while done < m:
            k = min(m - done, gen - (at + done) % gen)
            e[done: done + k] = part[(at + done) % gen: (at + done) % gen + k]
            done += k
        entries.append(e)
        at += m
    for bs in (int(x) for x in a.blocks.split(",")):
        for line in case(entries, lens, total, bs, a, stream):
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
