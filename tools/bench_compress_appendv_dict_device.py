"""What writing a dictionary archive from a table of tensors costs: --entries tensors in device memory (lengths uniform within
+-50 % of their mean, adding up to --bytes of the silesia mix, zxc_amd/corpus.py; every entry a tensor of its own) compressed at
level 3 into one archive by one append session begun with a dictionary of --dict-size bytes cut from the corpus, in the three ways
a caller has:
  (a) one append per entry,
  (b) torch.cat of the entries, then one append of the copy; the copy's own time and the extra device memory it takes are reported,
  (c) one appendv_dict over the table,
alternating in one process, at 4 KiB and 64 KiB blocks, max_piece 256 MiB. Wall-clock from the first enqueue to the stream's end;
warm-up runs, then --runs timed repetitions; medians and p10 / p90. Every archive is compared with compress_dict_device's for the
concatenation before and after the timed runs. One JSON line per (block size, variant), printed and appended to --out.
--skip-appends leaves (a) out, for tables of so many entries that one append each takes minutes.

    python tools/bench_compress_appendv_dict_device.py [--bytes 268435456] [--entries 500] [--blocks 4096,65536] [--dict-size 65535]
                                                       [--level 3] [--max-piece 268435456] [--runs 7] [--warmup 2] [--skip-appends]
                                                       [--out profiles/compress_appendv_dict_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from zxc_amd import corpus  # noqa: E402
from bench_compress_appendv_device import CORPUS_BYTES, alternating  # noqa: E402
from devbench import lengths_uniform as lengths, pct  # noqa: E402


def case(entries, lens, total, bs, dd, a, stream):
    sp = stream.cuda_stream
    n = len(lens)
    D = dd[1]
    cap = int(zxc_amd.lib().zxc_compress_bound(total))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    out_1 = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_s = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ws_1 = zxc_amd.compress_dict_device_work_size(total, D, a.level, bs, True, False)
    ws = zxc_amd.compress_append_dict_device_work_size(total, a.max_piece, D, a.level, bs, True, False)
    ss = zxc_amd.compress_appendv_dict_device_scratch_size(n, a.max_piece, D, a.level, bs, True, False)
    assert ws_1 > 0 and ws > 0 and ss > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(ss, dtype=torch.uint8, device="cuda")
    table = np.zeros(n, dtype=zxc_amd.IOV_DTYPE)
    table["base"], table["len"] = [e.data_ptr() for e in entries], lens
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    ptrs = [e.data_ptr() for e in entries]
    keep = []

    def begin():
        return zxc_amd.compress_begin_dict_device(out_s.data_ptr(), cap, total, a.max_piece, dd, work.data_ptr(), ws, a.level, bs, True, False, sp)

    def appends():
        s = begin()
        for p, m in zip(ptrs, lens):
            s.append(p, m, sp)
        s.end(res.data_ptr(), sp)

    def cat_only():
        keep[:] = [torch.cat(entries)]  # (held until the next run: the append reads it on the stream)

    def cat_append():
        cat_only()
        s = begin()
        s.append(keep[0].data_ptr(), total, sp)
        s.end(res.data_ptr(), sp)

    def appendv_dict():
        s = begin()
        s.appendv_dict(d_table.data_ptr(), n, total, scratch.data_ptr(), ss, sp)
        s.end(res.data_ptr(), sp)

    def same(what):
        """the sessions' archives against compress_dict_device's for a concatenated copy"""
        whole = torch.cat(entries + [torch.zeros(64, dtype=torch.uint8, device="cuda")])
        work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
        zxc_amd.compress_dict_device(whole.data_ptr(), total, out_1.data_ptr(), cap, dd, work_1.data_ptr(), ws_1, res.data_ptr(), a.level, bs, True,
                                     False, sp)
        stream.synchronize()
        size = int(res.item())
        assert size > 0, size
        for name, fn in ((("append per entry", appends),) if not a.skip_appends else ()) + (("cat, append", cat_append), ("appendv_dict", appendv_dict)):
            out_s.zero_()
            fn()
            stream.synchronize()
            assert int(res.item()) == size, (what, name, int(res.item()), size)
            assert torch.equal(out_s[:size], out_1[:size]), "%s: the archive of %s differs from compress_dict_device's" % (what, name)
        del whole, work_1
        return size

    size = same("before timing")
    variants = [("a: session, one append per entry", appends, ws, 0), ("b: torch.cat, then one append", cat_append, ws, total),
                ("b: the torch.cat alone", cat_only, 0, total), ("c: session, one appendv_dict", appendv_dict, ws + ss, 0)]
    if a.skip_appends:
        del variants[0]
    ms = alternating([fn for _, fn, _, _ in variants], a.runs, a.warmup, stream)
    assert same("after timing") == size
    keep.clear()
    lines = []
    for (call, _, wbytes, extra), m in zip(variants, ms):
        walls = sorted(m)
        wall = statistics.median(walls)
        lines.append({"call": call, "entries": n, "corpus": "silesia mix", "level": a.level, "block_size": bs, "dict_size": D,
                      "max_piece": a.max_piece, "source_bytes": total, "archive_bytes": size, "work_bytes": wbytes, "extra_hbm_bytes": extra,
                      "runs": a.runs, "wall_ms": round(wall, 3), "wall_ms_p10": round(pct(walls, 0.1), 3),
                      "wall_ms_p90": round(pct(walls, 0.9), 3), "source_gbps": round(total / wall / 1e6, 2)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--entries", type=int, default=500)
    ap.add_argument("--blocks", default="4096,65536", help="comma-separated block sizes")
    ap.add_argument("--dict-size", type=int, default=65535)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--max-piece", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-appends", action="store_true", help="leave variant (a) out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_appendv_dict_device_bench.jsonl"))
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
    text = corpus.synth_silesia(gen + a.dict_size, seed=3)
    part = torch.frombuffer(bytearray(text[:gen]), dtype=torch.uint8).to("cuda")
    d_content = torch.frombuffer(bytearray(text[gen:]), dtype=torch.uint8).to("cuda")  # the dictionary: the corpus's next bytes
    d_id = torch.zeros(1, dtype=torch.int32, device="cuda")
    dd = (d_content.data_ptr(), a.dict_size, 0, d_id.data_ptr())
    zxc_amd.dict_prepare_device(dd[0], dd[1], dd[2], dd[3], stream.cuda_stream)
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
        for line in case(entries, lens, total, bs, dd, a, stream):
            out = json.dumps(line)
            print(out, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(out + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
