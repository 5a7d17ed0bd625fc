"""What taking an archive into a table of tensors costs: one level-3 seekable archive of --bytes of the silesia mix
(zxc_amd/corpus.py), written by compress_device, decoded into a seeded state-dict-like list of destination tensors in device memory
(about 2 000 entries, lengths log-uniform from 4 bytes to 64 MiB, scaled to --bytes; every entry a tensor of its own) by
  (a)  one decompress_device into one buffer,
  (a') that plus the per-entry device copies out of it,
  (b)  one take session with one take per entry,
  (c)  one take session with one takev over the table,
alternating in one process, at 64 KiB and 512 KiB blocks, max_piece 256 MiB. Wall-clock from the first enqueue to the stream's
end; warm-up runs, then --runs timed repetitions; medians and p10 / p90. Every variant's bytes are compared with the source before
and after the timed runs. One JSON line per (block size, variant), printed and appended to --out. --skip-takes leaves (b) out, for
tables of so many small entries that one take each takes minutes (--entries 65536 --bytes 268435456: the scaling leaves lengths
from 1 byte to about 64 KiB, where nearly every block meets an entry boundary and goes through the scatter).

    python tools/bench_decompress_takev_device.py [--bytes 1073741824] [--entries 2000] [--blocks 65536,524288] [--level 3]
                                                  [--max-piece 268435456] [--runs 7] [--warmup 2] [--skip-takes]
                                                  [--out profiles/decompress_takev_device_bench.jsonl]"""
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


def case(d_src, lens, total, bs, a, stream):
    sp = stream.cuda_stream
    n = len(lens)
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    cap = int(zxc_amd.lib().zxc_compress_bound(total))
    d_arc = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    ws_c = zxc_amd.compress_device_work_size(total, a.level, bs, True, False)
    work_c = torch.empty(ws_c, dtype=torch.uint8, device="cuda")
    zxc_amd.compress_device(d_src.data_ptr(), total, d_arc.data_ptr(), cap, work_c.data_ptr(), ws_c, res.data_ptr(), a.level, bs, True, False, sp)
    stream.synchronize()
    n_arc = int(res.item())
    assert n_arc > 0, n_arc
    del work_c
    torch.cuda.empty_cache()

    whole = torch.zeros(total, dtype=torch.uint8, device="cuda")
    entries = [torch.zeros(m, dtype=torch.uint8, device="cuda") for m in lens]  # every entry a tensor of its own
    ws_1 = zxc_amd.decompress_device_work_size(n_arc, total, bs)
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    ws = zxc_amd.decompress_take_device_work_size(n_arc, total, a.max_piece, bs)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    ss = zxc_amd.decompress_takev_device_scratch_size(n, a.max_piece, bs)
    scratch = torch.empty(ss, dtype=torch.uint8, device="cuda")
    table = np.zeros(n, dtype=zxc_amd.IOV_DTYPE)
    table["base"], table["len"] = [e.data_ptr() for e in entries], lens
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    offs = np.concatenate(([0], np.cumsum(lens))).tolist()
    views = [whole[offs[k]: offs[k + 1]] for k in range(n)]
    ptrs = [e.data_ptr() for e in entries]

    def one_buffer():
        zxc_amd.decompress_device(d_arc.data_ptr(), n_arc, whole.data_ptr(), total, bs, work_1.data_ptr(), ws_1, res.data_ptr(), False, sp)

    def one_buffer_and_copies():
        one_buffer()
        for v, e in zip(views, entries):
            e.copy_(v, non_blocking=True)

    def takes():
        s = zxc_amd.decompress_begin_device(d_arc.data_ptr(), n_arc, total, a.max_piece, bs, work.data_ptr(), ws, False, sp)
        for p, m in zip(ptrs, lens):
            s.take(p, m, sp)
        s.end(res.data_ptr(), sp)

    def takev():
        s = zxc_amd.decompress_begin_device(d_arc.data_ptr(), n_arc, total, a.max_piece, bs, work.data_ptr(), ws, False, sp)
        s.takev(d_table.data_ptr(), n, total, scratch.data_ptr(), ss, sp)
        s.end(res.data_ptr(), sp)

    variants = [("a decompress_device, one buffer", one_buffer, ws_1, False),
                ("a' decompress_device + per-entry copies", one_buffer_and_copies, ws_1 + total, True),
                ("b session, one take per entry", takes, ws, True), ("c session, one takev", takev, ws + ss, True)]
    if a.skip_takes:
        del variants[2]

    def same(what):
        for name, fn, _, into_entries in variants:
            whole.zero_()
            for e in entries:
                e.zero_()
            fn()
            stream.synchronize()
            assert int(res.item()) == total, (what, name, int(res.item()))
            got = torch.cat(entries) if into_entries else whole
            assert torch.equal(got, d_src[:total]), "%s: %s does not give the source" % (what, name)

    same("before timing")
    ms = alternating([fn for _, fn, _, _ in variants], a.runs, a.warmup, stream)
    same("after timing")
    lines = []
    for (call, _, wbytes, _), m in zip(variants, ms):
        walls = sorted(m)
        wall = statistics.median(walls)
        lines.append({"variant": call, "entries": n, "min_len": min(lens), "max_len": max(lens), "corpus": "silesia mix", "level": a.level,
                      "block_size": bs, "max_piece": a.max_piece, "decoded_bytes": total, "archive_bytes": n_arc, "extra_hbm_bytes": wbytes,
                      "runs": a.runs, "wall_ms": round(wall, 3), "wall_ms_p10": round(pct(walls, 0.1), 3),
                      "wall_ms_p90": round(pct(walls, 0.9), 3), "decoded_gbps": round(total / wall / 1e6, 2)})
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
    ap.add_argument("--skip-takes", action="store_true", help="leave variant (b) out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_takev_device_bench.jsonl"))
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
    d_src = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    for at in range(0, total, gen):
        d_src[at: min(at + gen, total)] = part[: min(gen, total - at)]
    lens = lengths(a.entries, total, a.seed)
    for bs in (int(x) for x in a.blocks.split(",")):
        for line in case(d_src, lens, total, bs, a, stream):
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
