"""What random access into separate tensors costs: one level-3 seekable archive of --mib MiB of the silesia mix (zxc_amd/corpus.py),
written by compress_device and opened on the device, and --ranges seeded ranges of it (lengths uniform in [--max-len / 4, --max-len],
any offset: "load these experts"), each with a destination tensor of its own, fetched by
  (a)  one decompress_rangesv_device, every base = offset (mod 16): whole blocks decode in place,
  (b)  one decompress_ranges_device of the same ranges into ONE buffer, dst_off = offset (mod 16),
  (c)  (b) plus one device-to-device copy per range into the separate tensors: what a caller does without the new call,
  (d)  one decompress_rangesv_device with every base at an odd alignment against its offset: every block through a slot and a copy,
alternating in one process, at 64 KiB and 512 KiB blocks. Wall-clock from the first enqueue to the stream's end; warm-up runs, then
--runs timed repetitions; medians, p10 / p90 and the full spread. Every fetched byte of every variant is compared with the source
before the timed runs, and again after them. One JSON line per (block size, variant), with the ratios of (a) to (b) and to (c) on
(a)'s line, printed and appended to --out.

    python tools/bench_decompress_rangesv_device.py [--mib 256] [--ranges 512] [--max-len 1048576] [--blocks 65536,524288]
                                                    [--level 3] [--runs 10] [--warmup 2]
                                                    [--out profiles/decompress_rangesv_device_bench.jsonl]"""
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
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from bench_decompress_device import archive_on_device  # noqa: E402
from devbench import pct  # noqa: E402
from zxc_amd import corpus  # noqa: E402

CORPUS_BYTES = 64 << 20  # generated once; a larger source repeats it


def case(d_src, total, bs, a, stream):
    sp = stream.cuda_stream
    nb = -(-total // bs)
    arc, n_arc = archive_on_device(d_src, total, a.level, bs, True, False, stream)
    isz = zxc_amd.seekable_index_size(nb)
    index = torch.zeros((isz + 7) // 8, dtype=torch.int64, device="cuda")
    zxc_amd.seekable_open_device(arc.data_ptr(), n_arc, bs, nb, index.data_ptr(), isz, sp)
    stream.synchronize()
    assert int(index[:1].cpu().numpy().view(np.int32)[0]) == 0, "open failed"

    rng = np.random.default_rng(a.seed + bs)
    n, max_len = a.ranges, a.max_len
    lens = rng.integers(max_len // 4, max_len + 1, n).astype(np.int64)
    offs = rng.integers(0, total - max_len, n).astype(np.int64)
    wanted = int(lens.sum())
    tensors = [torch.zeros(int(m) + 16, dtype=torch.uint8, device="cuda") for m in lens]  # every range a tensor of its own
    ptr = np.array([t.data_ptr() for t in tensors], dtype=np.uint64)
    assert not (ptr & 15).any()
    k_same = (offs & 15).astype(np.uint64)
    k_odd = ((offs + 1 + np.arange(n) % 15) & 15).astype(np.uint64)

    def table_v(k):
        t = np.zeros(n, dtype=zxc_amd.RANGEV_DTYPE)
        t["offset"], t["len"], t["base"] = offs, lens, ptr + k
        return torch.from_numpy(t.view(np.uint8).copy()).to("cuda")

    tv_same, tv_odd = table_v(k_same), table_v(k_odd)
    d_one = np.zeros(n, dtype=np.int64)  # (b): one buffer, dst_off = offset (mod 16), 16 spare bytes between ranges
    at = 0
    for i in range(n):
        d_one[i] = at + int(offs[i] & 15)
        at = (int(d_one[i] + lens[i]) + 31) // 16 * 16
    cap = at
    one = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    t1 = np.zeros(n, dtype=zxc_amd.RANGE_DTYPE)
    t1["offset"], t1["len"], t1["dst_off"] = offs, lens, d_one
    t_one = torch.from_numpy(t1.view(np.uint8).copy()).to("cuda")
    ws = zxc_amd.decompress_rangesv_device_work_size(n, max_len, bs)
    assert ws == zxc_amd.decompress_ranges_device_work_size(n, max_len, bs) and ws > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n, dtype=torch.int64, device="cuda")
    views_one = [one[int(d): int(d + m)] for d, m in zip(d_one, lens)]
    views_same = [t[int(k): int(k + m)] for t, k, m in zip(tensors, k_same, lens)]
    views_odd = [t[int(k): int(k + m)] for t, k, m in zip(tensors, k_odd, lens)]

    def rangesv_same():
        zxc_amd.decompress_rangesv_device(arc.data_ptr(), n_arc, index.data_ptr(), tv_same.data_ptr(), n, max_len, bs, work.data_ptr(), ws,
                                          res.data_ptr(), sp)

    def rangesv_odd():
        zxc_amd.decompress_rangesv_device(arc.data_ptr(), n_arc, index.data_ptr(), tv_odd.data_ptr(), n, max_len, bs, work.data_ptr(), ws,
                                          res.data_ptr(), sp)

    def ranges_one():
        zxc_amd.decompress_ranges_device(arc.data_ptr(), n_arc, index.data_ptr(), t_one.data_ptr(), n, max_len, one.data_ptr(), cap, bs,
                                         work.data_ptr(), ws, res.data_ptr(), sp)

    def ranges_one_and_copies():
        ranges_one()
        for v, e in zip(views_one, views_same):
            e.copy_(v, non_blocking=True)

    variants = [("a rangesv, base = offset (mod 16)", rangesv_same, views_same, 0),
                ("b ranges, one buffer", ranges_one, views_one, cap),
                ("c ranges, one buffer + one copy per range", ranges_one_and_copies, views_same, cap),
                ("d rangesv, odd alignments", rangesv_odd, views_odd, 0)]

    def same(what):
        for name, fn, views, _ in variants:
            one.zero_()
            for t in tensors:
                t.zero_()
            res.zero_()
            fn()
            stream.synchronize()
            assert np.array_equal(res.cpu().numpy(), lens), (what, name)
            for i, v in enumerate(views):
                o = int(offs[i])
                assert torch.equal(v, d_src[o: o + int(lens[i])]), "%s: %s, range %d does not give the source" % (what, name, i)

    same("before timing")
    ms = devbench.alternating([fn for _, fn, _, _ in variants], a.runs, a.warmup, stream, "wall")
    same("after timing")
    med = [statistics.median(m) for m in ms]
    lines = []
    for (name, _, _, extra), m, wall in zip(variants, ms, med):
        walls = sorted(m)
        line = {"variant": name, "ranges": n, "min_len": int(lens.min()), "max_len": max_len, "corpus": "silesia mix", "level": a.level,
                "block_size": bs, "wanted_bytes": wanted, "archive_bytes": n_arc, "work_bytes": ws, "extra_hbm_bytes": extra, "runs": a.runs,
                "wall_ms": round(wall, 3), "wall_ms_p10": round(pct(walls, 0.1), 3), "wall_ms_p90": round(pct(walls, 0.9), 3),
                "wall_ms_min": round(walls[0], 3), "wall_ms_max": round(walls[-1], 3), "spread": round((walls[-1] - walls[0]) / wall, 4),
                "wanted_gbps": round(wanted / wall / 1e6, 2)}
        if name.startswith(("a ", "d ")):
            line["rate_over_b"] = round(med[1] / wall, 4)
            line["rate_over_c"] = round(med[2] / wall, 4)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--ranges", type=int, default=512)
    ap.add_argument("--max-len", type=int, default=1 << 20)
    ap.add_argument("--blocks", default="65536,524288", help="comma-separated block sizes")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_rangesv_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    L.zxc_compress_bound.restype = ctypes.c_uint64
    L.zxc_compress_bound.argtypes = [ctypes.c_size_t]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    total = a.mib << 20
    gen = min(total, CORPUS_BYTES)
    part = torch.frombuffer(bytearray(corpus.synth_silesia(gen, seed=3)), dtype=torch.uint8).to("cuda")
    d_src = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    for at in range(0, total, gen):
        d_src[at: min(at + gen, total)] = part[: min(gen, total - at)]
    for bs in (int(x) for x in a.blocks.split(",")):
        for line in case(d_src, total, bs, a, stream):
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
