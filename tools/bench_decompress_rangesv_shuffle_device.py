"""What reading a byte-shuffled checkpoint back by range costs: --mib MiB of bf16 weights and of int64 ids made on the device
(the buffers of bench_compress_shuffle_device.py), each written as a level-3 seekable archive twice, by compress_shuffle_device and,
plain, by compress_device, and --ranges seeded ranges of the plain bytes (lengths uniform in [--max-len / 4, --max-len], any
offset), each with a destination tensor of its own, fetched by
  (a)  one decompress_rangesv_shuffle_device over the shuffled archive,
  (b)  today's path over the same archive, written out: the ranges rounded out to blocks on the host, one decompress_ranges_device
       of the supersets into one scratch buffer, one unshuffle_device per range into a second, one device copy per range into the
       tensors,
  (c)  one decompress_rangesv_device at odd alignments over the PLAIN archive of the same tensor: every block is staged there too,
       so it shows what the gather costs beside the copy-out (its decode launch reads other, larger blocks: the filter's gain),
alternating in one process, at 64 KiB and 512 KiB blocks. Wall-clock from the first enqueue to the stream's end; warm-up runs, then
--runs timed repetitions; medians with min and max. Every fetched byte of every variant is compared with the source before the
timed runs, and again after them. One JSON line per (data, block size, variant), with the time ratios (a)/(b) and (a)/(c) on (a)'s
line, printed and appended to --out. No threshold gates anything.

    python tools/bench_decompress_rangesv_shuffle_device.py [--mib 64] [--ranges 512] [--max-len 1048576] [--blocks 65536,524288]
                                                            [--level 3] [--runs 10] [--warmup 2]
                                                            [--out profiles/decompress_rangesv_shuffle_device_bench.jsonl]"""
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
from bench_compress_shuffle_device import buffers  # noqa: E402
from bench_decompress_device import archive_on_device  # noqa: E402


def shuffled_archive_on_device(src, n, E, level, bs, stream):
    """-> (tensor with compress_shuffle_device's archive and 64 readable bytes behind it, archive size)"""
    cap = int(zxc_amd.lib().zxc_compress_bound(n))
    ws = zxc_amd.compress_shuffle_device_work_size(n, 0, 0, level, bs, True, False)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    zxc_amd.compress_shuffle_device(src.data_ptr(), n, E, arc.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), 0, None, level, bs, True,
                                    False, stream.cuda_stream)
    size = int(res.item())
    assert size > 0, size
    return arc, size


def opened(arc, n_arc, bs, nb, stream):
    isz = zxc_amd.seekable_index_size(nb)
    index = torch.zeros((isz + 7) // 8, dtype=torch.int64, device="cuda")
    zxc_amd.seekable_open_device(arc.data_ptr(), n_arc, bs, nb, index.data_ptr(), isz, stream.cuda_stream)
    stream.synchronize()
    assert int(index[:1].cpu().numpy().view(np.int32)[0]) == 0, "open failed"
    return index


def case(name, E, d_src, total, bs, a, stream):
    sp = stream.cuda_stream
    nb = -(-total // bs)
    arc_s, n_s = shuffled_archive_on_device(d_src, total, E, a.level, bs, stream)
    arc_p, n_p = archive_on_device(d_src, total, a.level, bs, True, False, stream)
    index_s, index_p = opened(arc_s, n_s, bs, nb, stream), opened(arc_p, n_p, bs, nb, stream)

    rng = np.random.default_rng(a.seed + bs + E)
    n, max_len = a.ranges, a.max_len
    lens = rng.integers(max_len // 4, max_len + 1, n).astype(np.int64)
    offs = rng.integers(0, total - max_len, n).astype(np.int64)
    wanted = int(lens.sum())
    tensors = [torch.zeros(int(m) + 16, dtype=torch.uint8, device="cuda") for m in lens]  # every range a tensor of its own
    ptr = np.array([t.data_ptr() for t in tensors], dtype=np.uint64)
    assert not (ptr & 15).any()
    k_zero = np.zeros(n, dtype=np.uint64)
    k_odd = ((offs + 1 + np.arange(n) % 15) & 15).astype(np.uint64)  # base != offset (mod 16): rangesv stages every block

    def table_v(k):
        t = np.zeros(n, dtype=zxc_amd.RANGEV_DTYPE)
        t["offset"], t["len"], t["base"] = offs, lens, ptr + k
        return torch.from_numpy(t.view(np.uint8).copy()).to("cuda")

    tv_zero, tv_odd = table_v(k_zero), table_v(k_odd)
    ws_a = zxc_amd.decompress_rangesv_shuffle_device_work_size(n, max_len, bs)
    ws_c = zxc_amd.decompress_rangesv_device_work_size(n, max_len, bs)

    # (b): the supersets of whole blocks, back to back in one buffer (each a multiple of the block size, so 16-byte aligned)
    lo = offs // bs * bs
    hi = np.minimum((offs + lens + bs - 1) // bs * bs, total)
    sup = hi - lo
    at = np.concatenate(([0], np.cumsum(sup)[:-1])).astype(np.int64)
    cap, sup_max = int(sup.sum()), int(sup.max())
    t1 = np.zeros(n, dtype=zxc_amd.RANGE_DTYPE)
    t1["offset"], t1["len"], t1["dst_off"] = lo, sup, at
    t_one = torch.from_numpy(t1.view(np.uint8).copy()).to("cuda")
    ws_b = zxc_amd.decompress_ranges_device_work_size(n, sup_max, bs)
    assert ws_a > 0 and ws_b > 0 and ws_c > 0
    work = torch.empty(max(ws_a, ws_b, ws_c), dtype=torch.uint8, device="cuda")
    one, two = (torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = torch.zeros(n, dtype=torch.int64, device="cuda")
    views_two = [two[int(s + o - b): int(s + o - b + m)] for s, o, b, m in zip(at, offs, lo, lens)]
    views_zero = [t[: int(m)] for t, m in zip(tensors, lens)]
    views_odd = [t[int(k): int(k + m)] for t, k, m in zip(tensors, k_odd, lens)]
    sup_list = [(int(s), int(m)) for s, m in zip(at, sup)]

    def new_call():
        zxc_amd.decompress_rangesv_shuffle_device(arc_s.data_ptr(), n_s, index_s.data_ptr(), tv_zero.data_ptr(), n, max_len, E, bs,
                                                  work.data_ptr(), ws_a, res.data_ptr(), None, sp)

    def todays_path():
        zxc_amd.decompress_ranges_device(arc_s.data_ptr(), n_s, index_s.data_ptr(), t_one.data_ptr(), n, sup_max, one.data_ptr(), cap, bs,
                                         work.data_ptr(), ws_b, res.data_ptr(), sp)
        for s, m in sup_list:
            zxc_amd.unshuffle_device(one.data_ptr() + s, two.data_ptr() + s, m, E, bs, sp)
        for v, e in zip(views_two, views_zero):
            e.copy_(v, non_blocking=True)

    def rangesv_plain_odd():
        zxc_amd.decompress_rangesv_device(arc_p.data_ptr(), n_p, index_p.data_ptr(), tv_odd.data_ptr(), n, max_len, bs, work.data_ptr(), ws_c,
                                          res.data_ptr(), sp)

    variants = [("a rangesv_shuffle, shuffled archive", new_call, views_zero, lens, ws_a, 0, n_s, 1),
                ("b ranges + unshuffle per range + copy per range, shuffled archive", todays_path, views_zero, sup, ws_b, 2 * cap, n_s, 1 + 2 * n),
                ("c rangesv at odd alignments, plain archive", rangesv_plain_odd, views_odd, lens, ws_c, 0, n_p, 1)]

    def same(what):
        for vname, fn, views, want_res, *_ in variants:
            for t in tensors:
                t.zero_()
            res.zero_()
            fn()
            stream.synchronize()
            assert np.array_equal(res.cpu().numpy(), want_res), (what, vname)
            for i, v in enumerate(views):
                o = int(offs[i])
                assert torch.equal(v, d_src[o: o + int(lens[i])]), "%s: %s, range %d does not give the source" % (what, vname, i)

    same("before timing")
    ms = devbench.alternating([v[1] for v in variants], a.runs, a.warmup, stream, "wall")
    same("after timing")
    med = [statistics.median(m) for m in ms]
    lines = []
    for (vname, _, _, _, ws, extra, n_arc, calls), m, wall in zip(variants, ms, med):
        walls = sorted(m)
        line = {"variant": vname, "data": name, "elem_size": E, "bytes": total, "ranges": n, "min_len": int(lens.min()), "max_len": max_len,
                "level": a.level, "block_size": bs, "wanted_bytes": wanted, "archive_bytes": n_arc, "work_bytes": ws,
                "extra_hbm_bytes": extra, "host_calls": calls, "runs": a.runs, "wall_ms": round(wall, 3), "wall_ms_p10": round(devbench.pct(walls, 0.1), 3),
                "wall_ms_p90": round(devbench.pct(walls, 0.9), 3), "wall_ms_min": round(walls[0], 3),
                "wall_ms_max": round(walls[-1], 3), "spread": round((walls[-1] - walls[0]) / wall, 4),
                "wanted_gbps": round(wanted / wall / 1e6, 2)}
        if vname.startswith("a "):
            line["time_over_b"] = round(wall / med[1], 4)
            line["time_over_b_min_max"] = [round(walls[0] / max(ms[1]), 4), round(walls[-1] / min(ms[1]), 4)]
            line["time_over_c"] = round(wall / med[2], 4)
            line["time_over_c_min_max"] = [round(walls[0] / max(ms[2]), 4), round(walls[-1] / min(ms[2]), 4)]
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--ranges", type=int, default=512)
    ap.add_argument("--max-len", type=int, default=1 << 20)
    ap.add_argument("--blocks", default="65536,524288", help="comma-separated block sizes")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_rangesv_shuffle_device_bench.jsonl"))
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
    for name, E, d_src in buffers(total, a.seed):
        if not name.startswith(("bf16", "int64")):
            continue
        for bs in (int(x) for x in a.blocks.split(",")):
            for line in case(name, E, d_src, total, bs, a, stream):
                text = json.dumps(line)
                print(text, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
