"""What a table of tensors costs the inverse byte-shuffle calls on tensors that lie in HBM (include/zxc_mi355x_unshufflev.h),
alternating in one process:
  (a) unshufflev_device  against  unshuffle_device  on the same bytes lying contiguous, a buffer past the Infinity Cache, per element
      size and table: 1 entry, entries of 4 MiB, entries of 4 KiB (the entries are the slots of one buffer in a seeded random order,
      so consecutive entries are not neighbours; the reference kernel writes the buffer front to back). hipEvent time of the whole
      call (the scan's three kernels, the scatter-un-shuffle kernel, the status store); GB/s of bytes read plus bytes written; the
      ratio.
  (b) decompress_shufflev_device  against  the two paths a caller had before, on seeded bf16 weights N(0, 0.02) in --tensors tensors
      of their own, per block size: decompress_shuffle_device into a fresh contiguous buffer plus one copy_ per tensor, and one
      decompress_rangesv_shuffle_device over all tensors (an index opened once, outside the timed region). Wall-clock from the
      first enqueue to the stream's end, and the extra device memory of each path: the contiguous copy plus the work area, the
      ranges call's work area plus its index and table, against the new call's work area alone. Every tensor of every path is
      compared with the source before the timed runs.
Warm-up runs, then --runs timed repetitions; medians and p10 / p90. One JSON line per row, printed and appended to --out. No
threshold gates anything.

    python tools/bench_decompress_shufflev_device.py [--mib 64] [--tensors 256] [--kernel-mib 1024] [--level 3]
                                                     [--blocks 524288,65536] [--runs 7] [--warmup 2]
                                                     [--out profiles/decompress_shufflev_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from bench_compress_shuffle_device import stats  # noqa: E402
from bench_compress_shufflev_device import table_of  # noqa: E402


def kernel_case(E, unit, src, dst, n, entry_bytes, a, stream):
    sp = stream.cuda_stream
    count = n // entry_bytes
    order = np.random.default_rng(a.seed).permutation(count) if count > 1 else np.zeros(1, dtype=np.int64)
    table = table_of([(dst.data_ptr() + int(k) * entry_bytes, entry_bytes) for k in order])
    size = zxc_amd.unshufflev_device_scratch_size(count)
    scratch = torch.empty(size, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def scattered():
        zxc_amd.unshufflev_device(src.data_ptr(), table.data_ptr(), count, n, E, unit, scratch.data_ptr(), size, res.data_ptr(), sp)

    def contiguous():
        zxc_amd.unshuffle_device(src.data_ptr(), dst.data_ptr(), n, E, unit, sp)

    # the sibling's bytes for a contiguous destination, cut by the table
    contiguous()
    want = dst.clone()
    dst.zero_()
    scattered()
    got = dst.view(count, entry_bytes)[torch.from_numpy(order).to("cuda")].reshape(-1)
    assert int(res.item()) == 0 and torch.equal(got, want), (E, entry_bytes)
    del got, want
    torch.cuda.empty_cache()
    ms = devbench.alternating([scattered, contiguous], a.runs, a.warmup, stream, "event")
    line = {"kind": "kernel", "elem_size": E, "unit": unit, "bytes": n, "entries": count, "entry_bytes": entry_bytes, "runs": a.runs,
            "scratch_bytes": size}
    for prefix, m in zip(("unshufflev", "unshuffle"), ms):
        line.update(stats(m, 2 * n, prefix))  # bytes read plus bytes written
    line["unshufflev_over_unshuffle"] = round(line["unshufflev_ms"] / line["unshuffle_ms"], 3)
    return line


def archive_case(tensors, n, level, bs, a, stream):
    sp = stream.cuda_stream
    E, count, each = 2, len(tensors), tensors[0].numel()
    cap = int(zxc_amd.lib().zxc_compress_bound(n))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    # the archive: the state dict as it lies, seekable for the ranges call
    ws = zxc_amd.compress_shufflev_device_work_size(count, n, 0, 0, level, bs, True, False)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    src_table = table_of([(t.data_ptr(), t.numel()) for t in tensors])
    zxc_amd.compress_shufflev_device(src_table.data_ptr(), count, n, E, arc.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), 0, None, level,
                                     bs, True, False, sp)
    n_arc = int(res.item())
    assert n_arc > 0
    del work
    outs = [[torch.zeros_like(t) for t in tensors] for _ in range(3)]  # the fresh allocations of each path
    # path 1: one contiguous buffer, then a copy per tensor
    ws_s = zxc_amd.decompress_shuffle_device_work_size(n_arc, n, 0, bs)
    # path 2: one ranges call over all tensors
    nb = -(-n // bs)
    isz = zxc_amd.seekable_index_size(nb)
    index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    zxc_amd.seekable_open_device(arc.data_ptr(), n_arc, bs, nb, index.data_ptr(), isz, sp)
    ranges = np.zeros(count, dtype=zxc_amd.RANGEV_DTYPE)
    for r, t in enumerate(outs[1]):
        ranges[r] = (r * each, each, t.data_ptr())
    d_ranges = torch.from_numpy(ranges.view(np.uint8).copy()).to("cuda")
    ws_r = zxc_amd.decompress_rangesv_shuffle_device_work_size(count, each, bs)
    results = torch.zeros(count, dtype=torch.int64, device="cuda")
    # the new call
    ws_v = zxc_amd.decompress_shufflev_device_work_size(count, n_arc, n, 0, bs)
    dst_table = table_of([(t.data_ptr(), t.numel()) for t in outs[2]])
    assert min(ws_s, ws_r, ws_v) > 0
    work = torch.empty(max(ws_s, ws_r, ws_v), dtype=torch.uint8, device="cuda")

    def shuffle_then_copies():
        flat = torch.empty(n, dtype=torch.uint8, device="cuda")  # the copy the new call does without
        zxc_amd.decompress_shuffle_device(arc.data_ptr(), n_arc, flat.data_ptr(), n, E, bs, work.data_ptr(), ws_s, res.data_ptr(), 0, None, False, sp)
        for r, t in enumerate(outs[0]):
            t.copy_(flat[r * each: (r + 1) * each])

    def rangesv():
        zxc_amd.decompress_rangesv_shuffle_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), count, each, E, bs, work.data_ptr(),
                                                  ws_r, results.data_ptr(), None, sp)

    def shufflev():
        zxc_amd.decompress_shufflev_device(arc.data_ptr(), n_arc, dst_table.data_ptr(), count, n, E, bs, work.data_ptr(), ws_v, res.data_ptr(), 0,
                                           None, False, sp)

    for k, fn in enumerate((shuffle_then_copies, rangesv, shufflev)):
        fn()
        stream.synchronize()
        assert k == 1 or int(res.item()) == n, (k, int(res.item()))
        assert k != 1 or bool((results == each).all()), k
        assert all(torch.equal(o, t) for o, t in zip(outs[k], tensors)), k
    ms = devbench.alternating([shuffle_then_copies, rangesv, shufflev], a.runs, a.warmup, stream, "wall")
    line = {"kind": "archive", "data": "bf16 weights", "elem_size": E, "bytes": n, "tensors": count, "level": level, "block_size": bs,
            "runs": a.runs, "ratio": round(n / n_arc, 4), "extra_bytes_shuffle_copies": n + ws_s,
            "extra_bytes_rangesv": ws_r + isz + d_ranges.numel(), "extra_bytes_shufflev": ws_v}
    for prefix, m in zip(("shuffle_copies", "rangesv", "shufflev"), ms):
        line.update(stats(m, n, prefix))
    line["shufflev_over_shuffle_copies"] = round(line["shufflev_ms"] / line["shuffle_copies_ms"], 3)
    line["shufflev_over_rangesv"] = round(line["shufflev_ms"] / line["rangesv_ms"], 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--tensors", type=int, default=256)
    ap.add_argument("--kernel-mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--blocks", default="524288,65536", help="comma-separated block sizes")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_shufflev_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    L.zxc_compress_bound.restype = ctypes.c_uint64
    L.zxc_compress_bound.argtypes = [ctypes.c_size_t]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    n = a.kernel_mib << 20
    if n:
        src = torch.randint(0, 256, (n,), device="cuda", dtype=torch.uint8)
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        for E in (2, 4):
            for entry_bytes in (n, 4 << 20, 4096):
                emit(kernel_case(E, 524288, src, dst, n, min(entry_bytes, n), a, stream))
        del src, dst
        torch.cuda.empty_cache()
    n = a.mib << 20
    each = n // a.tensors // 2 * 2
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    tensors = [(torch.randn(each // 2, device="cuda", generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8) for _ in range(a.tensors)]
    n = each * a.tensors
    for bs in (int(x) for x in a.blocks.split(",")):
        emit(archive_case(tensors, n, a.level, bs, a, stream))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
