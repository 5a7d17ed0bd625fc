"""What compress_pack_device costs: n buffers of S bytes that lie in device memory, compressed by one pack call (archives back to
back, 16-byte aligned, no destination per item) and, beside it, by one compress_batch_device call over the same items with
destinations zxc_compress_bound apart. The batch call in the same run is the yardstick: the pack call runs the same encode and
gather and adds the size, scan and place passes over n_items words, so it should cost the batch call plus a few launches. Level 3
of the silesia mix (zxc_amd/corpus.py; 64 MiB of it, repeated where the area is larger) by default, over the shapes
N x S @ block size given with --shapes (those of tools/bench_compress_batch_device.py). Wall-clock from the first enqueue to the
stream's end, and hipEvent time on the stream; warm-up runs, then --runs timed repetitions with the two sides alternating;
medians, and the spread of both. Before the timed runs every archive of the pack call, found through d_packed, is compared with
the batch call's. Two JSON lines per shape (one per call), each with the destination bytes that call needs (*d_total for the
pack call, the sum of the bounds for the batch call), printed and appended to --out. There is no pass/fail threshold.

    python tools/bench_compress_pack_device.py [--shapes 4096x16384@4096,4096x65536@65536,512x1048576@65536] [--level 3] [--align 16]
                                               [--runs 7] [--warmup 2] [--out profiles/compress_pack_device_bench.jsonl]"""
import argparse
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
from bench_compress_batch_device import CORPUS_BYTES, SHAPES, alternating  # noqa: E402


def case(n, item, bs, a, stream):
    sp = stream.cuda_stream
    gen = min(item * n, CORPUS_BYTES) // item * item  # whole items of generated text, repeated to fill the area
    part = torch.frombuffer(bytearray(corpus.synth_silesia(gen, seed=3)), dtype=torch.uint8).to("cuda")
    d_src = torch.zeros(item * n + 64, dtype=torch.uint8, device="cuda")  # readable 64 bytes past the capacity
    for at in range(0, item * n, gen):
        d_src[at: min(at + gen, item * n)] = part[: min(gen, item * n - at)]
    L = zxc_amd.lib()
    cap = int(L.zxc_compress_bound(item))
    stride = (cap + 15) // 16 * 16
    dst_cap = n * stride  # what the batch call needs; the pack call gets the same area and reports what it used
    table = np.zeros(n, dtype=zxc_amd.ITEM_DTYPE)
    table["src_off"], table["src_size"] = np.arange(n, dtype=np.uint64) * item, item
    table["dst_off"], table["dst_capacity"] = np.arange(n, dtype=np.uint64) * stride, cap
    d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")  # the same table for both calls
    out_b = torch.zeros(dst_cap, dtype=torch.uint8, device="cuda")
    out_p = torch.zeros(dst_cap, dtype=torch.uint8, device="cuda")
    res_b = torch.zeros(n, dtype=torch.int64, device="cuda")
    res_p = torch.zeros(n, dtype=torch.int64, device="cuda")
    packed = torch.zeros(n, 4, dtype=torch.int64, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws_b = zxc_amd.compress_batch_device_work_size(n, item, a.level, bs, True, False)
    ws_p = zxc_amd.compress_pack_device_work_size(n, item, a.level, bs, True, False)
    work_b = torch.empty(ws_b, dtype=torch.uint8, device="cuda")
    work_p = torch.empty(ws_p, dtype=torch.uint8, device="cuda")

    def batch():
        zxc_amd.compress_batch_device(d_src.data_ptr(), item * n, d_items.data_ptr(), n, item, out_b.data_ptr(), dst_cap, work_b.data_ptr(),
                                      ws_b, res_b.data_ptr(), a.level, bs, True, False, sp)

    def pack():
        zxc_amd.compress_pack_device(d_src.data_ptr(), item * n, d_items.data_ptr(), n, item, out_p.data_ptr(), dst_cap, a.align,
                                     work_p.data_ptr(), ws_p, packed.data_ptr(), res_p.data_ptr(), d_total.data_ptr(), a.level, bs, True,
                                     False, sp)

    batch()
    pack()
    stream.synchronize()
    assert int(res_b.min().item()) > 0 and torch.equal(res_b, res_p), "the pack call's archive sizes differ from the batch call's"
    assert torch.equal(packed[:, 1], res_p) and torch.equal(packed[:, 2:], d_items.view(torch.int64).view(n, 4)[:, :2])
    total = int(d_total.item())
    at = packed[:, 0]
    assert int(at[0].item()) == 0 and bool((at % a.align == 0).all()) and total == int((at[-1] + res_p[-1]).item())
    assert bool((at[1:] - (at[:-1] + res_p[:-1]) < a.align).all()) and bool((at[1:] >= at[:-1] + res_p[:-1]).all())
    col = torch.arange(stride, device="cuda")[None, :]
    keep = col < res_b[:, None]  # the bytes of each archive
    rows = 256  # (the index matrix of the packed side, a slab of items at a time)
    for r0 in range(0, n, rows):
        k = keep[r0: r0 + rows]
        idx = (at[r0: r0 + rows, None] + col)[k]
        assert torch.equal(out_p[idx], out_b.view(n, stride)[r0: r0 + rows][k]), "the pack call's archives differ from the batch call's"
    archive_bytes = int(res_b.sum().item())
    del keep, col
    ms = alternating((pack, batch), a.runs, a.warmup, stream)
    source = item * n
    lines = []
    for kind, m, ws, dst_bytes in (("pack", ms[0], ws_p, total), ("batch", ms[1], ws_b, dst_cap)):
        walls, evs = sorted(w for w, _ in m), sorted(e for _, e in m)
        wall, ev = statistics.median(walls), statistics.median(evs)
        lines.append({"call": "compress_pack_device" if kind == "pack" else "compress_batch_device", "corpus": "silesia mix",
                      "level": a.level, "items": n, "item_bytes": item, "block_size": bs, "align": a.align, "source_bytes": source,
                      "archive_bytes": archive_bytes, "dst_bytes_needed": dst_bytes, "d_total": total, "sum_of_bounds": n * cap,
                      "work_bytes": ws, "runs": a.runs, "wall_ms": round(wall, 3), "wall_ms_min": round(walls[0], 3),
                      "wall_ms_max": round(walls[-1], 3), "event_ms": round(ev, 3), "event_ms_min": round(evs[0], 3),
                      "event_ms_max": round(evs[-1], 3), "source_gbps": round(source / wall / 1e6, 2)})
    lines[0]["wall_over_batch"] = round(lines[0]["wall_ms"] / lines[1]["wall_ms"], 3)
    lines[0]["event_over_batch"] = round(lines[0]["event_ms"] / lines[1]["event_ms"], 3)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated ITEMSxBYTES@BLOCK_SIZE")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--align", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_pack_device_bench.jsonl"))
    a = ap.parse_args()
    shapes = []
    for s in a.shapes.split(","):
        n, rest = s.split("x")
        item, bs = rest.split("@")
        shapes.append((int(n), int(item), int(bs)))
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    for n, item, bs in shapes:
        for line in case(n, item, bs, a, stream):
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
