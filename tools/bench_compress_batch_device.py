"""What compress_batch_device buys: n buffers of S bytes that lie in device memory, compressed by one batch call and, beside it, by
the only thing the library offered before, a loop of n compress_device calls on one stream over the same items. Level 3 of the
silesia mix (zxc_amd/corpus.py; 64 MiB of it, repeated where the area is larger) by default, over the shapes N x S @ block size
given with --shapes. Wall-clock from the first enqueue
to the stream's end, and hipEvent time on the stream; warm-up runs, then --runs timed repetitions with the two sides alternating;
medians, and the spread of the wall times. Before the timed runs every archive of the batch call is compared with the loop's.
Two JSON lines per shape (one for the batch call, one for the loop), each with its source GB/s, printed and appended to --out.

    python tools/bench_compress_batch_device.py [--shapes 4096x16384@4096,4096x65536@65536,512x1048576@65536] [--level 3]
                                                [--runs 7] [--warmup 2] [--out profiles/compress_batch_device_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from devbench import alternating  # noqa: E402  (per function [(wall ms, event ms) per run])
from zxc_amd import corpus  # noqa: E402

SHAPES = "4096x16384@4096,4096x65536@65536,512x1048576@65536"
CORPUS_BYTES = 64 << 20  # generated once per shape; larger areas repeat it


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
    dst_cap = n * stride
    table = np.zeros(n, dtype=zxc_amd.ITEM_DTYPE)
    table["src_off"], table["src_size"] = np.arange(n, dtype=np.uint64) * item, item
    table["dst_off"], table["dst_capacity"] = np.arange(n, dtype=np.uint64) * stride, cap
    d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    out = torch.zeros(dst_cap, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws_b = zxc_amd.compress_batch_device_work_size(n, item, a.level, bs, True, False)
    ws_1 = zxc_amd.compress_device_work_size(item, a.level, bs, True, False)
    work_b = torch.empty(ws_b, dtype=torch.uint8, device="cuda")
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    src_p, out_p, res_p = d_src.data_ptr(), out.data_ptr(), res.data_ptr()

    def batch():
        zxc_amd.compress_batch_device(src_p, item * n, d_items.data_ptr(), n, item, out_p, dst_cap, work_b.data_ptr(), ws_b, res_p, a.level, bs,
                                      True, False, sp)

    def loop():  # (one work area: calls on one stream run in order)
        w = work_1.data_ptr()
        for i in range(n):
            zxc_amd.compress_device(src_p + i * item, item, out_p + i * stride, cap, w, ws_1, res_p + 8 * i, a.level, bs, True, False, sp)

    seen = []
    for fn in (batch, loop):
        out.zero_()
        res.zero_()
        fn()
        stream.synchronize()
        assert int(res.min().item()) > 0, (fn.__name__, int(res.min().item()))
        seen.append((res.clone(), out.clone()))
    assert torch.equal(seen[0][0], seen[1][0]), "the batch call's archive sizes differ from the loop's"
    keep = torch.arange(stride, device="cuda")[None, :] < seen[0][0][:, None]  # the bytes of each archive
    assert torch.equal(seen[0][1].view(n, stride)[keep], seen[1][1].view(n, stride)[keep]), "the batch call's archives differ from the loop's"
    archive_bytes = int(seen[0][0].sum().item())
    del seen, keep
    ms = alternating((batch, loop), a.runs, a.warmup, stream)
    total = item * n
    lines = []
    for kind, m, ws in (("batch", ms[0], ws_b), ("loop", ms[1], ws_1)):
        walls = sorted(w for w, _ in m)
        wall, ev = statistics.median(walls), statistics.median(e for _, e in m)
        lines.append({"call": "compress_batch_device" if kind == "batch" else "loop of compress_device", "corpus": "silesia mix",
                      "level": a.level, "items": n, "item_bytes": item, "block_size": bs, "source_bytes": total,
                      "archive_bytes": archive_bytes, "work_bytes": ws, "runs": a.runs, "wall_ms": round(wall, 3),
                      "wall_ms_min": round(walls[0], 3), "wall_ms_max": round(walls[-1], 3), "event_ms": round(ev, 3),
                      "source_gbps": round(total / wall / 1e6, 2)})
    lines[0]["speedup_wall_over_loop"] = round(lines[1]["wall_ms"] / lines[0]["wall_ms"], 2)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated ITEMSxBYTES@BLOCK_SIZE")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_batch_device_bench.jsonl"))
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
