"""What decompress_batch_device buys: n small archives that lie in device memory, decoded by one batch call and, beside it, by the
only thing the library offered before, a loop of n decompress_device calls on one stream over the same items. Items of 4 KiB,
64 KiB and 256 KiB of the level-3 silesia mix (zxc_amd/corpus.py), one archive each (block size min(item, 64 KiB)), and at 4 KiB
also with a 32 KiB dictionary in device memory (decompress_batch_dict_device beside a loop of decompress_dict_device).
Wall-clock from the first enqueue to the stream's end, and hipEvent time on the stream; warm-up runs, then --runs timed
repetitions with the two sides alternating; medians. Every decoded byte is checked against the source before the timed runs. One
JSON line per case, printed and appended to --out.

    python tools/bench_batch_device.py [--items 2048,1024,256] [--runs 7] [--warmup 2]
                                       [--out profiles/decompress_batch_device_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from zxc_amd import corpus  # noqa: E402

ITEM_BYTES = (4096, 65536, 262144)
DICT_BYTES = 32768


def alternating(fns, runs, warmup, stream):
    """-> per function (median wall ms, median event ms, p10 and p90 of the wall ms); run i times every function once, in turn"""
    ms = devbench.alternating(fns, runs, warmup, stream)
    walls = [sorted(w for w, _ in m) for m in ms]
    return [(statistics.median(w), statistics.median(e for _, e in m), devbench.pct(w, 0.1), devbench.pct(w, 0.9)) for m, w in zip(ms, walls)]


def case(item, n, content, a, stream):
    sp = stream.cuda_stream
    bs = min(item, 65536)
    data = corpus.synth_silesia(item * n, seed=3)
    arcs = [zxc_amd.compress(data[i * item: (i + 1) * item], 3, bs, True, False, dict_=content) for i in range(n)]
    # the source area: every archive 16-byte aligned and readable 64 bytes past its end
    offs, at = [], 0
    for c in arcs:
        offs.append(at)
        at = (at + len(c) + 64 + 15) // 16 * 16
    area = np.zeros(at + 64, dtype=np.uint8)
    for o, c in zip(offs, arcs):
        area[o: o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    d_src = torch.from_numpy(area).to("cuda")
    cap = item + 32  # (every block decodes straight into the destination on both sides)
    stride = (cap + 15) // 16 * 16
    dst_cap = n * stride
    table = np.zeros(n, dtype=zxc_amd.ITEM_DTYPE)
    table["src_off"], table["src_size"] = offs, [len(c) for c in arcs]
    table["dst_off"], table["dst_capacity"] = np.arange(n, dtype=np.uint64) * stride, cap
    d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    want = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda").view(n, item)
    out = torch.zeros(dst_cap, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws_b = zxc_amd.decompress_batch_device_work_size(n, cap, bs)
    ws_1 = max(zxc_amd.decompress_device_work_size(len(c), cap, bs) for c in arcs)
    work_b = torch.empty(ws_b, dtype=torch.uint8, device="cuda")
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    dd = None
    if content:
        d_content = torch.frombuffer(bytearray(content), dtype=torch.uint8).to("cuda")
        d_id = torch.zeros(1, dtype=torch.int32, device="cuda")
        zxc_amd.dict_prepare_device(d_content.data_ptr(), len(content), 0, d_id.data_ptr(), sp)
        dd = (d_content.data_ptr(), len(content), 0, d_id.data_ptr())
    src_p, out_p, res_p = d_src.data_ptr(), out.data_ptr(), res.data_ptr()
    sizes = [len(c) for c in arcs]

    def batch():
        if dd:
            zxc_amd.decompress_batch_dict_device(src_p, at, d_items.data_ptr(), n, cap, out_p, dst_cap, bs, dd, work_b.data_ptr(), ws_b, res_p,
                                                 False, sp)
        else:
            zxc_amd.decompress_batch_device(src_p, at, d_items.data_ptr(), n, cap, out_p, dst_cap, bs, work_b.data_ptr(), ws_b, res_p, False, sp)

    def loop():  # (one work area: calls on one stream run in order)
        w = work_1.data_ptr()
        for i in range(n):
            if dd:
                zxc_amd.decompress_dict_device(src_p + offs[i], sizes[i], out_p + i * stride, cap, bs, dd, w, ws_1, res_p + 8 * i, False, sp)
            else:
                zxc_amd.decompress_device(src_p + offs[i], sizes[i], out_p + i * stride, cap, bs, w, ws_1, res_p + 8 * i, False, sp)

    for fn in (batch, loop):
        out.zero_()
        res.zero_()
        fn()
        stream.synchronize()
        assert int(res.min().item()) == item == int(res.max().item()), (fn.__name__, int(res.min().item()))
        assert torch.equal(out.view(n, stride)[:, :item], want), fn.__name__
    (b_wall, b_ev, b_p10, b_p90), (l_wall, l_ev, l_p10, l_p90) = alternating((batch, loop), a.runs, a.warmup, stream)
    total = item * n
    return {"corpus": "silesia mix, level 3", "item_bytes": item, "items": n, "block_size": bs, "dict_bytes": len(content) if content else 0,
            "source_bytes": total, "archive_bytes": sum(sizes), "runs": a.runs, "batch_work_bytes": ws_b,
            "batch_wall_ms": round(b_wall, 3), "batch_wall_ms_p10": round(b_p10, 3), "batch_wall_ms_p90": round(b_p90, 3), "batch_event_ms": round(b_ev, 3), "batch_gbps": round(total / b_wall / 1e6, 2),
            "loop_wall_ms": round(l_wall, 3), "loop_wall_ms_p10": round(l_p10, 3), "loop_wall_ms_p90": round(l_p90, 3), "loop_event_ms": round(l_ev, 3), "loop_gbps": round(total / l_wall / 1e6, 2),
            "speedup_wall": round(l_wall / b_wall, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="2048,1024,256", help="item counts for 4 KiB, 64 KiB and 256 KiB items")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_batch_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    counts = [int(x) for x in a.items.split(",")]
    content = corpus.synth_silesia(DICT_BYTES, seed=11)
    cases = [(item, n, None) for item, n in zip(ITEM_BYTES, counts)] + [(ITEM_BYTES[0], counts[0], content)]
    for item, n, dic in cases:
        text = json.dumps(case(item, n, dic, a, stream))
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
