"""What the append session costs against compress_device: the same corpus in device memory compressed by one compress_device call
(the baseline, measured in the same run) and by a session of appends of 16, 64 and 256 MiB (max_piece = the append), alternating
in one process. Level 3 of the silesia mix (zxc_amd/corpus.py; 64 MiB of it, repeated to 1 GiB by default), at 64 KiB and 512 KiB
blocks. Wall-clock from the first enqueue to the stream's end, and hipEvent time on the stream; warm-up runs, then --runs timed
repetitions; medians and p10 / p90 of the wall times. Every session's archive is compared with compress_device's before and after
the timed runs. One JSON line per (block size, call) with its source GB/s and its work-area size, printed and appended to --out.

    python tools/bench_compress_append_device.py [--bytes 1073741824] [--appends 16,64,256] [--blocks 65536,524288] [--level 3]
                                                 [--runs 7] [--warmup 2] [--out profiles/compress_append_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from devbench import alternating, pct  # noqa: E402  (per function [(wall ms, event ms) per run])
from zxc_amd import corpus  # noqa: E402

CORPUS_BYTES = 64 << 20  # generated once; a larger source repeats it


def case(d_src, total, bs, appends, a, stream):
    sp = stream.cuda_stream
    cap = int(zxc_amd.lib().zxc_compress_bound(total))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    out_1 = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_s = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ws_1 = zxc_amd.compress_device_work_size(total, a.level, bs, True, False)
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    src_p = d_src.data_ptr()

    def whole():
        zxc_amd.compress_device(src_p, total, out_1.data_ptr(), cap, work_1.data_ptr(), ws_1, res.data_ptr(), a.level, bs, True, False, sp)

    sessions = []
    for step in appends:
        ws = zxc_amd.compress_append_device_work_size(total, step, a.level, bs, True, False)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")

        def session(step=step, ws=ws, work=work):
            s = zxc_amd.compress_begin_device(out_s.data_ptr(), cap, total, step, work.data_ptr(), ws, a.level, bs, True, False, sp)
            for at in range(0, total, step):
                s.append(src_p + at, min(step, total - at), sp)
            s.end(res.data_ptr(), sp)

        sessions.append((step, ws, work, session))

    def same(what):
        """every session's archive against compress_device's"""
        whole()
        stream.synchronize()
        size = int(res.item())
        assert size > 0, size
        for step, _, _, fn in sessions:
            out_s.zero_()
            fn()
            stream.synchronize()
            assert int(res.item()) == size, (what, step, int(res.item()), size)
            assert torch.equal(out_s[:size], out_1[:size]), "%s: the archive of appends of %d bytes differs from compress_device's" % (what, step)
        return size

    size = same("before timing")
    ms = alternating([whole] + [fn for _, _, _, fn in sessions], a.runs, a.warmup, stream)
    assert same("after timing") == size
    lines = []
    for (call, step, ws), m in zip([("compress_device", 0, ws_1)] + [("append session", st, ws) for st, ws, _, _ in sessions], ms):
        walls = sorted(w for w, _ in m)
        wall, ev = statistics.median(walls), statistics.median(e for _, e in m)
        lines.append({"call": call, "append_bytes": step, "corpus": "silesia mix", "level": a.level, "block_size": bs, "source_bytes": total,
                      "archive_bytes": size, "work_bytes": ws, "runs": a.runs, "wall_ms": round(wall, 3), "wall_ms_p10": round(pct(walls, 0.1), 3),
                      "wall_ms_p90": round(pct(walls, 0.9), 3), "event_ms": round(ev, 3), "source_gbps": round(total / wall / 1e6, 2)})
    for line in lines[1:]:
        line["wall_over_compress_device"] = round(line["wall_ms"] / lines[0]["wall_ms"], 3)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--appends", default="16,64,256", help="comma-separated append sizes in MiB")
    ap.add_argument("--blocks", default="65536,524288", help="comma-separated block sizes")
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_append_device_bench.jsonl"))
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
    d_src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for at in range(0, total, gen):
        d_src[at: min(at + gen, total)] = part[: min(gen, total - at)]
    appends = [int(x) << 20 for x in a.appends.split(",")]
    for bs in (int(x) for x in a.blocks.split(",")):
        for line in case(d_src, total, bs, appends, a, stream):
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
