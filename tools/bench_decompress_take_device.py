"""What the take session costs against decompress_device: a level-3 seekable archive of the bench corpus in device memory, decoded
(a) by one decompress_device call into one buffer, (b) by that call plus the per-piece device copies a caller with a list of
tensors needs today, (c) by a session with 16-byte aligned pieces (the direct path) and (d) by a session with pieces at odd
addresses (everything through slots and the copy-out), alternating in one process. Silesia mix (zxc_amd/corpus.py; 64 MiB of it,
repeated to --bytes), 64 KiB blocks, pieces of 64 MiB. Wall-clock from the first enqueue to the stream's end, and hipEvent time on
the stream; warm-up runs, then --runs timed repetitions; medians and p10 / p90 of the wall times. Every variant's bytes are compared
with the source before and after the timed runs. One JSON line per variant with its decoded GB/s and the HBM it needs besides the
archive and the pieces, printed and appended to --out.

    python tools/bench_decompress_take_device.py [--bytes 1073741824] [--piece 64] [--block 65536] [--level 3] [--runs 7] [--warmup 2]
                                                 [--out profiles/decompress_take_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from devbench import once, pct  # noqa: E402  (once: (wall ms, event ms))
from zxc_amd import corpus  # noqa: E402

CORPUS_BYTES = 64 << 20  # generated once; a larger source repeats it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--piece", type=int, default=64, help="piece size in MiB")
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decompress_take_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    L.zxc_compress_bound.restype = ctypes.c_uint64
    L.zxc_compress_bound.argtypes = [ctypes.c_size_t]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    total, bs, piece = a.bytes, a.block, a.piece << 20
    gen = min(total, CORPUS_BYTES)
    part = torch.frombuffer(bytearray(corpus.synth_silesia(gen, seed=3)), dtype=torch.uint8).to("cuda")
    d_src = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    for at in range(0, total, gen):
        d_src[at: min(at + gen, total)] = part[: min(gen, total - at)]
    res = torch.zeros(1, dtype=torch.int64, device="cuda")

    # the archive, by compress_device
    cap = int(L.zxc_compress_bound(total))
    d_arc = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    ws_c = zxc_amd.compress_device_work_size(total, a.level, bs, True, False)
    work_c = torch.empty(ws_c, dtype=torch.uint8, device="cuda")
    zxc_amd.compress_device(d_src.data_ptr(), total, d_arc.data_ptr(), cap, work_c.data_ptr(), ws_c, res.data_ptr(), a.level, bs, True, False, sp)
    stream.synchronize()
    n_arc = int(res.item())
    assert n_arc > 0, n_arc
    del work_c
    torch.cuda.empty_cache()

    lens = [min(piece, total - at) for at in range(0, total, piece)]
    whole = torch.zeros(total, dtype=torch.uint8, device="cuda")
    aligned = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in lens]
    odd = [torch.zeros(n + 1, dtype=torch.uint8, device="cuda") for n in lens]
    ws_1 = zxc_amd.decompress_device_work_size(n_arc, total, bs)
    work_1 = torch.empty(ws_1, dtype=torch.uint8, device="cuda")
    ws_s = zxc_amd.decompress_take_device_work_size(n_arc, total, piece, bs)
    work_s = torch.empty(ws_s, dtype=torch.uint8, device="cuda")

    def one_buffer():
        zxc_amd.decompress_device(d_arc.data_ptr(), n_arc, whole.data_ptr(), total, bs, work_1.data_ptr(), ws_1, res.data_ptr(), False, sp)

    def one_buffer_and_copies():
        one_buffer()
        at = 0
        for t in aligned:
            t.copy_(whole[at: at + len(t)], non_blocking=True)
            at += len(t)

    def session(tensors, off):
        s = zxc_amd.decompress_begin_device(d_arc.data_ptr(), n_arc, total, piece, bs, work_s.data_ptr(), ws_s, False, sp)
        for t, n in zip(tensors, lens):
            s.take(t.data_ptr() + off, n, sp)
        s.end(res.data_ptr(), sp)

    variants = [("a decompress_device, one buffer", one_buffer, ws_1, lambda: whole),
                ("b decompress_device + per-piece copies", one_buffer_and_copies, ws_1 + total, lambda: torch.cat(aligned)),
                ("c take session, 16-aligned pieces", lambda: session(aligned, 0), ws_s, lambda: torch.cat(aligned)),
                ("d take session, odd pieces", lambda: session(odd, 1), ws_s, lambda: torch.cat([t[1:] for t in odd]))]

    def same(what):
        for name, fn, _, got in variants:
            for t in [whole] + aligned + odd:
                t.zero_()
            fn()
            stream.synchronize()
            assert int(res.item()) == total, (what, name, int(res.item()))
            assert torch.equal(got(), d_src[:total]), "%s: %s does not give the source" % (what, name)

    same("before timing")
    for _ in range(a.warmup):
        for _, fn, _, _ in variants:
            fn()
    stream.synchronize()
    ms = [[] for _ in variants]
    for _ in range(a.runs):
        for k, (_, fn, _, _) in enumerate(variants):
            ms[k].append(once(fn, stream))
    same("after timing")
    base = None
    for (name, _, extra, _), m in zip(variants, ms):
        walls = sorted(w for w, _ in m)
        wall, ev = statistics.median(walls), statistics.median(e for _, e in m)
        base = wall if base is None else base
        line = {"variant": name, "corpus": "silesia mix", "level": a.level, "block_size": bs, "decoded_bytes": total, "archive_bytes": n_arc,
                "piece_bytes": piece, "pieces": len(lens), "extra_hbm_bytes": extra, "runs": a.runs, "wall_ms": round(wall, 3),
                "wall_ms_p10": round(pct(walls, 0.1), 3), "wall_ms_p90": round(pct(walls, 0.9), 3), "event_ms": round(ev, 3),
                "decoded_gbps": round(total / wall / 1e6, 2), "wall_over_a": round(wall / base, 3)}
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
