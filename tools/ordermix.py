#!/usr/bin/env python3
"""Launch order A/B on the bench workload (GPU box only; needs an experiment build: tools/build_variant.sh order, the shim then
reads ZXC_EXP_ORDER_SLOTS on every launch: 0 = heaviest first, 0xFFFFFFFF = file order, else the residency zxc_dev_order_mix
mixes the head of the launch for). One process, one library, the variants alternating:
  sorted / file / mix (tail = OM_TAILS x residency)   the whole launch in each order
  heavy + middle + light                              the launch cut by order_bucket into three of equal summed n_seq, each a
                                                      launch of its own (heaviest first): what homogeneous residency costs
Every variant's bytes are checked once before the timing (OM_ROUNDS rounds of 5 launches per variant behind
OM_WARM untimed rounds). Env: AB_TILES (41), AB_LEVEL (3), OM_ROUNDS (4), OM_WARM (1), OM_TAILS ("2").
  --times   with a -DEXP_TIMES build: decoded bytes per ms and residency in 20 time bins of one launch per order, and the
            least-squares fit of block time on n_seq and n_lit (the cost key of the launch-order pass)
  --groups  the three homogeneous launches once each and nothing else (under rocprofv3 --pmc: the last three lean dispatches)"""
import os, sys
os.environ["ZXC_LIB_VARIANT"] = os.environ.get("ZXC_LIB_VARIANT", "libzxc_order.so"); os.environ["ZXC_TOOLS_AB"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BS = 65536


def headers(comp, off, sizes):
    """type, n_seq, n_lit, enc_lit, enc_tok of every block, and order_bucket's value (zxc_decode_kernel.hip)"""
    import numpy as np
    ok = sizes >= 20
    o = np.where(ok, off, 0).astype(np.int64)
    u32 = lambda at: sum(comp[o + at + k].astype(np.uint32) << (8 * k) for k in range(4))
    typ = comp[o]; n_seq = u32(8); n_lit = u32(12); enc_lit = comp[o + 16]; enc_tok = comp[o + 17]
    lz = ok & ((typ == 1) | (typ == 2))
    cost = n_seq + np.where(enc_tok == 2, n_seq, 0) + np.where(enc_lit == 1, n_lit >> 4, 0) + np.where(enc_lit >= 2, n_lit >> 2, 0)
    cost = np.where(lz, cost, 0).astype(np.uint64)
    bucket = 63 - np.minimum(cost * 320 // BS, 63).astype(np.int64)
    return lz, np.where(lz, n_seq, 0).astype(np.int64), np.where(lz, n_lit, 0).astype(np.int64), bucket


def main():
    import multiprocessing as mp
    import numpy as np, torch, zxc_amd, bench
    from zxc_amd import corpus
    tiles = int(os.environ.get("AB_TILES", "41")); level = int(os.environ.get("AB_LEVEL", "3"))
    rounds = int(os.environ.get("OM_ROUNDS", "4")); tails = [float(t) for t in os.environ.get("OM_TAILS", "2").split(",")]
    dev = torch.device("cuda", 0)
    with mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1)) as pool:
        d_comp, sizes, d_want, *_ = bench.build_rank_corpus(0, tiles * (corpus.TILE_BYTES // BS), level, BS, pool, dev)
    n = sizes.size
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))[:-1]]).astype(np.uint64)
    lz, n_seq, n_lit, bucket = headers(d_comp.cpu().numpy(), off, sizes)
    jobs = np.zeros(n, dtype=zxc_amd.api.JOB_DTYPE)
    jobs["comp_size"] = sizes; jobs["comp_off"] = off; jobs["out_off"] = np.arange(n, dtype=np.uint64) * BS; jobs["out_len"] = BS
    by_weight = np.argsort(bucket, kind="stable")
    cum = np.cumsum(n_seq[by_weight]); cuts = np.searchsorted(cum, [cum[-1] / 3, 2 * cum[-1] / 3])
    groups = dict(zip(("heavy", "middle", "light"), np.split(by_weight, cuts)))
    to_dev = lambda j: torch.frombuffer(bytearray(j.tobytes()), dtype=torch.uint8).to(dev)
    tables = {"all": (to_dev(jobs), n, np.arange(n))}
    for name, idx in groups.items():
        idx = np.sort(idx); tables[name] = (to_dev(jobs[idx]), idx.size, idx)
        print(f"group {name:6s}: {idx.size:6d} blocks, buckets {bucket[idx].min()}..{bucket[idx].max()}, sum n_seq {n_seq[idx].sum()}, "
              f"mean n_lit {n_lit[idx].mean():.0f}, RAW or other {int((~lz[idx]).sum())}", flush=True)
    d_out = torch.zeros(n * BS + 256, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    src = open(os.path.join(ROOT, "zxc_amd", "csrc", "zxc_decode_kernel.hip")).read()
    # (the lean kernel's residency as its launch bounds give it; the product asks the runtime)
    occ = torch.cuda.get_device_properties(0).multi_processor_count * 4 * int(src.split("#define LEAN_WAVES_PER_SIMD ")[1].split()[0])
    warm = int(os.environ.get("OM_WARM", "1"))

    def launch(table, order_slots):
        os.environ["ZXC_EXP_ORDER_SLOTS"] = str(order_slots)
        d_jobs, cnt, _ = tables[table]
        rc = zxc_amd.decode_blocks_device(d_comp.data_ptr(), d_jobs.data_ptr(), cnt, d_out.data_ptr(), d_st.data_ptr(), BS, False, stream)
        assert not rc, rc

    variants = {"sorted": [("all", 0)], "file": [("all", 0xFFFFFFFF)]}
    for t in tails: variants[f"mix T={t:g}x"] = [("all", max(1, int(occ * t / 2)))]
    variants["thirds"] = [(g, 0) for g in groups]
    if "--groups" in sys.argv:
        launch("all", 0); torch.cuda.synchronize()
        for g in groups: launch(g, 0); torch.cuda.synchronize()
        return
    if "--times" in sys.argv:
        for name in ("sorted", "file", f"mix T={tails[0]:g}x"):
            (table, slots), = variants[name]
            launch(table, slots); launch(table, slots); torch.cuda.synchronize()
            st = d_st.cpu().numpy().view(np.uint32)
            start = (st >> 16).astype(np.int64); dur = (st & 0xFFFF).astype(np.float64) * 0.32
            piv = int(np.median(start)); start = (((start - piv + 0x8000) & 0xFFFF) - 0x8000).astype(np.float64) * 0.32
            start -= start.min(); end = start + dur; T = end.max(); edges = np.linspace(0, T, 21)
            share = [(np.minimum(end, edges[i + 1]) - np.maximum(start, edges[i])).clip(0) for i in range(20)]
            print(f"{name}: span {T:.0f} us, mean block {dur.mean():.1f} us, p50 {np.percentile(dur, 50):.0f}, p99 {np.percentile(dur, 99):.0f}, max {dur.max():.0f}")
            print("  decoded MB per ms, per bin:", " ".join(f"{(s / np.maximum(dur, 0.32)).sum() * BS / (T / 20) / 1e3:.0f}" for s in share))
            print("  residency per bin:         ", " ".join(f"{s.sum() / (T / 20):.0f}" for s in share))
            print("  mean n_seq resident:       ", " ".join(f"{(s * n_seq).sum() / max(s.sum(), 1e-9):.0f}" for s in share))
            print("  mean n_lit resident:       ", " ".join(f"{(s * n_lit).sum() / max(s.sum(), 1e-9):.0f}" for s in share))
            A = np.stack([n_seq[lz], n_lit[lz], np.ones(int(lz.sum()))], axis=1).astype(np.float64)
            (a, b, c), *_ = np.linalg.lstsq(A, dur[lz], rcond=None)
            print(f"  block us ~ {a:.5f} n_seq + {b:.6f} n_lit + {c:.2f}: cost key n_seq + n_lit / {a / b if b > 0 else float('inf'):.1f}", flush=True)
        return
    for name, parts in variants.items():  # every byte, once per variant
        d_out.zero_(); d_st.zero_()
        ok = True
        for table, slots in parts:
            launch(table, slots); torch.cuda.synchronize()
            ok = ok and bool((d_st[:tables[table][1]] == BS).all().item())
        ok = ok and torch.equal(d_out[:n * BS], d_want)
        print(f"check {name:10s} ok={ok}", flush=True)
        assert ok
    ms = {name: [] for name in variants}
    for r in range(-warm, rounds):  # (the untimed rounds in front: clocks and caches settle in them)
        for name, parts in variants.items():
            for table, slots in parts: launch(table, slots)  # (the plan follows the stream's last launch: settle it)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                for table, slots in parts: launch(table, slots)
            e1.record(); torch.cuda.synchronize()
            if r >= 0: ms[name].append(e0.elapsed_time(e1) / 5)
    for name, v in ms.items():
        print(f"{name:10s} L{level} {n} blocks: ms per launch {' '.join(f'{x:.3f}' for x in v)} | min {min(v):.3f} median {np.median(v):.3f} "
              f"spread {max(v) - min(v):.3f} | {n * BS / np.median(v) / 1e6:.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
