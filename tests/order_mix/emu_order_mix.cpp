// emu_order_mix.cpp — the launch-order pass of zxc_amd/csrc with a residency of the caller's choice (zxc_dev_order_mix) in front
// of the decode kernels, on the CPU wave emulator (tests/wave_emu), for tests/test_order_mix_emu.py. Test infrastructure.
#include <functional>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "zxc_decode_kernel.hip"  // found via -I zxc_amd/csrc; <hip/hip_runtime.h> resolves to tests/wave_emu/hip/

namespace emu { void run_wave(const std::function<void()>& body, unsigned block, unsigned grid, int n_lanes); }
extern char __start_emu_lds[], __stop_emu_lds[];

// full_plan 0: the two-pass plan without section scratch (launch-order pass with its lists, RLE literals, lean kernel over every
// block, full kernel over its list); 1: the FULL plan with the launch-order pass (full kernel over every block through order[]).
// verify_trailer (two-pass plan): every block carries a checksum, verified by zxc_block_checksum_kernel beside the decode and merged.
// order_out[n_jobs] = order[]. -> bit 0 / 1: a store landed in the 4 KiB in front of / behind the output buffer.
extern "C" __attribute__((visibility("default")))
int emu_order_mix_decode(const uint8_t* comp, size_t comp_bytes, const zxc_dev_job_t* jobs, uint32_t n_jobs, uint8_t* out, size_t out_bytes,
                         int32_t* status, uint32_t block_size, uint32_t mix_slots, int full_plan, uint32_t* order_out, int verify_trailer) {
    std::vector<uint8_t> c(comp_bytes + 8192, 0xEE), o(out_bytes + 8192, 0xDD);
    memcpy(c.data() + 4096, comp, comp_bytes);
    memcpy(o.data() + 4096, out, out_bytes);
    const uint32_t stride = ZXC_DEV_SLOT_STRIDE(block_size), n_slots = 4, g256 = (n_jobs + 255u) / 256u;
    std::vector<uint8_t> scratch((size_t)n_slots * stride + 4096, 0xCC), rscratch(((size_t)4 << 20) + 4096, 0xC7);
    std::vector<uint32_t> busy(8192, 0);
    auto launch = [&](unsigned grid, int threads, const std::function<void()>& k) {
        for (unsigned g = 0; g < grid; g++) {
            memset(__start_emu_lds, 0xA5, (size_t)(__stop_emu_lds - __start_emu_lds));  // LDS is not zero at launch
            emu::run_wave(k, g, grid, threads);
        }
    };
    const zxc_dev_ord_layout_t at = zxc_dev_ord_layout(n_jobs);
    std::vector<uint32_t> buf(at.words, 0xA3A3A3A3u);  // poisoned except where the shim zeroes it
    memset(buf.data(), 0, 130u * 4u);
    memset(buf.data() + at.ctl, 0, ZXC_DEV_CTL_WORDS * 4u);
    uint32_t *order = buf.data() + at.order, *list = buf.data() + at.list, *ctl = buf.data() + at.ctl, *pre_entries = buf.data() + at.pre_ent;
    zxc_dev_sec_t* secs = (zxc_dev_sec_t*)(buf.data() + at.secs);
    zxc_dev_pre_t* pre = (zxc_dev_pre_t*)(buf.data() + at.pre);
    uint8_t* ck_bad = (uint8_t*)(buf.data() + at.ck_bad);
    const uint32_t tb = verify_trailer ? 4u | ZXC_DEV_TRAILER_ELSEWHERE : 0u;
    launch(g256, 256, [&] { zxc_order_hist_kernel(c.data() + 4096, jobs, n_jobs, block_size, buf.data()); });
    if (full_plan) {
        launch(g256, 256, [&] {
            zxc_order_scatter_kernel(c.data() + 4096, jobs, n_jobs, block_size, buf.data(), order, nullptr, 0u, nullptr, nullptr, nullptr, nullptr,
                                     0u, block_size + 2112u, 0u, mix_slots);
        });
        launch(n_jobs, 64, [&] {
            zxc_decode_blocks_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, 0u, scratch.data(), stride, 0u,
                                     busy.data(), n_slots, order, 0u, nullptr);
        });
    } else {
        launch(g256, 256, [&] {
            zxc_order_scatter_kernel(c.data() + 4096, jobs, n_jobs, block_size, buf.data(), order, list, tb & ~ZXC_DEV_TRAILER_ELSEWHERE, pre, ctl, pre_entries, secs, 0u,
                                     block_size + 2112u, (uint32_t)(((size_t)4 << 20) >> 4), mix_slots);
        });
        if (ctl[ZXC_DEV_CTL_RLE_LIST])
            launch(3u, 64, [&] { zxc_rle_expand_kernel(c.data() + 4096, jobs, pre, rscratch.data(), ctl + ZXC_DEV_CTL_RLE_LIST, pre_entries + n_jobs - 1u); });
        launch(n_jobs, 64, [&] {
            zxc_decode_blocks_lean_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, order, 0u, tb, pre, rscratch.data());
        });
        launch(n_jobs < 3u ? n_jobs : 3u, 64, [&] {
            zxc_decode_blocks_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, tb, scratch.data(), stride, 0u,
                                     busy.data(), n_slots, order, 0u, list);
        });
        if (verify_trailer) {
            launch((n_jobs + 8u) / 9u, 64, [&] { zxc_block_checksum_kernel(c.data() + 4096, jobs, n_jobs, order, ck_bad, mix_slots); });
            launch(g256, 256, [&] { zxc_checksum_merge_kernel(ck_bad, status, n_jobs); });
        }
    }
    memcpy(order_out, order, (size_t)n_jobs * 4u);
    memcpy(out, o.data() + 4096, out_bytes);
    int pads = 0;
    for (size_t i = 0; i < 4096; i++) {
        if (o[i] != 0xDD) pads |= 1;
        if (o[4096 + out_bytes + i] != 0xDD) pads |= 2;
    }
    return pads;
}
