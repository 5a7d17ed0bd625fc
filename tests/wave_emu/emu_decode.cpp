// emu_decode.cpp — the decode kernels of zxc_amd/csrc compiled for the CPU wave emulator and driven
// block by block (one emulated wavefront per block, like the real launch). Test infrastructure.
#include <functional>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "zxc_decode_kernel.hip"   // found via -I zxc_amd/csrc; <hip/hip_runtime.h> resolves to tests/wave_emu/hip/

namespace emu { void run_wave(const std::function<void()>& body, unsigned block, unsigned grid, int n_lanes); }
extern char __start_emu_lds[], __stop_emu_lds[];

static uint32_t emu_last_deferred = 0, emu_last_pre = 0, emu_last_secs[3] = {0, 0, 0};
static size_t emu_pscratch_bytes = (size_t)8 << 20;  // scratch of the workgroup section decoder (0: every coded block goes to the full kernel)
extern "C" __attribute__((visibility("default"))) uint32_t emu_last_deferred_count(void) { return emu_last_deferred; }
extern "C" __attribute__((visibility("default"))) uint32_t emu_last_pre_count(void) { return emu_last_pre; }
extern "C" __attribute__((visibility("default"))) void emu_set_pscratch_bytes(size_t n) { emu_pscratch_bytes = n; }
static size_t emu_rscratch_bytes = (size_t)4 << 20;  // scratch for the expanded literals of LEAN_RLE blocks (0: they go to the full kernel)
extern "C" __attribute__((visibility("default"))) void emu_set_rscratch_bytes(size_t n) { emu_rscratch_bytes = n; }
extern "C" __attribute__((visibility("default"))) uint32_t emu_last_section_count(int size_class) { return emu_last_secs[size_class]; }

// path markers (ZXC_PATH, zxc_lds.h): lanes that passed each marker since the last reset
extern "C" __attribute__((visibility("default"))) void emu_path_reset(void) { memset(emu::path_count, 0, sizeof(emu::path_count)); }
extern "C" __attribute__((visibility("default"))) uint32_t emu_path_read(uint64_t* out, uint32_t n) {
    for (uint32_t i = 0; i < n && i < (uint32_t)ZXC_PATH_COUNT; i++) out[i] = emu::path_count[i];
    return (uint32_t)ZXC_PATH_COUNT;
}

// per-block checksums: 1 = by zxc_block_checksum_kernel beside the decode, merged into the statuses; 0 = inside the decode kernels
static int emu_ck_apart = 1;
extern "C" __attribute__((visibility("default"))) void emu_set_ck_apart(int on) { emu_ck_apart = on; }

// the strict per-block capacity of zxc_decompress_block_safe (the kernels' cap_override argument; 0 = block_size + 2112)
static uint32_t emu_cap_override = 0;
extern "C" __attribute__((visibility("default"))) void emu_set_cap_override(uint32_t cap) { emu_cap_override = cap; }

// the product's plan table and launch-order buffer layout (zxc_dev.h), for tests/test_wave_emu_plans.py
extern "C" __attribute__((visibility("default"))) void emu_decode_plan_choose(const zxc_dev_plan_in_t* in, zxc_dev_plan_t* out) { *out = zxc_dev_plan_choose(in); }
extern "C" __attribute__((visibility("default"))) void emu_ord_layout(uint32_t n_jobs, zxc_dev_ord_layout_t* out) { *out = zxc_dev_ord_layout(n_jobs); }

extern "C" __attribute__((visibility("default")))
int emu_decode_blocks(const uint8_t* comp, size_t comp_bytes, const zxc_dev_job_t* jobs, uint32_t n_jobs, uint8_t* out,
                      size_t out_bytes, int32_t* status, uint32_t block_size, int verify_trailer, const uint8_t* dict,
                      uint32_t dict_size, const uint8_t* dict_huf) {
    // padded private copies: the kernels read (never use) a few bytes past the ends, as they may in device buffers. The output
    // starts as the caller's buffer between two 4 KiB pads of 0xDD; the return value tells whether a pad changed (bit 0: the one
    // in front, bit 1: the one behind), so a caller's own guard bytes and these pads together catch every stray store.
    std::vector<uint8_t> c(comp_bytes + 8192, 0xEE), o(out_bytes + 8192, 0xDD);
    memcpy(c.data() + 4096, comp, comp_bytes);
    memcpy(o.data() + 4096, out, out_bytes);
    const uint32_t stride = ZXC_DEV_SLOT_STRIDE(block_size);
    const uint32_t n_slots = 4;
    std::vector<uint8_t> scratch((size_t)n_slots * stride + 4096, 0xCC);
    std::vector<uint32_t> busy(8192, 0);
    std::vector<uint8_t> dct;
    const uint8_t* dptr = nullptr;
    if (dict && dict_size) { dct.assign(dict_size + 8192, 0xBB); memcpy(dct.data() + 4096, dict, dict_size); dptr = dct.data() + 4096; }
    // The plan from the knobs, through the product's chooser as for a first launch (the knobs' scratch sizes); emu_set_ck_apart(1)
    // also puts the checksums apart beside PRE blocks, which the product's chooser never picks.
    zxc_dev_plan_in_t in = {(uint32_t)(dptr || dict_huf), emu_cap_override, n_jobs, ~0u, 0u, (uint32_t)(verify_trailer != 0), block_size, 1u, 1u};
    in.ck_inline = !emu_ck_apart, in.pscratch_failed = !emu_pscratch_bytes;
    zxc_dev_plan_t p = zxc_dev_plan_choose(&in);
    if (p.kind >= ZXC_DEV_PLAN_TWO_PASS && verify_trailer && emu_ck_apart) p.ck_apart = 1u, p.trailer_bytes = 4u | ZXC_DEV_TRAILER_ELSEWHERE;
    const uint32_t tb = p.trailer_bytes, g256 = (n_jobs + 255u) / 256u;
    auto launch = [&](unsigned grid, int threads, const std::function<void()>& k) {
        for (unsigned g = 0; g < grid; g++) {
            memset(__start_emu_lds, 0xA5, (size_t)(__stop_emu_lds - __start_emu_lds));  // LDS is not zero at launch
            emu::run_wave(k, g, grid, threads);
        }
    };
    if (p.kind < ZXC_DEV_PLAN_TWO_PASS) {  // dictionary kernel, or the full kernel alone under the strict capacity (zxc_hip_shim.hip)
        launch(n_jobs, 64, [&] {
            if (p.kind == ZXC_DEV_PLAN_DICT)
                zxc_decode_blocks_dict_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, tb, scratch.data(), stride,
                                              0u, busy.data(), n_slots, nullptr, emu_cap_override, dptr, dict_size, dict_huf);
            else
                zxc_decode_blocks_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, tb, scratch.data(), stride, 0u,
                                         busy.data(), n_slots, nullptr, emu_cap_override, nullptr);
        });
    } else {
        // the two-pass launch of zxc_hip_shim.hip, kernel by kernel, over one launch-order buffer carved as on the device and
        // poisoned except where the shim zeroes it: launch-order pass, section kernels, lean kernel, its second entry, full kernel
        const zxc_dev_ord_layout_t at = zxc_dev_ord_layout(n_jobs);
        std::vector<uint32_t> buf(at.words, 0xA3A3A3A3u);
        memset(buf.data(), 0, 130u * 4u);
        memset(buf.data() + at.ctl, 0, ZXC_DEV_CTL_WORDS * 4u);
        uint32_t *order = buf.data() + at.order, *list = buf.data() + at.list, *ctl = buf.data() + at.ctl, *pre_entries = buf.data() + at.pre_ent;
        zxc_dev_sec_t* secs = (zxc_dev_sec_t*)(buf.data() + at.secs);
        zxc_dev_pre_t* pre = (zxc_dev_pre_t*)(buf.data() + at.pre);
        uint8_t* ck_bad = (uint8_t*)(buf.data() + at.ck_bad);
        std::vector<uint8_t> pscratch(emu_pscratch_bytes + 4096, 0xC3);
        std::vector<uint8_t> rscratch(emu_rscratch_bytes + 4096, 0xC7);  // expanded literals of the LEAN_RLE blocks
        launch(g256, 256, [&] { zxc_order_hist_kernel(c.data() + 4096, jobs, n_jobs, block_size, buf.data()); });
        launch(g256, 256, [&] {
            zxc_order_scatter_kernel(c.data() + 4096, jobs, n_jobs, block_size, buf.data(), order, list, tb & ~ZXC_DEV_TRAILER_ELSEWHERE, pre, ctl,
                                     pre_entries, secs, (uint32_t)(emu_pscratch_bytes >> 4), emu_cap_override ? emu_cap_override : block_size + 2112u,
                                     (uint32_t)(emu_rscratch_bytes >> 4));
        });
        emu_last_pre = ctl[ZXC_DEV_CTL_PRE];
        uint32_t* sec_hdr = ctl + ZXC_DEV_CTL_SEC;
        for (int k = 0; k < 3; k++) emu_last_secs[k] = sec_hdr[2 * k];
        if (sec_hdr[0]) launch(2, 128, [&] { zxc_pivco_sections_small_kernel(c.data() + 4096, secs, sec_hdr, pre, pscratch.data()); });
        if (sec_hdr[2]) launch(2, 256, [&] { zxc_pivco_sections_medium_kernel(c.data() + 4096, secs + 2u * (size_t)n_jobs, sec_hdr + 2, pre, pscratch.data()); });
        if (sec_hdr[4]) launch(2, 512, [&] { zxc_pivco_sections_large_kernel(c.data() + 4096, secs + 4u * (size_t)n_jobs, sec_hdr + 4, pre, pscratch.data()); });
        if (ctl[ZXC_DEV_CTL_RLE_LIST])
            launch(3u, 64, [&] { zxc_rle_expand_kernel(c.data() + 4096, jobs, pre, rscratch.data(), ctl + ZXC_DEV_CTL_RLE_LIST, pre_entries + n_jobs - 1u); });
        launch(n_jobs, 64, [&] {
            zxc_decode_blocks_lean_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, order, emu_cap_override, tb, pre, rscratch.data());
        });
        if (ctl[ZXC_DEV_CTL_PRE]) launch(n_jobs, 64, [&] {
            zxc_decode_blocks_lean_pre_kernel(c.data() + 4096, jobs, o.data() + 4096, status, block_size, emu_cap_override, tb, pre, pscratch.data(),
                                              ctl + ZXC_DEV_CTL_PRE, pre_entries);
        });
        emu_last_deferred = list[0];
        launch(n_jobs < 3u ? n_jobs : 3u, 64, [&] {
            zxc_decode_blocks_kernel(c.data() + 4096, jobs, n_jobs, o.data() + 4096, status, block_size, tb, scratch.data(), stride, 0u,
                                     busy.data(), n_slots, order, emu_cap_override, list);
        });
        if (p.ck_apart) {
            launch((n_jobs + 8u) / 9u, 64, [&] { zxc_block_checksum_kernel(c.data() + 4096, jobs, n_jobs, order, ck_bad); });
            launch(g256, 256, [&] { zxc_checksum_merge_kernel(ck_bad, status, n_jobs); });
        }
    }
    memcpy(out, o.data() + 4096, out_bytes);
    int pads = 0;
    for (size_t i = 0; i < 4096; i++) {
        if (o[i] != 0xDD) pads |= 1;
        if (o[4096 + out_bytes + i] != 0xDD) pads |= 2;
    }
    return pads;
}
