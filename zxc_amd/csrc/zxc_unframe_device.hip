// zxc_unframe_device.hip — zxc_mi355x_decompress_device: a whole v8 archive in device memory decoded into device memory.
//
// The mirror image of zxc_mi355x_compress_device. zxc_decompress (zxc_host.c) reads the container on the host around the device decoder;
// here the container is parsed, validated and judged on the device, so that an archive already in HBM never crosses the link. The
// container rules are the inline C of zxc_container.h, which the CPU tests run as well. The stream order of one call:
//
//   clear    both job tables = 0 (a job of size 0 is answered with an error status, nothing is read or written for it)
//   head     file header, footer, seek-table probe                                                   -> control word
//   tiles    seek path, per tile of 1024 entries: sum of the entries, plausibility
//   scan     one workgroup: tile offsets; the entries must sum from offset 16 to the EOF block
//   scatter  per tile: block offsets, every thread checks its own block header, jobs, part of the global hash
//   walk     one workgroup: accepts the table's chain, or else follows the header chain from offset 16 like frame_source
//   decode   the existing decode launch over jobs [0, k) into d_dst and over jobs [k, n_jobs) into staged slots
//   tail     staged slot -> d_dst, min(status, capacity left) bytes
//   events   per block found: its own error, the capacity, regularity -> the first one in archive order (64-bit atomic min)
//   result   *d_result = decoded size or the error, written once, after everything above
//
// No workgroup waits for another: every dependency is the stream order between launches, and every stage is predicated on the
// control word. The host knows n_jobs = ceil(dst_capacity / block_size) + 1 and k without reading the archive: an archive with more
// blocks cannot fit, and the one extra job lets a failing block behind a full destination keep its precedence over DST_TOO_SMALL.
// Whether the blocks carry checksum trailers is known on the device only, and the decode launch takes it by value: a call that
// asks for verification decodes two job tables, one with verify_trailer = 1 and one without, and the head stage picks the one
// that gets the jobs (ctl.sel); the other stays empty.
//
// zxc_mi355x_decompress_dict_device is the same call with a dictionary in device memory: the head stage compares the header's
// dictionary id with the word zxc_mi355x_dict_prepare_device wrote, and the decode launches get the dictionary (the plan then is
// the dictionary kernel, one wavefront per block).
#include "zxc_device_util.h"  // the tile passes, the copy, the host-side plumbing; zxc_container.h: the container rules

// ---------------------------------------------------------------- kernels
extern "C" __global__ void __launch_bounds__(64)
zxc_unframe_head_kernel(const uint8_t* __restrict__ src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, uint32_t want_verify,
                        uint32_t n_jobs, zc_ctl_t* __restrict__ ctl, const uint32_t* __restrict__ dict_id) {
    if (threadIdx.x == 0) zc_head_dict(src, src_size, dst_capacity, block_size, (int)want_verify, n_jobs, ctl, dict_id != nullptr, dict_id ? *dict_id : 0u);
}

// Tile t covers entries [t * ZC_TILE_BLOCKS, ...), ZD_PER_THREAD consecutive entries per thread: the tile's sum and whether an entry is
// implausible (such an entry is never added or used as a length). Every tile of the grid writes, also those behind the table.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_unframe_tiles_kernel(const uint8_t* __restrict__ src, const zc_ctl_t* __restrict__ ctl, uint64_t* __restrict__ tile_sum,
                         uint32_t* __restrict__ tile_bad) {
    if (ctl->final || ctl->seek != 1u) return;
    const uint32_t t = threadIdx.x, nb = ctl->nb, file_ck = ctl->file_ck;
    const uint8_t* ent = zc_seek_entries(src, ctl);
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + t * ZD_PER_THREAD;
    uint32_t sum = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        const uint32_t e = zc_rd32(ent + 4ull * b);
        if (zc_seek_entry_ok(e, file_ck)) sum += e;
        else bad = 1u;
    }
    const zd_totals tile = zd_tile_reduce(sum, 0u, bad);
    if (t == 0) {
        tile_sum[blockIdx.x] = tile.sum;
        tile_bad[blockIdx.x] = tile.bad;
    }
}

// One workgroup. tile_sum[t] becomes the archive offset of tile t's first block (exclusive prefix + 16, in place); the table goes on
// (ctl.seek = 2) only when no entry was implausible and the entries sum exactly to the EOF block the head stage found.
extern "C" __global__ void __launch_bounds__(256)
zxc_unframe_scan_kernel(uint64_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_bad, uint32_t n_tiles, zc_ctl_t* __restrict__ ctl) {
    if (ctl->final || ctl->seek != 1u) return;
    const zd_totals all = zd_scan_tiles(  // (behind its barrier every thread has read ctl->seek)
        n_tiles, ZC_FILE_HDR, [=](uint32_t i, uint32_t&, uint32_t& bad) { const uint64_t s = tile_sum[i]; bad |= tile_bad[i]; return s; },
        [=](uint32_t i, uint64_t off) { tile_sum[i] = off; });
    if (threadIdx.x == 0) ctl->seek = (!all.bad && ZC_FILE_HDR + all.sum == ctl->eof_at) ? 2u : 0u;
}

// Per tile: block b's offset is the prefix sum of the entries; its thread checks the block header found there against the entry and
// writes the job. Every offset + entry lies in front of the EOF block (the scan checked the sum), so every read is inside the archive.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_unframe_scatter_kernel(const uint8_t* __restrict__ src, const zc_ctl_t* __restrict__ ctl, const uint64_t* __restrict__ tile_off,
                           uint32_t block_size, uint32_t k_direct, uint32_t n_jobs, zxc_dev_job_t* __restrict__ jobs,
                           uint32_t* __restrict__ tile_hash, uint32_t* __restrict__ tile_bad) {
    if (ctl->final || ctl->seek != 2u) return;
    const uint32_t t = threadIdx.x, nb = ctl->nb, file_ck = ctl->file_ck, verify = ctl->verify;
    const uint8_t* ent = zc_seek_entries(src, ctl);
    zxc_dev_job_t* tab = jobs + (uint64_t)ctl->sel * n_jobs;
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + t * ZD_PER_THREAD;
    uint32_t e[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        e[j] = b0 + j < nb ? zc_rd32(ent + 4ull * (b0 + j)) : 0u;
        sum += e[j];
    }
    uint64_t run = zd_tile_offset(sum, tile_off[blockIdx.x]);
    uint32_t hash = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        if (!zc_seek_block_ok(src, run, e[j], file_ck)) bad = 1u;
        else if (verify) hash ^= zc_hash_term(src, run, e[j], nb, b);
        if (b < n_jobs) tab[b] = zc_job(run, b, e[j], block_size, k_direct);
        run += e[j];
    }
    const zd_totals tile = zd_tile_reduce(0u, hash, bad);
    if (t == 0) {
        tile_hash[blockIdx.x] = tile.hash;
        tile_bad[blockIdx.x] = tile.bad;
    }
}

// One workgroup. If every tile of the scatter pass agreed, the table's chain is the walk's chain and this kernel only records it.
// Otherwise the table is ignored, as zxc_decompress ignores it: the jobs it wrote are cleared and one thread follows the header
// chain, a series of dependent loads (DESIGN.md has its cost per block).
extern "C" __global__ void __launch_bounds__(256)
zxc_unframe_walk_kernel(const uint8_t* __restrict__ src, uint64_t src_size, uint32_t block_size, uint32_t k_direct, uint32_t n_jobs,
                        const uint32_t* __restrict__ tile_hash, const uint32_t* __restrict__ tile_bad, zxc_dev_job_t* __restrict__ jobs,
                        zc_ctl_t* __restrict__ ctl) {
    if (ctl->final) return;
    const uint32_t t = threadIdx.x;
    zxc_dev_job_t* tab = jobs + (uint64_t)ctl->sel * n_jobs;
    if (ctl->seek == 2u) {
        const uint32_t tiles = (ctl->nb + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS;  // (nb <= n_jobs: inside the grid of the scatter pass)
        uint32_t hash = 0, bad = 0;
        for (uint32_t i = t; i < tiles; i += 256u) { hash ^= tile_hash[i]; bad |= tile_bad[i]; }
        const zd_totals all = zd_tile_reduce(0u, hash, bad);
        if (!all.bad) {
            if (t == 0) zc_chain_from_table(ctl, all.hash);
            return;
        }
        uint64_t* words = (uint64_t*)tab;  // 24-byte jobs, 8-byte aligned
        for (uint64_t i = t; i < 3ull * n_jobs; i += 256u) words[i] = 0;
        __syncthreads();
    }
    if (t == 0) zc_walk(src, src_size, block_size, k_direct, n_jobs, ctl, tab);
}

// Staged block k_direct + blockIdx.x -> its place in the destination, as many bytes as it decoded to and the capacity still holds.
extern "C" __global__ void __launch_bounds__(256)
zxc_unframe_tail_kernel(const uint8_t* __restrict__ stage, const int32_t* __restrict__ status, const zc_ctl_t* __restrict__ ctl,
                        uint32_t block_size, uint32_t k_direct, uint32_t n_jobs, uint8_t* __restrict__ dst, uint64_t dst_capacity) {
    const uint32_t i = k_direct + blockIdx.x;
    if (ctl->final || i >= n_jobs) return;
    const uint32_t n = zc_tail_bytes(i, status[(uint64_t)ctl->sel * n_jobs + i], block_size, dst_capacity);
    copy_bytes(dst + (uint64_t)i * block_size, stage + (uint64_t)blockIdx.x * block_size, n, threadIdx.x, 256u);
}

// The first block, in archive order, whose status ends the call: zc_block_event is local to a block as long as no earlier block has
// an event, and the minimum of (index, code) is exactly that first one.
extern "C" __global__ void __launch_bounds__(256)
zxc_unframe_events_kernel(const int32_t* __restrict__ status, uint32_t block_size, uint32_t n_jobs, uint64_t dst_capacity,
                          zc_ctl_t* __restrict__ ctl) {
    if (ctl->final) return;
    const uint32_t found = ctl->found, done = ctl->done;
    const int32_t* st = status + (uint64_t)ctl->sel * n_jobs;
    unsigned long long key = ZC_NO_EVENT;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < found; i += (uint64_t)gridDim.x * 256u) {
        const int32_t ev = zc_block_event((uint32_t)i, st[i], found, done, block_size, dst_capacity);
        if (ev != 0) { key = zc_event_key((uint32_t)i, ev); break; }  // (a thread's later blocks have larger indices)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63u) == 0 && key != ZC_NO_EVENT) atomicMin(&ctl->event, key);
}

extern "C" __global__ void __launch_bounds__(64)
zxc_unframe_result_kernel(const zc_ctl_t* __restrict__ ctl, const int32_t* __restrict__ status, uint32_t block_size, uint32_t n_jobs,
                          int64_t* __restrict__ result) {
    if (threadIdx.x != 0) return;
    const int32_t last = (!ctl->final && ctl->found) ? status[(uint64_t)ctl->sel * n_jobs + ctl->found - 1u] : 0;
    *result = zc_verdict(ctl, last, block_size);
}

// ---------------------------------------------------------------- host side
extern "C" {

uint64_t zxc_mi355x_decompress_device_work_size(uint64_t src_size, uint64_t dst_capacity, uint32_t block_size) {
    zc_shape_t s;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER || zc_shape(dst_capacity, block_size, &s) != 0) return 0u;
    return s.bytes;
}

// Both calls. dict == NULL: the call that takes no dictionary.
static int unframe_call(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                        const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result,
                        void* stream) {
    if (!d_src || !d_work || !d_result || (!d_dst && dst_capacity > 0)) return ZXC_ERROR_NULL_INPUT;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER) return ZXC_ERROR_SRC_TOO_SMALL;
    zc_shape_t s;
    if (zc_shape(dst_capacity, block_size, &s) != 0) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if ((uintptr_t)d_dst & 15u) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (work_size < s.bytes) return ZXC_ERROR_MEMORY;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const uint32_t want_verify = (opts && opts->checksum_enabled) ? 1u : 0u, tables = 1u + want_verify;
    uint8_t* base = zd_work_base(d_work);
    const zd_cwork_t w = zd_cwork(base, s);
    const zd_dict_t dc = zd_dict_of(dict);
    uint8_t* stage = base + s.o_stage;

    const int crc = zd_container_stages(w, (const uint8_t*)d_src, src_size, dst_capacity, block_size, want_verify, s.k_direct, dc.id, st);
    if (crc != ZXC_OK) return crc;
    if (dst_capacity > 0) {
        // Not zd_decode_tables: per table the direct launch, then the staged one. Two calls of the helper would enqueue both
        // tables' direct launches in front of the staged ones, another stream order than this call has always had.
        for (uint32_t tb = 0; tb < tables; tb++) {
            const zxc_dev_job_t* tab = w.jobs + (uint64_t)tb * s.n_jobs;
            int32_t* tst = w.status + (uint64_t)tb * s.n_jobs;
            int rc = zxc_hip_decode_blocks(d_src, tab, s.k_direct, d_dst, tst, block_size, (int)tb, dc.content, dc.size, dc.huf, 0u, stream);
            if (rc == ZXC_OK)
                rc = zxc_hip_decode_blocks(d_src, tab + s.k_direct, s.n_jobs - s.k_direct, stage, tst + s.k_direct, block_size, (int)tb, dc.content,
                                           dc.size, dc.huf, 0u, stream);
            if (rc != ZXC_OK) return rc;
        }
        hipLaunchKernelGGL(zxc_unframe_tail_kernel, dim3(ZC_STAGED_MAX), dim3(256), 0, st, (const uint8_t*)stage, (const int32_t*)w.status,
                           (const zc_ctl_t*)w.ctl, block_size, s.k_direct, s.n_jobs, (uint8_t*)d_dst, dst_capacity);
    }
    return zd_verdict_stages(w, block_size, dst_capacity, d_result, st);  // (its first launch check covers the tail stage)
}

int zxc_mi355x_decompress_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                 const zxc_decompress_opts_t* opts, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    return unframe_call(d_src, src_size, d_dst, dst_capacity, block_size, opts, NULL, d_work, work_size, d_result, stream);
}

int zxc_mi355x_decompress_dict_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                      const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size,
                                      int64_t* d_result, void* stream) {
    return unframe_call(d_src, src_size, d_dst, dst_capacity, block_size, opts, dict, d_work, work_size, d_result, stream);
}

int zxc_mi355x_frame_info_device(const void* d_src, uint64_t src_size, uint32_t* block_size, uint64_t* decompressed_size, int* has_checksum,
                                 void* stream) {
    if (!d_src) return ZXC_ERROR_NULL_INPUT;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER) return ZXC_ERROR_SRC_TOO_SMALL;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t h[ZC_FILE_HDR + ZC_FOOTER];
    if (hipMemcpyAsync(h, d_src, ZC_FILE_HDR, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h + ZC_FILE_HDR, (const uint8_t*)d_src + src_size - ZC_FOOTER, ZC_FOOTER, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return ZXC_ERROR_GPU_UNAVAILABLE;
    uint32_t lg = 0, ck = 0, dict_id = 0;
    const int rc = zc_file_header(h, &lg, &ck, &dict_id);
    if (rc != ZXC_OK) return rc;
    // the footer's size, when it is plausible for the archive's bytes (zxc_get_decompressed_size: >= 8 compressed bytes per block)
    const uint64_t total = zc_rd64(h + ZC_FILE_HDR), bs = 1ull << lg, need = total / bs + (total % bs != 0);
    if (block_size) *block_size = (uint32_t)bs;
    if (decompressed_size) *decompressed_size = need <= src_size / ZC_BLK_HDR ? total : 0u;
    if (has_checksum) *has_checksum = (int)ck;
    return ZXC_OK;
}

}  // extern "C"
