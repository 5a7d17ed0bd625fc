"""zxc_mi355x_decompress_device without a GPU: the three symbols, every synchronous argument check in its stated order (the device
pointers below are never dereferenced), the work-size arithmetic, and the container rules the kernels run
(zxc_amd/csrc/zxc_container.h), compiled here with the host C compiler and driven over every golden archive: the seek-table path
and the walk give the job table of Seekable.plan() / of a header walk restated below, and the verdict fed with the oracle
decoder's block statuses gives what the oracle's whole-frame decoder (the CPU restatement of zxc_decompress) returns."""
import ctypes as C
import os

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from devtest import ERR
from zxc_amd.api import _DecompressOpts

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x40000
JOB_BYTES = 24
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
# archives written with a dictionary: the call takes none, so the device's answer is the header's dictionary id -> DICT_REQUIRED
# (what zxc_decompress returns without a dictionary); with opts->dict the call is refused with GPU_UNSUPPORTED before any launch
DICT_ARCHIVES = {"conformance/valid/dict_http.zxc", "conformance/valid/dict_seekable_l7.zxc", "conformance/invalid/dict_required.zxc",
                 "format/09_block_dict.zxc", "format/12_glo_huffman_dict.zxc"}


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_decompress_device"), "libzxc_mi355x.so does not export zxc_mi355x_decompress_device"
    return L


def _ws(L, n, cap, bs):
    return int(L.zxc_mi355x_decompress_device_work_size(n, cap, bs))


def _call(L, n=1000, cap=1 << 20, bs=65536, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES, opts=None):
    ws = max(_ws(L, n, cap, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_device(src, n, dst, cap, bs, C.byref(opts) if opts is not None else None, work, ws, res, None)


def _dict_opts():
    o = _DecompressOpts()
    o.dict, o.dict_size = FAKE_SRC, 100
    return o


def test_symbols_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_decompress_device", "zxc_mi355x_decompress_device_work_size", "zxc_mi355x_frame_info_device"):
        assert hasattr(L, sym), sym
    for name in ("decompress_device", "decompress_device_work_size", "frame_info_device"):
        assert hasattr(product, name), name


def test_each_synchronous_error(L):
    assert _call(L, src=None) == ERR["NULL_INPUT"]
    assert _call(L, work=None) == ERR["NULL_INPUT"]
    assert _call(L, res=None) == ERR["NULL_INPUT"]
    assert _call(L, dst=None) == ERR["NULL_INPUT"]
    for n in (0, 1, 27):
        assert _call(L, n=n) == ERR["SRC_TOO_SMALL"], n
    for bad in (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22):
        assert _call(L, bs=bad, ws=1 << 30) == ERR["BAD_BLOCK_SIZE"], bad
    assert _call(L, opts=_dict_opts()) == ERR["GPU_UNSUPPORTED"]
    for off in (1, 4, 8, 15):
        assert _call(L, dst=FAKE_DST + off) == ERR["GPU_UNSUPPORTED"], off
    for n, cap, bs in ((28, 1, 4096), (1000, 1 << 20, 65536), (1 << 24, 1 << 30, 4096)):
        assert _call(L, n=n, cap=cap, bs=bs, ws=_ws(L, n, cap, bs) - 1) == ERR["MEMORY"], (n, cap, bs)


def test_synchronous_errors_come_in_the_stated_order(L):
    """each call breaks one rule and every later one; the earliest is reported"""
    late = dict(opts=_dict_opts(), ws=0)
    assert _call(L, src=None, n=5, bs=5000, dst=FAKE_DST + 1, **late) == ERR["NULL_INPUT"]
    assert _call(L, dst=None, n=5, bs=5000, **late) == ERR["NULL_INPUT"]
    assert _call(L, n=5, bs=5000, dst=FAKE_DST + 1, **late) == ERR["SRC_TOO_SMALL"]
    assert _call(L, bs=5000, dst=FAKE_DST + 1, **late) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, dst=FAKE_DST + 1, **late) == ERR["GPU_UNSUPPORTED"]  # the dictionary
    assert _call(L, dst=FAKE_DST + 1, ws=0) == ERR["GPU_UNSUPPORTED"]    # the alignment
    assert _call(L, ws=0) == ERR["MEMORY"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _call(L) == ERR["GPU_UNAVAILABLE"]
        assert _call(L, n=28, cap=0, dst=None) == ERR["GPU_UNAVAILABLE"]  # the empty-frame probe: NULL d_dst is fine
        assert _call(L, opts=_DecompressOpts(checksum_enabled=1), bs=4096) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.frame_info_device(FAKE_SRC, 100)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_work_size(L):
    for bs in BLOCK_SIZES:
        prev = 0
        for cap in (0, 1, 31, 32, 33, bs - 1, bs, bs + 1, bs + 32, 2 * bs + 31, 5 * bs, 1023 * bs + 7, 1024 * bs, 1025 * bs, 1 << 32, 1 << 36):
            w = _ws(L, 1 << 20, cap, bs)
            n_max = -(-cap // bs)
            assert w > 0 and w >= prev, (bs, cap, w, prev)
            assert w >= n_max * JOB_BYTES + 2 * bs, (bs, cap, w)
            prev = w
        assert _ws(L, 28, 10 * bs, bs) == _ws(L, 1 << 30, 10 * bs, bs)  # the capacity sizes the call, not the archive
    for bad in (0, 1000, 4095, 5000, 3 << 12, 1 << 22):
        assert _ws(L, 1 << 20, 1 << 20, bad) == 0, bad
    assert _ws(L, 27, 1 << 20, 65536) == 0
    assert _ws(L, 1 << 20, (1 << 31) * 4096, 4096) == 0  # more blocks than a launch counts


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.decompress_device(FAKE_SRC, 1000, FAKE_DST, 1 << 20, 65536, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_device(FAKE_SRC, 1000, 0, 1 << 20, 65536, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_device(FAKE_SRC, 1000, FAKE_DST, 1 << 20, 5000, FAKE_WORK, 1 << 30, FAKE_RES, checksum=True)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.frame_info_device(0, 1000)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.frame_info_device(FAKE_SRC, 27)
    assert e.value.code == ERR["SRC_TOO_SMALL"]
    assert product.decompress_device_work_size(1000, 1 << 20, 5000) == 0
    assert product.decompress_device_work_size(1000, 1 << 20, 65536) > 0


# ---------------------------------------------------------------- the shared container header, run on the CPU
class Ctl(C.Structure):  # zc_ctl_t
    _fields_ = [("head_result", C.c_int64), ("total", C.c_uint64), ("eof_at", C.c_uint64), ("event", C.c_uint64), ("final", C.c_uint32),
                ("file_ck", C.c_uint32), ("verify", C.c_uint32), ("sel", C.c_uint32), ("stored_hash", C.c_uint32), ("nb", C.c_uint32),
                ("seek", C.c_uint32), ("found", C.c_uint32), ("done", C.c_uint32), ("saw_eof", C.c_uint32), ("tail_err", C.c_int32),
                ("ghash", C.c_uint32)]


class Shape(C.Structure):  # zc_shape_t
    _fields_ = [("n_jobs", C.c_uint32), ("k_direct", C.c_uint32), ("n_tiles", C.c_uint32)] + \
               [(n, C.c_uint64) for n in ("o_tile_sum", "o_tile_hash", "o_tile_bad", "o_jobs", "o_status", "o_stage", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "container", "container/container_shim.c")
    S.t_ctl_size.restype = S.t_shape_size.restype = C.c_size_t
    assert S.t_ctl_size() == C.sizeof(Ctl) and S.t_shape_size() == C.sizeof(Shape)
    S.t_shape.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(Shape)]
    S.t_plan.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(Ctl), C.c_void_p]
    S.t_verdict.restype = C.c_int64
    S.t_verdict.argtypes = [C.POINTER(Ctl), C.c_void_p, C.c_uint32, C.c_uint64]
    S.t_tail_bytes.restype = C.c_uint32
    S.t_tail_bytes.argtypes = [C.c_uint32, C.c_int32, C.c_uint32, C.c_uint64]
    return S


def _golden_archives():
    out = []
    for d in ("conformance/valid", "conformance/invalid", "format"):
        out += [f"{d}/{f}" for f in sorted(os.listdir(os.path.join(GOLDEN, d))) if f.endswith(".zxc")]
    return out


def _hash8(hdr7: bytes) -> int:
    M = (1 << 64) - 1
    h = int.from_bytes(hdr7 + b"\0", "little") ^ 0x9E3779B97F4A7C15
    h ^= (h << 13) & M
    h ^= h >> 7
    h ^= (h << 17) & M
    return ((h >> 32) ^ h) & 0xFF


def _host_walk(comp: bytes, bs: int, file_ck: int, limit: int):
    """frame_source of zxc_host.c, restated: -> [(comp_off, comp_size)] of the blocks a header walk finds, at most `limit`"""
    ip, jobs = 16, []
    while len(jobs) < limit and ip < len(comp):
        rem = len(comp) - ip
        if rem < 8 or comp[ip + 7] != _hash8(comp[ip: ip + 7]) or comp[ip] == 255:
            break
        phys = 8 + int.from_bytes(comp[ip + 3: ip + 7], "little") + 4 * file_ck
        jobs.append((ip, min(phys, rem)))
        if phys >= rem:
            break
        ip += phys
    return jobs


def _plan(shim, product, comp, cap, bs, checksum, use_table, k=None):
    sh = Shape()
    assert shim.t_shape(cap, bs, C.byref(sh)) == 0
    ctl = Ctl()
    jobs = np.zeros(sh.n_jobs, dtype=product.JOB_DTYPE)
    used = shim.t_plan(comp, len(comp), cap, bs, int(checksum), int(use_table), sh.n_jobs, sh.n_jobs if k is None else k, C.byref(ctl),
                       jobs.ctypes.data)
    return used, ctl, jobs, sh


def _verdict(shim, oracle, comp, ctl, jobs, bs, cap):
    st = np.zeros(max(ctl.found, 1), dtype=np.int32)
    for i in range(ctl.found):
        off, n = int(jobs["comp_off"][i]), int(jobs["comp_size"][i])
        st[i], _ = oracle.decode_block(comp[off: off + n], bs, checksum=bool(ctl.verify))
    return int(shim.t_verdict(C.byref(ctl), st.ctypes.data, bs, cap)), st


@pytest.mark.parametrize("rel", _golden_archives())
def test_container_rules_on_golden_archive(shim, product, oracle, rel):
    comp = open(os.path.join(GOLDEN, rel), "rb").read()
    lg = comp[5] if len(comp) > 5 else 0
    bs = 1 << lg if 12 <= lg <= 21 else 65536
    if len(comp) < 28:  # refused before any launch, with the code the whole-frame decoder gives
        want, _ = oracle.decompress(comp, 1 << 20)
        got = product.lib().zxc_mi355x_decompress_device(C.c_void_p(FAKE_SRC), C.c_uint64(len(comp)), C.c_void_p(FAKE_DST), C.c_uint64(1 << 20),
                                                         C.c_uint32(bs), None, C.c_void_p(FAKE_WORK), C.c_uint64(1 << 30), C.c_void_p(FAKE_RES), None)
        assert got == want == ERR["SRC_TOO_SMALL"], rel
        return
    size = product.get_decompressed_size(comp)
    exp = os.path.join(GOLDEN, rel[:-4] + ".expected")
    if os.path.exists(exp):
        size = os.path.getsize(exp)
    for checksum in (False, True):
        for cap in sorted({size, size + 1000, max(size - 1, 0), 0, 1 << 20}):
            what = (rel, checksum, cap)
            want, _ = oracle.decompress(comp, cap, checksum=checksum)
            used, ctl, jobs, sh = _plan(shim, product, comp, cap, bs, checksum, True)
            _, ctl_w, jobs_w, _ = _plan(shim, product, comp, cap, bs, checksum, False)
            if rel in DICT_ARCHIVES and cap > 0:
                assert ctl.final and ctl.head_result == ERR["DICT_REQUIRED"] == want, what
            # the two paths agree on everything the later stages read
            assert (jobs == jobs_w).all(), what
            for f in ("final", "head_result", "found", "done", "saw_eof", "tail_err", "ghash", "verify", "sel"):
                assert getattr(ctl, f) == getattr(ctl_w, f), (what, f)
            if ctl.final:
                assert ctl.found == 0 and not jobs["comp_size"].any(), what  # no block is decoded
            else:
                ref_jobs = _host_walk(comp, bs, ctl.file_ck, sh.n_jobs)
                assert ctl.found == len(ref_jobs), what
                for i, (off, n) in enumerate(ref_jobs):
                    assert (int(jobs["comp_off"][i]), int(jobs["comp_size"][i]), int(jobs["out_off"][i]), int(jobs["out_len"][i])) == \
                        (off, n, i * bs, bs), (what, i)
                assert not jobs["comp_size"][ctl.found:].any(), what
            got, st = _verdict(shim, oracle, comp, ctl, jobs, bs, cap)
            assert got == want, (what, got, want, list(st[:8]))
            got_w, _ = _verdict(shim, oracle, comp, ctl_w, jobs_w, bs, cap)
            assert got_w == want, what
            if used:  # a table that was used is the host's table
                s = product.Seekable(comp)
                try:
                    assert s.num_blocks == ctl.found, what
                    plan = s.plan()
                finally:
                    s.close()
                for f in ("comp_off", "out_off", "comp_size"):
                    assert (plan[f] == jobs[f][: ctl.found]).all(), (what, f)
                assert (plan["out_len"][:-1] == bs).all() and plan["out_len"][-1] == size - (ctl.found - 1) * bs, what


def test_seek_table_path_is_taken_and_survives_nothing_wrong(shim, product):
    """the seekable goldens use their table when the capacity holds the archive; a table with one entry changed, one with a
    broken header hash and one whose entries miss the EOF block are ignored, and the walk gives the same jobs"""
    for rel in ("conformance/valid/seekable_4blocks.zxc", "conformance/valid/seekable_checksum.zxc", "format/08_seekable_table.zxc"):
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        bs, size = 1 << comp[5], product.get_decompressed_size(comp)
        used, ctl, jobs, _ = _plan(shim, product, comp, size, bs, True, True)
        assert used == 1 and ctl.seek == 3 and ctl.found == ctl.nb >= 1, rel
        first_entry = len(comp) - 12 - 4 * ctl.nb
        for at, delta in ((first_entry, 1), (first_entry + 4 * (ctl.nb - 1), 4), (first_entry - 1, 1), (first_entry - 5, 4)):
            bad = bytearray(comp)
            bad[at] = (bad[at] + delta) & 0xFF
            used_b, ctl_b, jobs_b, _ = _plan(shim, product, bytes(bad), size, bs, True, True)
            assert used_b == 0 and ctl_b.found == ctl.found and (jobs_b == jobs).all() and ctl_b.ghash == ctl.ghash, (rel, at)
        # a capacity that cannot hold the archive's blocks sends it to the walk, which stops at the job limit
        if ctl.nb >= 3:
            used_c, ctl_c, jobs_c, sh = _plan(shim, product, comp, bs, bs, True, True)
            assert used_c == 0 and sh.n_jobs == 2 and ctl_c.found == 2 and ctl_c.done == 0, rel


def test_the_k_split_and_the_tail_copy(shim, product):
    comp = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    bs, size = 1 << comp[5], product.get_decompressed_size(comp)
    for cap in (size, size + 31, size + 32, 4 * bs, 4 * bs + 32, 5 * bs + 40):
        sh = Shape()
        assert shim.t_shape(cap, bs, C.byref(sh)) == 0
        n_max = -(-cap // bs)
        assert sh.n_jobs == n_max + 1 and sh.k_direct == min((cap - 32) // bs, sh.n_jobs) and 1 <= sh.n_jobs - sh.k_direct <= 3, cap
        for i in range(sh.n_jobs):  # a direct slot and the 32 bytes the decoders may store behind it lie inside the capacity
            assert (i < sh.k_direct) == ((i + 1) * bs + 32 <= cap), (cap, i)
        for use_table in (0, 1):
            _, ctl, jobs, _ = _plan(shim, product, comp, cap, bs, False, use_table, k=sh.k_direct)
            for i in range(ctl.found):
                assert int(jobs["out_off"][i]) == (i if i < sh.k_direct else i - sh.k_direct) * bs, (cap, i)
    assert shim.t_tail_bytes(3, 100, 4096, 3 * 4096 + 100) == 100
    assert shim.t_tail_bytes(3, 100, 4096, 3 * 4096 + 99) == 99
    assert shim.t_tail_bytes(3, 5000, 4096, 1 << 20) == 4096  # never more than the slot holds
    assert shim.t_tail_bytes(3, 100, 4096, 3 * 4096) == 0 and shim.t_tail_bytes(3, -7, 4096, 1 << 20) == 0
    assert shim.t_tail_bytes(0, 4096, 4096, 31) == 31
