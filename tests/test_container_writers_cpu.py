"""The writers of zxc_amd/csrc/zxc_container.h against archives the reference wrote: what the readers parse out of a file header, an
EOF block, a seek-table header and a footer, the writers turn back into exactly the bytes that were there. The host API and the
device-to-device compress calls write the container through these functions alone. No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

DIRS = ("conformance/valid", "format", "synth")
BLK_SEK, BLK_EOF = 254, 255


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("container_writers") / "libcontainer_shim.so")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "container", "container_shim.c")], check=True)
    S = C.CDLL(so)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    S.t_file_header.argtypes = [C.c_char_p, u32p, u32p, u32p]
    S.t_put_file_header.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32]
    S.t_put_blk_hdr.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
    S.t_put_footer.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32]
    S.t_block_size_lg.restype = C.c_uint32
    S.t_block_size_lg.argtypes = [C.c_uint64]
    S.t_hash_fold.restype = C.c_uint32
    S.t_hash_fold.argtypes = [C.c_uint32, C.c_uint32]
    S.t_seek_tail.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, u64p]
    S.t_chain_eof.restype = C.c_int64
    S.t_chain_eof.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32]
    return S


def _archives():
    out = []
    for d in DIRS:
        for base, _, files in os.walk(os.path.join(GOLDEN, d)):
            out += [os.path.join(base, f) for f in files if f.endswith(".zxc")]
    return sorted(out)


def test_writers_rebuild_what_the_reference_wrote(shim):
    paths = _archives()
    visited = with_ck = with_dict = with_eof = with_seek = 0
    for path in paths:
        comp = open(path, "rb").read()
        assert len(comp) >= 28, path
        # file header: parse, write again
        lg, ck, did = C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert shim.t_file_header(comp[:16], C.byref(lg), C.byref(ck), C.byref(did)) == 0, path
        assert shim.t_block_size_lg(1 << lg.value) == lg.value, path
        hdr = C.create_string_buffer(16)
        shim.t_put_file_header(hdr, lg.value, ck.value, int(did.value != 0), did.value)
        assert hdr.raw == comp[:16], path
        with_ck += ck.value
        with_dict += did.value != 0
        # footer: from its own size and hash
        total, stored = int.from_bytes(comp[-12:-4], "little"), int.from_bytes(comp[-4:], "little")
        foot = C.create_string_buffer(12)
        shim.t_put_footer(foot, total, stored)
        assert foot.raw == comp[-12:], path
        # EOF block, where the chain ends cleanly at one
        b8 = C.create_string_buffer(8)
        eof_at = shim.t_chain_eof(comp, len(comp), ck.value)
        if eof_at >= 0:
            shim.t_put_blk_hdr(b8, BLK_EOF, 0)
            assert b8.raw == comp[eof_at: eof_at + 8], path
            with_eof += 1
        # seek-table header, where the archive ends in a table
        bs = 1 << lg.value
        nb, at = -(-total // bs), C.c_uint64()
        if nb and shim.t_seek_tail(comp, len(comp), nb, C.byref(at)):
            shim.t_put_blk_hdr(b8, BLK_SEK, 4 * nb)
            assert b8.raw == comp[at.value + 8: at.value + 16], path
            if eof_at >= 0:
                assert at.value == eof_at, path
            with_seek += 1
        visited += 1
    assert visited == len(paths) and visited > 0
    assert with_ck >= 1 and with_dict >= 1 and with_seek >= 1 and with_eof >= 1, (with_ck, with_dict, with_seek, with_eof)
    names = {os.path.basename(p) for p in paths}
    assert {"text_1k_checksum.zxc", "dict_http.zxc", "seekable_4blocks.zxc"} <= names


def test_hash_fold_is_rotl1_xor(shim):
    h = 0
    for t in (0x80000001, 0xDEADBEEF, 0, 0xFFFFFFFF, 0x12345678):
        want = (((h << 1) | (h >> 31)) & 0xFFFFFFFF) ^ t
        h = shim.t_hash_fold(h, t)
        assert h == want
