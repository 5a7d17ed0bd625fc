"""What the CPU tests of compress_batch_device and compress_pack_device share: the fake device pointers and the stated sizes, the
ctypes mirrors of the rules' structs (zxc_amd/csrc/zxc_cbatch.h), an archive cut into its blocks, and the reference's archives the
rules put together again. A plain module next to the tests, imported the way cshim is; the names are the ones the two test files
use."""
import ctypes as C

import numpy as np

import cshim
from cshim import FAKE_DICT, FAKE_HUF, FAKE_ID, dd as _dd, opts as _opts, ref as _ref  # noqa: F401  (both test files take them from here)
from devtest import ERR  # noqa: F401

FAKE_SRC, FAKE_ITEMS, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
REC_BYTES, JOB_BYTES, WORK_FIXED, IMAGE_FIXED = 64, 28, 1536, 320  # the stated bound: n J (S + 28) + 64 n + 1536 (+ images + 320)
CANARY = 0xC3
M64 = (1 << 64) - 1


def _stride(bs):
    return 2 * bs + 512  # zxc_mi355x_encode_slot_stride, checked against the library below


def _host_dict_opts(**kw):
    return cshim.host_dict(_opts(**kw))


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Rec(C.Structure):  # zcb_rec_t
    _fields_ = [("result", C.c_int64), ("dst_off", C.c_uint64), ("cap", C.c_uint64), ("src_size", C.c_uint64), ("nb", C.c_uint32),
                ("rsv0", C.c_uint32), ("rsv", C.c_uint64 * 3)]


class Item(C.Structure):  # zxc_dev_item_t
    _fields_ = [("src_off", C.c_uint64), ("src_size", C.c_uint64), ("dst_off", C.c_uint64), ("dst_capacity", C.c_uint64)]


class Shape(C.Structure):  # zcb_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_jobs", "slot_stride", "chunk_jobs")] + \
               [(n, C.c_uint64) for n in ("o_rec", "o_jobs", "o_sizes", "o_offsets", "o_slots", "o_images", "bytes")]


JOB = np.dtype([("src_off", "<u8"), ("len", "<u4"), ("pad", "<u4")])


class Arc:
    """an archive cut into its parts: the blocks with their headers (and trailers), and what the header and footer say"""

    def __init__(self, comp, what):
        self.comp, self.what = comp, what
        assert int.from_bytes(comp[0:4], "little") == 0x9CB02EF5 and comp[4] == 8
        self.bs = 1 << comp[5]
        self.checksum, self.has_dict = bool(comp[6] & 0x80), bool(comp[6] & 0x40)
        self.dict_id = int.from_bytes(comp[7:11], "little") if self.has_dict else 0
        self.blocks, at = [], 16
        while comp[at] != 255:
            n = 8 + int.from_bytes(comp[at + 3: at + 7], "little") + (4 if self.checksum else 0)
            self.blocks.append(comp[at: at + n])
            at += n
        rest = len(comp) - at - 8 - 12
        self.seekable = rest > 0
        assert rest == ((8 + 4 * len(self.blocks)) if self.seekable else 0), what
        self.size = int.from_bytes(comp[-12:-4], "little")
        self.regular = len(self.blocks) == -(-self.size // self.bs)  # one block per block_size bytes of the source


_REF_ARCS = {}


def _ref_arcs(ref, bs, checksum, seekable):
    from zxc_amd import corpus
    key = (bs, checksum, seekable)
    if key not in _REF_ARCS:
        text = corpus.synth_text(4 * bs, seed=11)
        noise = np.random.default_rng(bs).integers(0, 256, 4 * bs, dtype=np.uint8).tobytes()
        out = []
        for k, n in enumerate((0, 1, 33, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5)):
            data = (noise if k % 3 == 2 else text)[:n]
            out.append(Arc(ref.compress(data, 1 + k % 5, bs, bool(seekable), bool(checksum)), (n, bs, checksum, seekable)))
        _REF_ARCS[key] = out
    return _REF_ARCS[key]
