"""What the tests of the device calls share: the `gpu` fixture, the error codes, and the makers of inputs, device buffers and
dictionaries. A plain module next to the tests, imported the way conftest is. Where the tests' own copies differed, the difference
is an argument here and each test file passes the value its copy had."""
import ctypes as C

import numpy as np
import pytest

UNSET = -(1 << 62)  # a result word nothing has written
CANARY = 4096       # pattern bytes behind a capacity
PAD = 64            # an archive or source area in device memory must be readable 64 bytes past its end

# include/zxc_error.h
ERR = dict(MEMORY=-1, DST_TOO_SMALL=-2, SRC_TOO_SMALL=-3, BAD_MAGIC=-4, BAD_VERSION=-5, BAD_HEADER=-6, BAD_CHECKSUM=-7, CORRUPT_DATA=-8,
           BAD_OFFSET=-9, OVERFLOW=-10, IO=-11, NULL_INPUT=-12, BAD_BLOCK_TYPE=-13, BAD_BLOCK_SIZE=-14, DICT_REQUIRED=-15,
           DICT_MISMATCH=-16, DICT_TOO_LARGE=-17, BAD_LEVEL=-18, GPU_UNAVAILABLE=-100, GPU_UNSUPPORTED=-101)


def gpu_fixture(needs=None, session_method=None, torch_device=True):
    """-> the module-scoped `gpu` fixture of a test file: a device is present, then zxc_amd has the name `needs` (or
    zxc_amd.api's session class `session_method[0]` the method `session_method[1]`); the product is returned with device 0
    selected, in torch too unless the file does not use torch."""
    @pytest.fixture(scope="module", name="gpu")
    def gpu(product):
        if torch_device:
            import torch
        assert product.lib().zxc_mi355x_device_count() >= 1, "no HIP device"
        if needs:
            assert hasattr(product, needs), f"zxc_amd has no {needs}"
        if session_method:
            assert hasattr(getattr(product.api, session_method[0]), session_method[1]), "zxc_amd has no %s.%s" % session_method
        product.lib().zxc_mi355x_set_device(0)
        if torch_device:
            torch.cuda.set_device(0)
        return product
    return gpu


def area_4k_fixture(area_class, sizes, make_payload):
    """-> the module-scoped `area_4k` fixture of the compress batch and pack tests"""
    @pytest.fixture(scope="module", name="area_4k")
    def area_4k(gpu):
        """every size of the issue as text and as bytes that do not compress, shuffled in the table"""
        import random
        area = area_class(gpu, 21)
        for k, size in enumerate(sizes):
            area.add(make_payload(size, 4 * k))      # text
            area.add(make_payload(size, 4 * k + 3))  # incompressible
        order = list(range(len(area.rows)))
        random.Random(5).shuffle(order)
        return area, area.tensor(), area.table(order), [area.datas[k] for k in order]
    return area_4k


def pattern(n):
    return np.tile(np.arange(1, 252, dtype=np.uint8), n // 251 + 1)[:n]


def to_dev(data: bytes, pad=0, exact=False):
    """-> uint8 tensor of len(data) + pad bytes (the pad is 0xA5: never used, only readable). exact: the bytes alone, moved as
    they are (no fill, no pad)."""
    import torch
    if exact:
        if not data:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    t = torch.full((len(data) + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[: len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    return t


def bound(gpu, n):
    return int(gpu.lib().zxc_compress_bound(n))


_TEXT = {}


def text(size):
    """the generated text of `size` bytes the payloads and dictionaries are cut from, made once"""
    from zxc_amd import corpus
    if size not in _TEXT:
        _TEXT[size] = corpus.synth_text(size, seed=17)
    return _TEXT[size]


def payload(n, seed, stored_every=2, text_size=6 << 20):
    """a slice of one generated text of text_size bytes (a function of n where the size depends on it), or bytes that do not
    compress (stored blocks) for the last seed of every `stored_every`: the odd seeds, or every fourth"""
    if seed % stored_every == stored_every - 1:
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    size = text_size(n) if callable(text_size) else text_size
    at = (seed * 100003) % (size - n + 1)
    return text(size)[at: at + n]


def canary(n=CANARY):
    import torch
    return torch.arange(n, dtype=torch.int32).remainder(251).to(torch.uint8) + 1


def canary_ok(dst, cap, n=CANARY):
    import torch
    return torch.equal(dst[cap:].cpu(), canary(n))


def inputs(bs):
    from zxc_amd import corpus
    rng = np.random.default_rng(bs)
    text = corpus.synth_text(3 * bs + 1000, seed=bs & 0xFFFF)
    return {
        "empty": b"",
        "1B": b"Q",
        "bs-1": text[: bs - 1],
        "bs": text[bs: 2 * bs],
        "bs+1": text[7: bs + 8],
        "text": text,
        "random": rng.integers(0, 256, 2 * bs + 77, dtype=np.uint8).tobytes(),
        "zeros": bytes(2 * bs + 5),
    }


def piece(data: bytes, k):
    """the piece's bytes at an odd offset of a buffer that ends with them -> (tensor that keeps it alive, pointer)"""
    import torch
    off = 1 + 2 * (k % 7)
    t = torch.full((off + len(data),), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[off:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    return t, t.data_ptr() + off


def split(data, lens):
    assert sum(lens) == len(data)
    out, at = [], 0
    for n in lens:
        out.append(data[at: at + n])
        at += n
    return out


class DevDict:
    """a dictionary in device memory: content, optional table, the prepared id word. odd: the content lies at an odd address.
    The tensors have exactly the dictionary's length, but torch's allocator rounds an allocation up, so these tests could not see
    a read past `size`: that the calls make none is established by reading the kernels (include/zxc_mi355x.h)."""

    def __init__(self, gpu, content, huf=None, stream=None, odd=False):
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        self.content, self.huf = content, huf
        with torch.cuda.stream(s):
            self.d_content = to_dev(b"\xA5" + content if odd else content)
            self.d_huf = to_dev(huf) if huf else None
            self.d_id = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            self.tup = (self.d_content.data_ptr() + int(odd), len(content), self.d_huf.data_ptr() if huf else 0, self.d_id.data_ptr())
            gpu.dict_prepare_device(self.tup[0], len(content), self.tup[2], self.tup[3], s.cuda_stream)

    def id(self):
        import torch
        torch.cuda.synchronize()
        return int(self.d_id.cpu().numpy().view(np.uint32)[0])


def device_written(gpu, data, level, bs, seekable, checksum):
    """compress_device -> the archive as a device tensor"""
    import torch
    src = to_dev(data)
    cap = bound(gpu, len(data))
    ws = gpu.compress_device_work_size(len(data), level, bs, seekable, checksum)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.empty(cap, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    gpu.compress_device(src.data_ptr() if data else 0, len(data), arc.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level, bs,
                        seekable, checksum)
    n = int(res.item())
    assert n > 0
    return arc[:n]


def ref_decompress(ref, comp, n, content=None, huf=None, checksum=False):
    """the unmodified reference's zxc_decompress, options built as in tests/test_gpu_encode.py::test_dictionary_compression"""
    import oracle_py
    o = oracle_py.DecompressOpts()
    o.checksum_enabled = int(checksum)
    keep = None
    if content:
        keep = (C.create_string_buffer(content, len(content)), C.create_string_buffer(huf, 128) if huf else None)
        o.dict, o.dict_size = C.cast(keep[0], C.c_void_p), len(content)
        o.dict_huf = C.cast(keep[1], C.c_void_p) if huf else None
    out = C.create_string_buffer(max(n, 1))
    rc = ref.lib.zxc_decompress(comp, len(comp), out, n, C.byref(o))
    return rc, out.raw[:max(rc, 0)]
