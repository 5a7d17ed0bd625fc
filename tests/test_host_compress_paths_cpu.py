"""The host COMPRESS paths pinned without a GPU (zxc_compress, zxc_compress_block, zxc_compress_cctx, the contexts,
zxc_stream_compress, zxc_cstream_create) on the mock device of tests/mock_device: the block codec underneath is the reference's,
so every archive must be byte for byte the reference's and every verdict the reference's. These are the calls that read
zxc_compress_opts_t, run the serial (dictionary) encode and write the archive tail; the pipelined no-dictionary paths are in
tests/test_host_mock_device.py."""
import ctypes as C
import random

import pytest

import oracle_py
import zxc_amd.api as api

BS = 4096
NULL_INPUT, DST_TOO_SMALL, BAD_BLOCK_SIZE, DICT_TOO_LARGE = -12, -2, -14, -17
PATTERN = 0xA5


def _text(rng, n, vocab=60):  # the word-list generator of tests/test_host_mock_device.py
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz ,.") for _ in range(rng.randrange(3, 10))) for _ in range(vocab)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words)
    return bytes(out[:n])


@pytest.fixture(scope="module")
def libs(mockdev, ref):
    for L in (mockdev, ref.lib):
        oracle_py.bind_zxc_api(L)
    return mockdev, ref.lib


@pytest.fixture(scope="module")
def corpus():
    rng = random.Random(20261020)
    return _text(rng, 20000), _text(rng, 3 * (1 << 20) + 4321)  # (the dictionary, the text every case cuts its input from)


def _opts(dict_=None, dict_size=None, dict_huf=None, **kw):
    """-> (CompressOpts, the buffers it points to)"""
    o = oracle_py.CompressOpts(**kw)
    keep = []
    if dict_ is not None:
        keep.append(C.create_string_buffer(dict_, len(dict_)))
        o.dict = C.cast(keep[-1], C.c_void_p)
        o.dict_size = len(dict_) if dict_size is None else dict_size
    elif dict_size is not None:
        o.dict_size = dict_size
    if dict_huf is not None:
        keep.append(C.create_string_buffer(dict_huf, 128))
        o.dict_huf = C.cast(keep[-1], C.c_void_p)
    return o, keep


def _compress(L, data, cap=None, null_dst=False, **kw):
    """zxc_compress into a REAL buffer of zxc_compress_bound + 4096 bytes filled with a pattern, whatever capacity is stated
    (the reference writes ~4 KiB past a stated capacity of 16..35 bytes before it answers -2). -> (rc, the archive, what lies
    at and behind the stated capacity)"""
    o, _keep = _opts(**kw)
    bound = int(L.zxc_compress_bound(len(data)))
    real = bound + 4096
    cap = bound if cap is None else cap
    buf = C.create_string_buffer(bytes([PATTERN]) * real, real)
    rc = L.zxc_compress(data, len(data), None if null_dst else buf, cap, C.byref(o))
    return rc, buf.raw[:max(rc, 0)], buf.raw[cap:]


@pytest.mark.parametrize("seekable,checksum", [(0, 0), (1, 1)])
@pytest.mark.parametrize("level", [1, 3, 6])
def test_compress_with_a_dictionary_writes_the_reference_s_archive(libs, corpus, level, seekable, checksum):
    mock, ref = libs
    dict_, text = corpus
    for n in (0, 1, 4095, 4096, 4097, 9 * 4096 + 77):
        kw = dict(level=level, block_size=BS, seekable=seekable, checksum_enabled=checksum, dict_=dict_)
        want = _compress(ref, text[:n], **kw)
        got = _compress(mock, text[:n], **kw)
        assert want[0] > 0 and got[:2] == want[:2], (n, got[0], want[0])
        assert got[2] == bytes([PATTERN]) * 4096
        if n == 0:
            assert got[0] == 36


def _block_api(L):
    L = oracle_py.bind_block_api(L)
    ctx = L.zxc_create_cctx(None)
    assert ctx
    return L, ctx


def _compress_block(L, ctx, data, cap, **kw):
    o, _keep = _opts(**kw)
    buf = C.create_string_buffer(bytes([PATTERN]) * 16384, 16384)
    rc = L.zxc_compress_block(ctx, data, len(data), buf, cap, C.byref(o))
    return rc, buf.raw[:max(rc, 0)], buf.raw[cap:]


def test_compress_block_with_a_dictionary(libs, corpus):
    mock, ref = libs
    dict_, text = corpus
    src = text[5000:8000]
    res = {}
    for L in (mock, ref):
        L, ctx = _block_api(L)
        res[L is mock] = [_compress_block(L, ctx, src, 8192, block_size=BS, checksum_enabled=ck, dict_=dict_)[:2] for ck in (0, 1)]
        L.zxc_free_cctx(ctx)
    assert res[True] == res[False]
    (n0, b0), (n1, b1) = res[True]
    assert n0 > 8 and n1 == n0 + 4 and b1[:3] == b0[:3] and b1[8:n0] == b0[8:]  # (the same block + its 4-byte trailer)
    for kw in (dict(dict_=dict_), {}):
        for L in (mock, ref):
            L, ctx = _block_api(L)
            rc, _, behind = _compress_block(L, ctx, src, 16, block_size=BS, **kw)
            L.zxc_free_cctx(ctx)
            assert rc == DST_TOO_SMALL, (L is mock, bool(kw), rc)
            if L is mock:
                assert behind == bytes([PATTERN]) * (16384 - 16)


@pytest.mark.parametrize("seekable,checksum", [(True, True), (False, False)])
def test_stream_compress_with_a_dictionary(libs, corpus, tmp_path, monkeypatch, seekable, checksum):
    """3 MiB + 4321 bytes in batches of 512 KiB of source: the file is the reference's one-shot archive with the same dictionary"""
    mock, ref = libs
    dict_, text = corpus
    monkeypatch.setenv("ZXC_STREAM_BATCH_BYTES", str(2 << 20))
    src, arc = tmp_path / "in.bin", tmp_path / "a.zxc"
    src.write_bytes(text)
    n = api.stream_compress(str(src), str(arc), level=3, block_size=BS, seekable=seekable, checksum=checksum, library=mock, dict_=dict_)
    want = _compress(ref, text, level=3, block_size=BS, seekable=int(seekable), checksum_enabled=int(checksum), dict_=dict_)
    assert want[0] > 0 and n == want[0] == arc.stat().st_size
    assert arc.read_bytes() == want[1]


def test_compress_error_precedence(libs, corpus):
    mock, ref = libs
    dict_, text = corpus
    big = text[:70000]
    data = text[:10000]
    cases = [  # (what, input, keywords of _compress, the verdict)
        ("NULL dst", data, dict(null_dst=True), NULL_INPUT),
        ("capacity 0", data, dict(cap=0), NULL_INPUT),
        ("block size 5000", data, dict(block_size=5000), BAD_BLOCK_SIZE),
        ("block size 2048", data, dict(block_size=2048), BAD_BLOCK_SIZE),
        ("block size 1<<22", data, dict(block_size=1 << 22), BAD_BLOCK_SIZE),
        ("dict_size 70000", data, dict(dict_=big), DICT_TOO_LARGE),
        ("dict_size 70000, block size 5000", data, dict(dict_=big, block_size=5000), DICT_TOO_LARGE),  # the dictionary is judged first
        ("capacity 15", data, dict(cap=15), DST_TOO_SMALL),
        ("capacity 15, block size 5000", data, dict(cap=15, block_size=5000), BAD_BLOCK_SIZE),
        ("capacity 20, 5000 bytes", text[:5000], dict(cap=20), DST_TOO_SMALL),
    ]
    for what, src, kw, verdict in cases:
        kw = dict(dict(level=3, block_size=BS), **kw)
        for L in (mock, ref):
            rc, _, behind = _compress(L, src, **kw)
            assert rc == verdict, (what, L is mock, rc)
            if L is mock and not kw.get("null_dst"):
                assert behind == bytes([PATTERN]) * len(behind), what  # nothing at or behind the stated capacity was written
    # a seekable archive fits one byte below the bound
    bound = int(ref.zxc_compress_bound(len(data)))
    want = _compress(ref, data, cap=bound - 1, level=3, block_size=BS, seekable=1)
    got = _compress(mock, data, cap=bound - 1, level=3, block_size=BS, seekable=1)
    assert want[0] > 0 and got[:2] == want[:2]
    assert got[2] == bytes([PATTERN]) * (4096 + 1)
    # levels beyond the range: 99 is level 7, a negative one the default
    for L in (mock, ref):
        assert _compress(L, data, level=99, block_size=BS)[:2] == _compress(L, data, level=7, block_size=BS)[:2]
        assert _compress(L, data, level=-3, block_size=BS)[:2] == _compress(L, data, level=0, block_size=BS)[:2] \
            == _compress(L, data, level=3, block_size=BS)[:2]
    assert _compress(mock, data, level=99, block_size=BS)[:2] == _compress(ref, data, level=99, block_size=BS)[:2]
    assert _compress(mock, data, level=-3, block_size=BS)[:2] == _compress(ref, data, level=-3, block_size=BS)[:2]


def _compress_cctx(L, ctx, data, o):
    cap = int(L.zxc_compress_bound(len(data)))
    buf = C.create_string_buffer(cap)
    rc = L.zxc_compress_cctx(ctx, data, len(data), buf, cap, C.byref(o) if o is not None else None)
    return rc, buf.raw[:max(rc, 0)]


def test_contexts_read_their_options(libs, corpus, tmp_path):
    mock, ref = libs
    dict_, text = corpus
    data = text[:3 * BS + 5]
    L = oracle_py.bind_block_api(mock)
    assert not L.zxc_create_cctx(C.byref(oracle_py.CompressOpts(block_size=5000)))
    # level 99 at creation: a context of level 7
    ctx = L.zxc_create_cctx(C.byref(oracle_py.CompressOpts(level=99, block_size=BS)))
    assert ctx
    assert _compress_cctx(L, ctx, data, None) == _compress(mock, data, level=7, block_size=BS)[:2]
    L.zxc_free_cctx(ctx)
    # the static reader does not clamp: no workspace size for level 99
    L.zxc_static_cctx_workspace_size.restype = C.c_size_t
    L.zxc_static_cctx_workspace_size.argtypes = [C.c_size_t, C.c_int]
    L.zxc_init_static_cctx.restype = C.c_void_p
    L.zxc_init_static_cctx.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    ws = C.create_string_buffer(4096 + 64)
    base = (C.addressof(ws) + 63) & ~63
    assert L.zxc_static_cctx_workspace_size(BS, 99) == 0
    assert not L.zxc_init_static_cctx(base, 4096, C.byref(oracle_py.CompressOpts(level=99, block_size=BS)))
    assert L.zxc_init_static_cctx(base, 4096, C.byref(oracle_py.CompressOpts(level=7, block_size=BS)))
    # zxc_compress_cctx: without options the context's checksum setting, with options theirs (0 included)
    ctx = L.zxc_create_cctx(C.byref(oracle_py.CompressOpts(level=3, block_size=BS, checksum_enabled=1)))
    assert ctx
    with_ck = _compress(mock, data, level=3, block_size=BS, checksum_enabled=1)[:2]
    without = _compress(mock, data, level=3, block_size=BS)[:2]
    assert with_ck != without
    assert _compress_cctx(L, ctx, data, None) == with_ck
    assert _compress_cctx(L, ctx, data, oracle_py.CompressOpts()) == without
    assert _compress_cctx(L, ctx, data, None) == without  # (the call's options stick to the context)
    assert _compress_cctx(L, ctx, data, oracle_py.CompressOpts(checksum_enabled=1)) == with_ck
    L.zxc_free_cctx(ctx)
    # the push stream refuses a dictionary, whichever of its three fields is set
    api._bind_pstream(mock)
    buf = C.create_string_buffer(dict_, len(dict_))
    for kw in (dict(dict=C.addressof(buf)), dict(dict_size=100), dict(dict_huf=C.addressof(buf))):
        assert not mock.zxc_cstream_create(C.byref(api._CompressOpts(block_size=BS, **kw))), kw
    cs = mock.zxc_cstream_create(C.byref(api._CompressOpts(block_size=BS)))
    assert cs
    mock.zxc_cstream_free(cs)
    # zxc_stream_compress judges the block size in front of the dictionary (zxc_compress: the other way round)
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    assert api.stream_compress(str(src), str(tmp_path / "a.zxc"), block_size=5000, library=mock, dict_=text[:70000]) == BAD_BLOCK_SIZE
    assert api.stream_compress(str(src), str(tmp_path / "a.zxc"), block_size=BS, library=mock, dict_=text[:70000]) == DICT_TOO_LARGE
