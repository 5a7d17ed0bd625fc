"""What the tests of the decode executors share, on the device and on the CPU wave emulator: the `dev` fixture and the guarded
launch of the limits tests, the `emu` fixture with its path counters and guarded launch, and the Runner of the launch-plan tests
with the HIP runtime's stream maker. A plain module next to the tests; a test file imports the fixtures it uses by name (pytest
finds a fixture in the module that holds its name)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import decode_limit_cases as D
import decode_plan_cases as P

sys.path.insert(0, os.path.join(D.ROOT, "tests", "wave_emu"))

IDS = D.path_ids()

_DECODE_BLOCKS_DICT = (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_void_p])


def _bind_decode_blocks_dict(L):
    L.zxc_mi355x_decode_blocks_dict_device.restype, L.zxc_mi355x_decode_blocks_dict_device.argtypes = _DECODE_BLOCKS_DICT
    return L


# ---------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def dev(product):
    import torch
    assert product.lib().zxc_mi355x_device_count() >= 1, "no HIP device"
    product.lib().zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    _bind_decode_blocks_dict(product.lib())
    return product


def launch(dev, case, lcases, what):
    """One guarded launch of a packed job table on the default stream, then the checks."""
    import torch
    size = P.guarded_layout(case, seed=case.n)
    d_comp = torch.frombuffer(bytearray(case.comp) + bytearray(64), dtype=torch.uint8).to("cuda")
    d_jobs = torch.frombuffer(bytearray(case.jobs.tobytes()), dtype=torch.uint8).to("cuda")
    d_out = torch.from_numpy(P.canary(size)).to("cuda")
    d_st = torch.full((case.n,), -999, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if case.dict_ is not None:
        d_dict = torch.frombuffer(bytearray(case.dict_), dtype=torch.uint8).to("cuda")
        torch.cuda.synchronize()
        rc = dev.lib().zxc_mi355x_decode_blocks_dict_device(d_comp.data_ptr(), d_jobs.data_ptr(), case.n, d_out.data_ptr(), d_st.data_ptr(),
                                                            case.block_size, int(case.checksum), d_dict.data_ptr(), len(case.dict_), None, None)
        assert rc == 0, (what, rc)
    else:
        dev.decode_blocks_device(d_comp.data_ptr(), d_jobs.data_ptr(), case.n, d_out.data_ptr(), d_st.data_ptr(), case.block_size,
                                 case.checksum, 0)
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    try:
        P.check_guarded(case, out, st, what)
    except AssertionError as e:
        raise AssertionError(f"{what}: {D.explain(case, lcases, out, st)}\n{e}") from None


def _hip():
    """The HIP runtime the process already uses (torch loads it before the product library)."""
    import torch  # noqa: F401
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    H = C.CDLL(path or "libamdhip64.so")
    H.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    H.hipStreamCreateWithFlags.restype = C.c_int
    return H


def new_stream(H):
    s = C.c_void_p()
    assert H.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value  # hipStreamNonBlocking
    return s.value


class Runner:
    """Uploads a case, lays its output out guarded, launches it on a stream and checks the result."""

    def __init__(self, zxc):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.L = _bind_decode_blocks_dict(zxc.lib())
        self.zxc = zxc

    def run(self, case, stream, what=""):
        torch = self.torch
        size = P.guarded_layout(case, seed=case.n)
        d_comp = torch.frombuffer(bytearray(case.comp) + bytearray(64), dtype=torch.uint8).to(self.dev)
        d_jobs = torch.frombuffer(bytearray(case.jobs.tobytes()), dtype=torch.uint8).to(self.dev)
        d_out = torch.from_numpy(P.canary(size)).to(self.dev)
        d_st = torch.full((case.n,), -999, dtype=torch.int32, device=self.dev)
        keep = []
        torch.cuda.synchronize()
        if case.dict_ is not None:
            d_dict = torch.frombuffer(bytearray(case.dict_), dtype=torch.uint8).to(self.dev)
            d_huf = torch.frombuffer(bytearray(case.dict_huf), dtype=torch.uint8).to(self.dev) if case.dict_huf else None
            keep += [d_dict, d_huf]
            torch.cuda.synchronize()
            rc = self.L.zxc_mi355x_decode_blocks_dict_device(d_comp.data_ptr(), d_jobs.data_ptr(), case.n, d_out.data_ptr(), d_st.data_ptr(),
                                                             case.block_size, int(case.checksum), d_dict.data_ptr(), len(case.dict_),
                                                             d_huf.data_ptr() if d_huf is not None else None, stream)
            assert rc == 0, (case.label, rc)
        else:
            self.zxc.decode_blocks_device(d_comp.data_ptr(), d_jobs.data_ptr(), case.n, d_out.data_ptr(), d_st.data_ptr(), case.block_size,
                                          case.checksum, stream)
        torch.cuda.synchronize()  # (the launch's hint has landed before the next launch on this stream reads it)
        P.check_guarded(case, d_out.cpu().numpy(), d_st.cpu().numpy(), what)


# ---------------------------------------------------------------- on the CPU wave emulator
@pytest.fixture(scope="module")
def emu():
    import emu_py
    e = emu_py.Emu()
    e.lib.emu_path_read.argtypes = [C.c_void_p, C.c_uint32]
    e.lib.emu_path_read.restype = C.c_uint32
    e.lib.emu_set_pscratch_bytes.argtypes = [C.c_size_t]
    e.lib.emu_set_rscratch_bytes.argtypes = [C.c_size_t]
    assert e.lib.emu_path_read(None, 0) == len(IDS), "enum zxc_path_id and the emulator library disagree"
    return e


def counts(emu):
    a = np.zeros(len(IDS), dtype=np.uint64)
    emu.lib.emu_path_read(a.ctypes.data, len(IDS))
    return {n: int(a[i]) for n, i in IDS.items()}


def run(emu, case, lcases, route, **kw):
    """One guarded launch; -> the path counters of it."""
    size = P.guarded_layout(case)
    if route == "strict":
        kw["cap_override"] = case.block_size
    emu.lib.emu_path_reset()
    st, out = emu.decode_jobs(case.comp, case.jobs, size, case.block_size, verify_trailer=case.checksum, dict_=case.dict_,
                              init=P.canary(size).tobytes(), **kw)
    o = np.frombuffer(out, dtype=np.uint8)
    assert emu.last_pads == 0, (case.label, "a store landed outside the output buffer", emu.last_pads)
    try:
        P.check_guarded(case, o, st)
    except AssertionError as e:
        raise AssertionError(f"{case.label}: {D.explain(case, lcases, o, st)}\n{e}") from None
    return counts(emu)
