"""What the CPU tests of the device calls share: the host C compiler's command lines for the rule shims (tests/*/..._shim.c, loaded
with ctypes) and for the stand-alone sanitizer programs (tests/*/..._san_main.c, each with its own main: nothing of them is loaded
into this process), and the small makers of options and dictionary structs their argument checks use."""
import ctypes as C
import os
import subprocess

from conftest import ROOT
from zxc_amd.api import _CompressOpts, _DevDict

GCC = ["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
SAN_MARKERS = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")

FAKE_DICT, FAKE_HUF, FAKE_ID = 0x70000, 0x80000, 0x90000  # device pointers that are never dereferenced


def build_shim(tmp_path_factory, name, source, flags=()):
    """tests/<source> as a shared library in a directory of its own -> CDLL"""
    so = str(tmp_path_factory.mktemp(name) / f"lib{name}_shim.so")
    subprocess.run(GCC + list(flags) + ["-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", source)], check=True)
    return C.CDLL(so)


def run_san_program(tmp_path, source, args=(), flags=()):
    """tests/<source> (a program with its own main) built with AddressSanitizer and UBSan and run once: it compiles, exits 0 and
    reports nothing -> the completed process, for the caller's own "... OK <count>" line"""
    exe = str(tmp_path / os.path.basename(source).replace("_main.c", ""))
    r = subprocess.run(GCC + list(flags) + SANITIZE + ["-o", exe, os.path.join(ROOT, "tests", source)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    bad = [k for k in SAN_MARKERS if k in r.stderr]
    assert r.returncode == 0 and not bad, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return r


def ref(x):
    return C.byref(x) if x is not None else None


def opts(level=3, block_size=65536, seekable=False, checksum=False):
    return _CompressOpts(level=level, block_size=block_size, seekable=int(seekable), checksum_enabled=int(checksum))


def host_dict(o, src=0x10000):
    """the opts with a host dictionary set, which every device call refuses"""
    o.dict, o.dict_size = src, 100
    return o


def dd(size=1000, content=FAKE_DICT, huf=FAKE_HUF, id_=FAKE_ID):
    return _DevDict(content, huf, id_, size)
