"""Regenerates tests/golden/encoder_limits/digests.json: size and SHA-256 of the archive the encode kernel writes ON THE CPU WAVE
EMULATOR for every case of tests/encode_limit_cases.py, keyed by case, level and block size. This is the project's own output,
not the reference's: tests/test_gpu_encode_limits.py asks the device for the same bytes, so a deliberate change of the encoder
regenerates the file in the same commit.

    python tests/golden/make_encoder_limits.py           compare with the file, list the entries that differ
    python tests/golden/make_encoder_limits.py --write   rewrite the file"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("", "oracle", "tests", os.path.join("tests", "wave_emu")):
    sys.path.insert(0, os.path.join(ROOT, d))


def dict_id_fn(lib):
    lib.zxc_dict_id.restype = C.c_uint32
    lib.zxc_dict_id.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    return lambda d: int(lib.zxc_dict_id(d, len(d), None))


def generate():
    import emu_py
    import encode_limit_cases as E
    import oracle_py
    emu, did = emu_py.Emu(), dict_id_fn(oracle_py.Ref().lib)
    return {E.key(c, lv, ck): E.digest(E.emu_archives(emu, c, lv, ck, did)) for c in E.cases() for lv, ck in E.variants(c)}


def main():
    import encode_limit_cases as E
    path = os.path.join(ROOT, E.DIGESTS)
    new = generate()
    if "--write" in sys.argv[1:]:
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join('%s: %s' % (json.dumps(k), json.dumps(new[k], separators=(",", ":"))) for k in sorted(new)) + "\n}\n")
        print("wrote %d entries to %s" % (len(new), path))
        return 0
    old = json.load(open(path)) if os.path.exists(path) else {}
    diff = sorted(k for k in set(old) | set(new) if old.get(k) != new.get(k))
    for k in diff:
        print("differs:", k)
    print("%d entries, %d differ" % (len(new), len(diff)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
