/* Stand-alone program (its own main, not loaded into anything) that replays dictionary sessions of zxc_amd/csrc/zxc_append.h the
 * way the entry points and kernels of zxc_append_device.hip run them (append_dict_replay.h), over heap buffers of exactly the sizes
 * a session is promised, so that AddressSanitizer and UBSan see any read or write outside them: archives of stored blocks built
 * serially here with a dictionary header (rpd_selftest), the promises of every images-mode plan near the block boundaries, and for
 * every triple of arguments <archive> <decoded bytes> <dictionary content> that archive cut near the ends of its first block at
 * every byte, between them at every 97th (the test runs every byte boundary outside this program), and at random. Built by tests/test_compress_append_dict_device_cpu.py with -fsanitize=address,undefined.
 * Prints "APPEND DICT OK <cut sets>" and exits 0. */
#include "../container/san_util.h"

#include "append_dict_replay.h"

static uint8_t* slurp(const char* path, uint64_t* n) {
    FILE* f = fopen(path, "rb");
    CHECK(f != NULL);
    CHECK(fseek(f, 0, SEEK_END) == 0);
    const long size = ftell(f);
    CHECK(size >= 0 && fseek(f, 0, SEEK_SET) == 0);
    uint8_t* p = malloc(size ? (size_t)size : 1u); /* exactly the file's bytes */
    CHECK(fread(p, 1, (size_t)size, f) == (size_t)size);
    fclose(f);
    *n = (uint64_t)size;
    return p;
}

int main(int argc, char** argv) {
    int64_t sets = rpd_selftest();
    if (sets < 0) { fprintf(stderr, "append_dict_replay.h:%lld failed\n", (long long)-sets); return 1; }
    for (int a = 1; a + 2 < argc; a += 3) {
        uint64_t nc, nd, nx;
        uint8_t *comp = slurp(argv[a], &nc), *data = slurp(argv[a + 1], &nd), *dict = slurp(argv[a + 2], &nx);
        const int64_t rc = rpd_check_archive(comp, nc, data, nd, dict, (uint32_t)nx, 11u + (uint32_t)a, 0);
        if (rc < 0) { fprintf(stderr, "%s: append_dict_replay.h:%lld failed\n", argv[a], (long long)-rc); return 1; }
        sets += rc;
        free(dict); free(data); free(comp);
    }
    const uint32_t carries[] = {0u, 1u, 31u, 32u, 33u, 2048u, 4063u, 4064u, 4095u};
    for (unsigned c = 0; c < sizeof(carries) / sizeof(carries[0]); c++)
        for (uint64_t n = 1; n < 3u * 4096u + 70u; n += (n % 4096u < 70u || n % 4096u > 4026u) ? 1u : 97u) CHECK(rpd_plan_check(carries[c], n, 4096u) == 0);
    printf("APPEND DICT OK %lld\n", (long long)sets);
    return 0;
}
