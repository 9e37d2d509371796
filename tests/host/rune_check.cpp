// rune_check: jb_common.h's rune rules as a program of their own (no HIP), for tests/test_codepoint_cases.py.
//   rune_check decode FILE   FILE holds little-endian u32 words, four text bytes each; one line per word:
//                            jb_decode's rune and width under lim = 1, 2, 3, 4 (eight numbers)
//   rune_check classes       one line per value 0 .. 0x110000: jb_is_han, jb_is_space and jb_is_alnum
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jb_common.h"

static int decode_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        perror(path);
        return 2;
    }
    std::vector<uint32_t> words;
    uint32_t chunk[4096];
    size_t n;
    while ((n = fread(chunk, sizeof(uint32_t), 4096, f)) > 0) words.insert(words.end(), chunk, chunk + n);
    fclose(f);
    std::vector<char> line(128);
    for (uint32_t x : words) {
        int p = 0;
        for (uint32_t lim = 1; lim <= 4; lim++) {
            uint32_t r = 0xDEADBEEFu;
            const uint32_t w = jb_decode(x, lim, &r);
            p += snprintf(line.data() + p, line.size() - (size_t)p, "%u %u ", r, w);
        }
        line[(size_t)p - 1] = '\n';
        fwrite(line.data(), 1, (size_t)p, stdout);
    }
    return 0;
}

static int classes() {
    for (uint32_t r = 0; r <= 0x110000u; r++)
        printf("%d %d %d\n", (int)jb_is_han(r), (int)jb_is_space(r), (int)jb_is_alnum(r));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "decode")) return decode_file(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "classes")) return classes();
    fprintf(stderr, "usage: rune_check decode FILE | rune_check classes\n");
    return 2;
}
