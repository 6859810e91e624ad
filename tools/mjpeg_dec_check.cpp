// mjpeg_dec_check FILE.jpg [FILE.jpg ...]: the Motion-JPEG decoder's parser and shared entropy routine (csrc/mjpeg_dec.cpp,
// csrc/mjpeg_dec_core.h) as host code under the sanitizers, on damaged input.  Build (tests/test_mjpeg_dec_cpu.py does):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I kalman-hydra_amd/csrc tools/mjpeg_dec_check.cpp kalman-hydra_amd/csrc/mjpeg_dec.cpp -o mjpeg_dec_check -lpthread
//
// and once more at -O3, the library's level (clang: -static-libsan for the two -static-lib flags).  The sanitizers'
// runtimes are linked statically.  The pool of host threads is exercised too: the clean file is decoded through MjdPool.
//
// For every file: the file itself must decode clean; then every prefix of it and every single-bit flip of it is parsed
// and, when the parser accepts it, decoded.  Each such input must be refused, or decode with bad intervals counted, or
// decode clean -- and touch nothing outside its buffers, which is what the sanitizers watch: the input and the
// coefficients live in heap blocks of exactly their size.  Exit 0 and one summary line per file when all is well.
#include "mjpeg_dec_core.h"
#include "../include/hydra_mi.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static char g_err[512];
void hm_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Count { long refused = 0, bad = 0, clean = 0; };

// 0 refused, 1 decoded with bad intervals, 2 clean; -1: the decoder broke a promise
static int decode(const uint8_t *data, size_t n, int W, int H)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);                  // exactly n bytes: a read past them is a report
    memcpy(file, data, n);
    MjdParsed p;
    g_err[0] = 0;
    const int rc = mjd_parse(file, n, &p);
    int result = 0;
    if (rc != HM_OK) {
        if (rc != HM_ERR_ARG || !g_err[0]) result = -1;            // a refusal names its cause
    } else if (p.W != W || p.H != H) {
        result = 0;                                                // the decoder refuses another size
    } else {
        const size_t blocks = (size_t)p.frame.scan.n_mcu * p.hs * p.vs;
        int16_t *coef = (int16_t *)aligned_alloc(128, blocks * 128);
        memset(coef, 0x55, blocks * 128);
        const uint32_t bad = mjd_entropy_host(p, file, coef);
        if (bad > p.intervals.size()) result = -1;
        else result = bad ? 1 : 2;
        for (const MjdInterval &iv : p.intervals)                  // the table the device would get
            if (iv.start > iv.end || iv.end > n) result = -1;
        free(coef);
    }
    free(file);
    return result;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: mjpeg_dec_check FILE.jpg [FILE.jpg ...]\n");
        return 2;
    }
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(f);
        MjdParsed p;
        if (mjd_parse(data.data(), data.size(), &p) != HM_OK) { fprintf(stderr, "%s: refused: %s\n", argv[a], g_err); return 1; }
        const int W = p.W, H = p.H;
        if (decode(data.data(), data.size(), W, H) != 2) { fprintf(stderr, "%s: does not decode clean\n", argv[a]); return 1; }
        {                                                          // the same file four times through the pool, twice
            MjdPool pool(3);
            const size_t blocks = (size_t)p.frame.scan.n_mcu * p.hs * p.vs;
            std::vector<int16_t *> coef(4);
            for (int16_t *&q : coef) q = (int16_t *)aligned_alloc(128, blocks * 128);
            const MjdParsed *ps[4] = {&p, &p, &p, &p};
            const uint8_t *fs[4] = {data.data(), data.data(), data.data(), data.data()};
            uint32_t bad[4];
            for (int round = 0; round < 2; round++) {
                for (uint32_t &x : bad) x = 99;
                pool.run(4, ps, fs, coef.data(), bad);
                for (int i = 0; i < 4; i++)
                    if (bad[i] != 0 || memcmp(coef[i], coef[0], blocks * 128)) { fprintf(stderr, "%s: the pool's decode %d differs\n", argv[a], i); return 1; }
            }
            for (int16_t *q : coef) free(q);
        }
        Count c;
        auto tally = [&](int r, const char *what, size_t at) {
            if (r < 0) { fprintf(stderr, "%s: %s %zu: the decoder broke a promise (%s)\n", argv[a], what, at, g_err); exit(1); }
            (r == 0 ? c.refused : r == 1 ? c.bad : c.clean)++;
        };
        for (size_t n = 0; n < data.size(); n++) tally(decode(data.data(), n, W, H), "prefix", n);
        std::vector<uint8_t> flip(data);
        for (size_t bit = 0; bit < 8 * data.size(); bit++) {
            flip[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            tally(decode(flip.data(), flip.size(), W, H), "bit", bit);
            flip[bit >> 3] = data[bit >> 3];
        }
        printf("%s: %zu bytes, %ld inputs: %ld refused, %ld with bad intervals, %ld clean\n", argv[a], data.size(),
               c.refused + c.bad + c.clean, c.refused, c.bad, c.clean);
    }
    return 0;
}
