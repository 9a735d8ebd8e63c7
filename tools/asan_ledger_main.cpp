// asan_ledger_main.cpp - the file ledger's host functions (hx_xhead.cpp: hx_ledger_open, hx_ledger_update,
// hx_xing_load_points, then hx_xing_update_info on the loaded points) over random call histories, as a stand-alone program
// for AddressSanitizer + UBSan: tools/asan_ledger.sh builds it together with hx_xhead.cpp and runs it.  No GPU, no Python.
// Checks nothing but what the sanitizers see and that every file ends; tests/test_ledger_host.py checks the values.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/hmp3_amd.h"

static unsigned long long rng_s = 88172645463325252ull;
static unsigned rnd(unsigned n) { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (unsigned) (rng_s >> 33) % n; }

int main()
{
    hx_xing *x = hx_xing_create();
    unsigned char tag[2048];
    int files = 0;
    for (int it = 0; it < 300; it++) {
        const int fpc = 1 + (it & 1), ncalls = it < 4 ? 1 + it : 1 + (int) rnd(it % 10 == 0 ? 2600 : 700);
        const int head = hx_xing_header(x, fpc == 1 ? 44100 : 22050, 1, 1, 1, 0x4F, 0, 0, 50, nullptr, tag, nullptr, nullptr, 128);
        HX_LEDGER r;
        hx_ledger_open(&r, ncalls, fpc, head, it % 7 ? 1 : 0);
        unsigned fr = 0, by = 0;
        int fed = 0;
        const int lag = (int) rnd(3 * fpc + 1);
        while (!r.ended && fed < ncalls + 64) {
            const int n = (int) rnd(97);            // 0 .. 96 frames, 0 included
            std::vector<int> st(2 * (size_t) n + 2);
            std::vector<unsigned short> crc((size_t) n + 1);
            const unsigned by0 = by;
            for (int f = 0; f < n; f++, fed++) {
                const unsigned want = (unsigned) ((fed + 1) * fpc > lag ? (fed + 1) * fpc - lag : 0);
                while (fr < want) { fr++; by += 96 + rnd(1100); }
                st[2 * f] = (int) fr; st[2 * f + 1] = (int) by;
                crc[f] = (unsigned short) rnd(65536);
            }
            hx_ledger_update(&r, st.data(), crc.data(), n, (int) (by - by0));
        }
        if (!r.ended) { fprintf(stderr, "file %d (%d calls) did not end\n", it, ncalls); return 1; }
        std::vector<int> st(2, 0);
        unsigned short c = 0;
        hx_ledger_update(&r, st.data(), &c, 1, 0);          // a call after the end
        HX_LEDGER_BRIEF brief;
        hx_ledger_brief(&r, r.bytes, &brief);               // the record's short form (file images)
        if (!brief.ended || brief.bytes != r.bytes || brief.call_bytes != 0) { fprintf(stderr, "file %d: brief differs\n", it); return 1; }
        if (!hx_xing_load_points(x, &r)) { fprintf(stderr, "file %d: points refused\n", it); return 1; }
        hx_xing_update_info(x, r.frames, head + (int) r.bytes, 50, nullptr, tag, nullptr, nullptr, (unsigned long long) ncalls * 1152, (unsigned) head + r.bytes,
                            16000, 44100, 44100, (unsigned short) r.crc);
        files++;
    }
    hx_xing_destroy(x);
    printf("asan_ledger: %d files ok\n", files);
    return 0;
}
