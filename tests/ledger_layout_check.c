/* ledger_layout_check.c - prints the layout of HX_LEDGER and HX_LEDGER_OPEN as a C compiler sees include/hmp3_amd.h, one
 * "name offset size" line per field and a "sizeof" line per struct; tests/test_ledger_host.py compares it with the ctypes
 * mirror in hmp3_amd/api.py.  Test infrastructure.
 * Build: gcc -I include -o ledger_layout_check tests/ledger_layout_check.c
 */
#include <stddef.h>
#include <stdio.h>
#include "hmp3_amd.h"

#define FIELD(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *) 0)->f))

int main(void)
{
    FIELD(HX_LEDGER, ncalls); FIELD(HX_LEDGER, frames_per_call); FIELD(HX_LEDGER, head_bytes); FIELD(HX_LEDGER, flags);
    FIELD(HX_LEDGER, open); FIELD(HX_LEDGER, ended); FIELD(HX_LEDGER, fed); FIELD(HX_LEDGER, frames); FIELD(HX_LEDGER, bytes);
    FIELD(HX_LEDGER, crc); FIELD(HX_LEDGER, call_bytes); FIELD(HX_LEDGER, toc_counter); FIELD(HX_LEDGER, npt); FIELD(HX_LEDGER, every);
    FIELD(HX_LEDGER, pad0); FIELD(HX_LEDGER, pt); FIELD(HX_LEDGER, pad1);
    printf("sizeof HX_LEDGER %zu\n", sizeof(HX_LEDGER));
    FIELD(HX_LEDGER_OPEN, ncalls); FIELD(HX_LEDGER_OPEN, head_bytes); FIELD(HX_LEDGER_OPEN, flags); FIELD(HX_LEDGER_OPEN, reserved);
    printf("sizeof HX_LEDGER_OPEN %zu\n", sizeof(HX_LEDGER_OPEN));
    printf("HX_LEDGER_POINTS %d\n", HX_LEDGER_POINTS);
    return 0;
}
