// hx_count1.hip - the twin of hx_alloc1.hip that holds the test tap k_debug_count_a1 (tests only, hx_debug_count) in the stream walk's
// place: the same sources, macros and flags (HX_TAP, hx_alloc3.inc).
#define HX_TAP 1
#include "hx_alloc1.hip"
