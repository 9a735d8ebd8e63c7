// hx_src.h - host-side sample-format / sample-rate converter in front of the encoder (hx_src.cpp), and the plan that the
// batch's conversion kernel (hx_src.hip) runs from
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
typedef struct hx_src hx_src;
hx_src *hx_src_create(void);
void hx_src_destroy(hx_src *s);
/* Csrc::sr_convert_init (reference srcc.cpp:730): bytes the caller must hold per convert call, 0 = unsupported */
int hx_src_init(hx_src *s, int source, int channels, int bits, int is_float, int target, int target_channels,
                int *encode_cutoff_freq);
/* Csrc::sr_convert (reference srcc.cpp:795): 1152 samples per output channel into yout (fp32 at int16 scale);
   returns the input bytes consumed.  Reads up to 1152 * (source / target + 1) sample frames from xin. */
int hx_src_convert(hx_src *s, const unsigned char *xin, float *yout, int *out_bytes);
/* input bytes each of the next nframes calls of a converter that has made `calls` calls consumes (in_bytes may be NULL);
   returns the bytes those calls read, counted from the first unconsumed byte.  Integer only, changes nothing. */
long long hx_src_schedule(const hx_src *s, long long calls, int nframes, long long *in_bytes);

// The converter's plan as the conversion kernel takes it: what hx_src_init derived (case, layout, source format, the
// main stage's n m k ntaps and filter bank, stage 1's n1 m1 and fractions), nothing re-derived.
#define HX_SRC_COEF 1280
#define HX_SRC_COEF1 21
#define HX_SRC_STATUS_WINDOW 8     // status bit: a call's window exceeded the plan's bound (its output was not written)
#define HX_SRC_CARRY 192        // case 4: intermediate samples carried per channel (at most 128 + ntaps are read again)
typedef struct {
    int ncase, layout, channels, bits, is_float, nch;       // nch: output channels
    int n, m, k, ntaps, totcoef, n1, m1;
    int xwin, zwin;             // largest input window / intermediate window of one call, in sample frames
    int cmax;                   // most input sample frames one call consumes
    float coef1[HX_SRC_COEF1];
    float coef[HX_SRC_COEF];
} HxSrcPlan;
// the plan of an initialised converter (0 = not initialised)
int hx_src_plan(const hx_src *s, HxSrcPlan *p);
// hx_src_schedule from a plan
long long hx_src_plan_schedule(const HxSrcPlan *p, long long calls, int nframes, long long *in_bytes);

// arguments of the conversion kernel k_src (hx_src.hip)
struct SrcArgs {
    const unsigned char *in;            // [S][in_stride] bytes
    long long in_stride;
    const long long *off;               // [S][nframes] byte offset of each call's input in the row, or null: consecutive
    const HxSrcPlan *plan;
    const int *cls;                     // stream -> plan
    const long long *calls_in;          // [S] calls the stream's converter has made
    long long *calls_out;
    const float *carry_in;              // [S][2][HX_SRC_CARRY] case 4: the last intermediate samples formed, per channel
    float *carry_out;
    float *out;                         // [S][nframes * 1152 * nch] fp32 at int16 scale: a stream of plan->nch < nch channels fills the start of its row
    const int *nfr;                     // [S] the calls each stream makes of the launch's nframes, or null: all of them
    int nframes, nch, xwin, zwin;       // xwin / zwin: sample frames of the input / intermediate samples per call, at most
    int zoff, coff;                     // LDS floats before the intermediate samples / before the filter bank
    int *status;                        // the batch's status word (HX_SRC_STATUS_WINDOW)
};

// Closed forms of the converter's phase (64-bit; shared by the host schedule and the kernel).  Output sample i (since init)
// follows w(i) = floor(i m / n) steps of the bank: its input position is u(i) = k i + w(i) (case 4: its position among the
// intermediate samples).  Case 4 refills 128 intermediate samples at a time, so after output i it has formed
// Q(i) = 128 ceil((u(i) + ntaps) / 128) of them; intermediate sample q reads input J(q) = floor(q m1 / n1) and J(q) + 1.
#if defined(__HIPCC__)
#define HX_SRC_HD __host__ __device__ static inline
#else
#define HX_SRC_HD static inline
#endif
HX_SRC_HD long long hx_src_u(const HxSrcPlan *p, long long i) { return (long long) p->k * i + i * p->m / p->n; }
HX_SRC_HD long long hx_src_j(const HxSrcPlan *p, long long q) { return q * p->m1 / p->n1; }
// intermediate samples formed before call c (case 4)
HX_SRC_HD long long hx_src_qstart(const HxSrcPlan *p, long long c)
{
    return c <= 0 ? 0 : 128 * ((hx_src_u(p, 1152 * c - 1) + p->ntaps + 127) / 128);
}
// input sample frames calls [c0, c1) consume together (the per-call sums telescope)
HX_SRC_HD long long hx_src_consumed(const HxSrcPlan *p, long long c0, long long c1)
{
    switch (p->ncase) {
    case 0: return 1152 * (c1 - c0);
    case 1: return 576 * (c1 - c0);
    case 2: case 3: return hx_src_u(p, 1152 * c1) - hx_src_u(p, 1152 * c0);
    default: return hx_src_j(p, hx_src_qstart(p, c1)) - hx_src_j(p, hx_src_qstart(p, c0));
    }
}
// input sample frames call c consumes and reads (from its first input sample)
HX_SRC_HD void hx_src_call_extent(const HxSrcPlan *p, long long c, long long *consumed, long long *read)
{
    long long used, rd;
    switch (p->ncase) {
    case 0: used = rd = 1152; break;
    case 1: used = 576; rd = 577; break;
    case 2: used = hx_src_u(p, 1152 * (c + 1)) - hx_src_u(p, 1152 * c); rd = used + 2; break;
    case 3: used = hx_src_u(p, 1152 * (c + 1)) - hx_src_u(p, 1152 * c); rd = hx_src_u(p, 1152 * c + 1151) - hx_src_u(p, 1152 * c) + p->ntaps; break;
    default: used = hx_src_j(p, hx_src_qstart(p, c + 1)) - hx_src_j(p, hx_src_qstart(p, c)); rd = used + 2; break;
    }
    *consumed = used;
    *read = rd;
}
#ifdef __cplusplus
}
#endif
