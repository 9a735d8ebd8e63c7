// hx_spec.hip - front-end kernels from the subband samples to the spectrum (batched MP3 encoder for MI355X, gfx950):
//   k_spec       K4  window + 18-point (3 x 6-point) MDCT + alias butterflies (hwin.c:147-322,
//                    emdct.c:104-288), MDCT-energy psy model (emap.c:61-96, spdsmr.c:64-273) and the
//                    L/R vs M/S metric (bitallo3.cpp:682-742, bitallos.cpp:377-416), one wave per granule
//   k_msscan     K5a the frames' stereo decisions: hysteresis scan over a stream's granules (bitallo3.cpp:693-751)
//                    (k_msscan also rolls the 3-granule subband carry and the PCM history into the next call)
// Parallel over streams x granules (x subbands / partitions).  Each lane
// evaluates its unit with the reference's operation order, so results are bit-identical.
// Built with LLVM's iterative-ilp scheduling strategy, which suits the long straight-line arithmetic: hx_units.tab.
#include "hx_dev.h"

// ---- MDCT kernels ------------------------------------------------------------------------------------
// An N-point kernel (N = 18 for long blocks, 6 for each short window) maps the folded, windowed input f to
// N spectral lines in three steps:
//   1. twiddle and pair the inputs:  g_i = pre[i] f[i];  s_i = g_i + g_{N-1-i};  d_i = odd[i] (g_i - g_{N-1-i})
//   2. an N/2-point cosine transform C of each half:  S = C(s),  D = C(d)
//   3. un-twist:  T_0 = D_0, T_k = D_k - T_{k-1};  y = (S_0, T_0, S_1, T_1, ...) with every element after the
//      first reduced by its finished predecessor.
// The cosine transforms are written out below; sums run left to right.  Operation order equals the
// reference's (emdct.c:104-303), hence bit-identical spectra.

// ((c0 v0 + c1 v1) + c2 v2) + c3 v3
__device__ __forceinline__ float dot4(const float *c, const float *v) { return c[0] * v[0] + c[1] * v[1] + c[2] * v[2] + c[3] * v[3]; }

struct Cos9 {       // 9-point: the input is folded once more into 5 sums (-> even outputs) and 4 differences (-> odd)
    static constexpr int n = 9;
    static __device__ __forceinline__ void run(const HxParams *p, const float *u, float *X)
    {
        float e[4], o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { e[q] = u[q] + u[8 - q]; o[q] = u[q] - u[8 - q]; }
        const float mid = u[4];
        X[0] = 0.5f * (e[0] + e[1] + e[2] + e[3] + mid);
        X[6] = 0.5f * (e[0] + e[2] + e[3]) - e[1] - mid;
        X[3] = p->dct9_k3 * (o[0] - o[2] - o[3]);
        X[2] = dot4(p->dct9_even[0], e) - mid;
        X[4] = dot4(p->dct9_even[1], e) + mid;
        X[8] = dot4(p->dct9_even[2], e) + mid;
        X[1] = dot4(p->dct9_odd[0], o);
        X[5] = dot4(p->dct9_odd[1], o);
        X[7] = dot4(p->dct9_odd[2], o);
    }
};

struct Cos3 {       // 3-point
    static constexpr int n = 3;
    static __device__ __forceinline__ void run(const HxParams *p, const float *u, float *X)
    {
        const float e = u[0] + u[2];
        X[0] = e + u[1];
        X[1] = p->dct3_k * (u[0] - u[2]);
        X[2] = e - u[1] - u[1];
    }
};

template <class Cos>
__device__ __forceinline__ void mdct_kernel(const HxParams *p, const float *pre, const float *odd, const float *f, float *y)
{
    constexpr int H = Cos::n, N = 2 * H;
    float s[H], d[H], S[H], D[H];
#pragma unroll
    for (int i = 0; i < H; i++) {
        const float lo = pre[i] * f[i], hi = pre[N - 1 - i] * f[N - 1 - i];
        s[i] = lo + hi;
        d[i] = odd[i] * (lo - hi);
    }
    Cos::run(p, s, S);
    Cos::run(p, d, D);
    float twist = D[0];
    y[0] = S[0];
    y[1] = twist - y[0];
#pragma unroll
    for (int k = 1; k < H; k++) {
        twist = D[k] - twist;
        y[2 * k] = S[k] - y[2 * k - 1];
        y[2 * k + 1] = twist - y[2 * k];
    }
}

// ---------------------------------------------------------------------------------------
// K4: hybrid MDCT + psychoacoustic model + M/S metric of one (stream, granule), one wavefront.
// The two subband blocks the transform needs (both channels) are fetched with coalesced 16-byte
// loads into LDS; the spectrum goes back to global memory the same way and stays in LDS for the
// psy model (lane = partition, channel after channel) and the M/S metric (lane = sfb), which
// therefore never re-read it from HBM.
//
// MDCT: lane = subband of channel lane >> 5.  Frequency inversion (hwin.c:282) is applied while
// reading, so the stored subband samples stay un-inverted; the alias butterflies exchange 8
// values with each neighbour lane.

// (hand-overs inside a wave take HX_WAVE_SYNC(), hx_dev.h: no workgroup barrier, no s_waitcnt)

// The lookup tables every psy / metric step gathers from (mB logarithm, mB exponential): staged in LDS once per
// workgroup.  Gathers from global memory queue behind the kernel's own streaming loads and stores in the vector
// memory path - a dozen dependent ones per channel were three quarters of this kernel's time.
struct SpecTabs { int mblog[256]; float mbexp_lo[256], mbexp_hi[256]; };

// Psychoacoustic model of a short granule's channel (reference emap.c:61-93, spdsmr.c:64-107): per-window partition
// energies, then mask[w][sfb] = spread(2 sfb partitions); pre-echo control happens in the allocator.  x = the
// channel's 576 lines (LDS); thr gets mask[12*w + sfb], etab zeros.  Short granules are rare: table reads from global memory.
// The function is out of line, so its pointers carry their address spaces: x and es are LDS, the rest global memory.  As
// generic pointers they compiled to FLAT loads and stores, and the wave-local hand-overs here (HX_WAVE_SYNC: no s_waitcnt,
// DS instructions execute in issue order) promise nothing about FLAT accesses that land in LDS.  tools/check_lds_flat.py
// fails the build check if a FLAT instruction reappears in a front-end or packing function.
__device__ __noinline__ void psy_short(const HX_LDS float *x, const HX_GLB HxParams *p, HX_GLB float *etab_out, HX_GLB float *thr_out, HX_LDS float (*es)[64])
{
    const int lane = threadIdx.x & 63;
    const HX_GLB HxPsyTab *ps = &p->psyS;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (lane < ps->npart_e) {
        int i0 = ps->pstart[lane], n = ps->nsum[lane];
        for (int k = 0; k < n; k++) {
            s0 += x[i0 + k] * x[i0 + k];
            s1 += x[192 + i0 + k] * x[192 + i0 + k];
            s2 += x[384 + i0 + k] * x[384 + i0 + k];
        }
    }
    es[0][lane] = s0; es[1][lane] = s1; es[2][lane] = s2;
    HX_WAVE_SYNC();
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if (lane < 12 && 2 * lane < ps->npart) {
        float a[3] = {0.5f, 0.5f, 0.5f}, b[3] = {0.5f, 0.5f, 0.5f};
        int i = 2 * lane, q = ps->off[i], n = ps->cnt[i], r = ps->row[i];
        for (int j = 0; j < n; j++)
            for (int w = 0; w < 3; w++) a[w] += ps->w[r + j] * es[w][q + j];
        q = ps->off[i + 1]; n = ps->cnt[i + 1]; r = ps->row[i + 1];
        for (int j = 0; j < n; j++)
            for (int w = 0; w < 3; w++) b[w] += ps->w[r + j] * es[w][q + j];
        m0 = a[0] + b[0]; m1 = a[1] + b[1]; m2 = a[2] + b[2];
    }
    etab_out[lane] = 0.0f;
    // thr layout for short granules: [12*w + sfb]
    if (lane < 12) { thr_out[lane] = m0; thr_out[12 + lane] = m1; thr_out[24 + lane] = m2; }
    else if (lane >= 36) thr_out[lane] = 0.0f;
    HX_WAVE_SYNC();
}

// Psychoacoustic model of a long granule, both channels in one pass (lane = partition): partition energies, spreading
// (reference emap.c / spdsmr.c:185-262), signal-to-noise statistics and the threshold scale.  The lane's table entries
// (pc: first line, lines, spreading row start / length / first source, absolute threshold) were read at the start of
// the kernel; the spreading weights of a row, the same for both channels, are read once for the two and eight at a
// time; per channel the order of operations is the reference's.  Outputs etab (energy + absolute threshold) and
// thr = a * stab (threshold before pre-echo control).
struct PsyLane { int i0, nsum, off, cnt, row; float wabs; };
__device__ __forceinline__ void psy_long2(const float *xl, const HxParams *p, const SpecTabs &T, const PsyLane &pc,
                                          float *etab_out, float *thr_out, float (*xtab)[64])
{
    const int lane = threadIdx.x & 63;
    const HxPsyTab *pt = &p->psyL;
    const float *w = pt->w;
    const float alpha = 0.30f;
    const int npart = pt->npart, npart2 = (npart + 1) & (~1);
    float e[2] = {0.0f, 0.0f};
    if (lane < pt->npart_e) {
        float s0 = 0.0f, s1 = 0.0f;
        const float *xa = xl + pc.i0, *xb = xl + 576 + pc.i0;
        for (int k = 0; k < pc.nsum; k++) { s0 += xa[k] * xa[k]; s1 += xb[k] * xb[k]; }
        e[0] = s0; e[1] = s1;
    }
    float et[2] = {0.0f, 0.0f};
    int mbe[2] = {0, 0};
    if (lane < npart2) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            et[c] = pc.wabs + e[c];
            mbe[c] = hx_mblog(T.mblog, et[c]);
            xtab[c][lane] = hx_mbexp(T.mbexp_lo, T.mbexp_hi, (int) (alpha * mbe[c]));
        }
    }
    HX_WAVE_SYNC();
    float sacc[2] = {0.1f, 0.1f};
    if (lane < npart) {
        const float *wr = w + pc.row, *xa = xtab[0] + pc.off, *xb = xtab[1] + pc.off;
        const int n = pc.cnt;
        // 16 weights per round, four 16-byte reads in flight (rows start at any word; what a read takes in beyond the
        // row's end - the next row, or past the table the struct's following members - is not used)
        for (int j0 = 0; j0 < n; j0 += 16) {
            typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
            float wv[16];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const f4u t = *reinterpret_cast<const f4u *>(wr + j0 + 4 * u);
                wv[4 * u] = t.x; wv[4 * u + 1] = t.y; wv[4 * u + 2] = t.z; wv[4 * u + 3] = t.w;
            }
#pragma unroll
            for (int u = 0; u < 16; u++) if (j0 + u < n) { sacc[0] += wv[u] * xa[j0 + u]; sacc[1] += wv[u] * xb[j0 + u]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        float stab = 0.0f;
        int snr = 0;
        if (lane < npart) {
            const float sa = (0.03f * 0.1f * 0.35f) * hx_mbexp(T.mbexp_lo, T.mbexp_hi, (int) ((1.0f / alpha) * hx_mblog(T.mblog, sacc[c]))) + pc.wabs;
            stab = sa;
            snr = mbe[c] - hx_mblog(T.mblog, pc.wabs + sa);
        }
        int prev = __shfl_up(snr, 1, 64);
        if (lane == 0) prev = 0;
        const bool in = lane < npart;
        int nsnr = hx_wave_sum((in && snr > 0) ? 1 : 0);
        int totsnr = hx_wave_sum(in ? max(-200, snr) : 0);
        int snrvar = hx_wave_sum(in ? abs(snr - prev) : 0);
        int d = 0;
        if (nsnr > 0) {
            int d0 = hx_round(1.3f * (totsnr / npart) - 850);
            int itmp = snrvar / npart;
            int dv = min(500 - itmp, 0);
            d = d0 + dv;
            d = max(d, -2000);
            d = min(d, 600);
        }
        d += 300;
        int dm0 = (300 - d) >> 4;
        int m = lane >> 1;
        int dm = max(dm0 * max(m - 13, 0), 0);
        float a = hx_mbexp(T.mbexp_lo, T.mbexp_hi, d + dm);
        etab_out[64 * c + lane] = (lane < npart2) ? et[c] : 0.0f;
        thr_out[64 * c + lane] = (lane < npart2) ? a * stab : 0.0f;
    }
    HX_WAVE_SYNC();
}

// M/S decision metric before hysteresis: lane = scalefactor band (reference bitallo3.cpp:695-742);
// x0 / x1 = the two channels' lines (LDS)
__device__ __forceinline__ void msmetric_unit(const float *x0, const float *x1, const HxParams *p, const int *t_mblog,
                                              int *out, bool is_short, int sb_start, int sb_n, unsigned run_word, int band_last)
{
    const int lane = threadIdx.x & 63;
    int v = 0;
    if (is_short) {         // short block (reference bitallos.cpp:377-416): lane = (window, sfb)
        const int w = lane >> 4, i = lane & 15;
        int d = 0;
        if (w < 3 && i < p->nsfs) {
            int k = 192 * w + p->startBand_s[i], n = p->nBand_s[i];
            float s0 = 0.0f, s1 = 0.0f;
            for (int j = 0; j < n; j++, k++) {
                float a = x0[k] * x0[k], b = x1[k] * x1[k];
                s0 += (a + b);
                a = fabsf(a - b);
                s1 += a;
            }
            if ((double) s1 > 0.80 * (double) s0) d++;
            if ((double) s1 > 0.95 * (double) s0) d += 2;
        }
        d = hx_wave_sum(d);
        if (lane == 0) *out = (p->nsfs - d) << 10;
        return;
    }
    if (p->alloc1) {        // the first-generation allocator's measure (reference bitallo1.cpp:385-431): bands where one channel dominates count against M/S
        int d = 0;
        if (lane < p->nsf[0]) {
            int k = p->startBand_l[lane], n = p->nBand_l[lane];
            float s0 = 0.0f, s1 = 0.0f;
            for (int j = 0; j < n; j++, k++) {
                float a = x0[k] * x0[k], b = x1[k] * x1[k];
                s0 += (a + b);
                a = fabsf(a - b);
                s1 += a;
            }
            if ((double) s1 > 0.80 * (double) s0) d++;
            if ((double) s1 > 0.95 * (double) s0) d += 2;
        }
        d = hx_wave_sum(d);
        if (lane == 0) *out = p->nsf[0] - 3 * d;
        return;
    }
    // The band's three sums - el = 100 + sum l^2, er = 100 + sum r^2 and the signed t = sum l r, each in line order in the
    // reference - feed four mbLogC arguments only: el + er, max(el, er), es + ed and max(es, ed) (es, ed = (el + er) +- 2 t).
    // So the lanes add the terms of their line runs (the runs of the stream walk's certified band sums, HxParams::lane_run),
    // a segmented scan brings the band's totals to its last lane, and the band lane certifies the four buckets from the
    // intervals the strict sums must lie in (hx_dev.h; the signed sum's half-width comes from sum |l r|); it runs the strict
    // loop only when an interval straddles a bucket boundary (about one band in a hundred).  Before, a wave paid for the widest
    // band's 76 iterations with a third of its lanes in the loop: a third of this kernel's instructions.
    // (tests/cert_sums_check.c checks the certificates on correlated channel pairs of every kind.)
    const bool bandlane = lane < p->nsf[0];
    bool strict = bandlane;
    int mblr = 0, mbsd = 0;
    if (p->ms_flag) {
        const int W = p->run_w;
        const int start = (int) (run_word & 511u) << 1, cnt = (int) ((run_word >> 9) & 7u) << 1, d = (int) (run_word >> 12);
        float sa = 0.0f, sb = 0.0f, sc = 0.0f, sm = 0.0f;
#pragma unroll
        for (int k = 0; k < 10; k += 2) {
            if (k < W) {
                const float2 l = *reinterpret_cast<const float2 *>(x0 + start + k), r = *reinterpret_cast<const float2 *>(x1 + start + k);
                const bool in = k < cnt;
                const float a0 = in ? l.x * l.x : 0.0f, a1 = in ? l.y * l.y : 0.0f, b0 = in ? r.x * r.x : 0.0f, b1 = in ? r.y * r.y : 0.0f;
                const float c0 = in ? l.x * r.x : 0.0f, c1 = in ? l.y * r.y : 0.0f;
                sa += (a0 + a1); sb += (b0 + b1); sc += (c0 + c1); sm += (fabsf(c0) + fabsf(c1));
            }
        }
        const int last4 = 4 * band_last;
        const float SA = hx_lane_read(last4, hx_seg_scan(sa, d, lane)), SB = hx_lane_read(last4, hx_seg_scan(sb, d, lane));
        const float SC = hx_lane_read(last4, hx_seg_scan(sc, d, lane)), SM = hx_lane_read(last4, hx_seg_scan(sm, d, lane));
        if (bandlane) {
            const float du = hx_cert_delta(sb_n + 1, W);      // (the 100 in front is one more term and one more addition)
            const float tel = 100.0f + SA, ter = 100.0f + SB;
            const float e1 = tel * du, e2 = ter * du, e3 = SM * du;
            // (a sum of non-negative terms that starts at 100 never falls below 100: rounding is monotone)
            const float el_lo = fmaxf(tel - e1, 100.0f), el_hi = tel + e1, er_lo = fmaxf(ter - e2, 100.0f), er_hi = ter + e2;
            const float t_lo = SC - e3, t_hi = SC + e3;
            const float tl2 = t_lo + t_lo, th2 = t_hi + t_hi;
            const float p1_lo = el_lo + er_lo, p1_hi = el_hi + er_hi;
            const float p2_lo = fmaxf(el_lo, er_lo), p2_hi = fmaxf(el_hi, er_hi);
            const float es_lo = p1_lo + tl2, es_hi = p1_hi + th2, ed_lo = p1_lo - th2, ed_hi = p1_hi - tl2;
            const float p3_lo = es_lo + ed_lo, p3_hi = es_hi + ed_hi;
            // (one of es, ed is el + er plus something non-negative, rounded: max(es, ed) >= el + er)
            const float p4_lo = fmaxf(fmaxf(es_lo, ed_lo), p1_lo), p4_hi = fmaxf(es_hi, ed_hi);
            const bool ok = p3_lo > 0.0f && p4_lo > 0.0f && (hx_f2bits(p1_lo) >> 15) == (hx_f2bits(p1_hi) >> 15) && (hx_f2bits(p2_lo) >> 15) == (hx_f2bits(p2_hi) >> 15)
                            && (hx_f2bits(p3_lo) >> 15) == (hx_f2bits(p3_hi) >> 15) && (hx_f2bits(p4_lo) >> 15) == (hx_f2bits(p4_hi) >> 15);
            if (ok) {       // every point of a certified interval has the strict value's log: take the lower ends
                strict = false;
                mblr = hx_mblog(t_mblog, p1_lo) - hx_mblog(t_mblog, p2_lo);
                mbsd = hx_mblog(t_mblog, p3_lo) - hx_mblog(t_mblog, p4_lo);
            }
        }
    }
    if (strict) {
        int k = sb_start;
        float el = 100.0f, er = 100.0f, t = 0.0f;
        for (int j = 0; j < sb_n; j++, k++) {
            float a = x0[k] * x0[k], b = x1[k] * x1[k], c = x0[k] * x1[k];
            el += a; er += b; t += c;
        }
        float es, ed;
        es = ed = el + er;
        t = t + t;
        es = es + t;
        ed = ed - t;
        mblr = hx_mblog(t_mblog, el + er) - hx_mblog(t_mblog, el > er ? el : er);
        mbsd = hx_mblog(t_mblog, es + ed) - hx_mblog(t_mblog, es > ed ? es : ed);
    }
    if (bandlane) {
        int psd = max(75 - abs(mblr - 120), 0);
        mbsd = min(mbsd, (mbsd >> 1) + 120);
        mbsd += psd;
        v = sb_n * (mblr - mbsd);
    }
    v = hx_wave_sum(v);
    if (lane == 0) *out = v;
}

// DIRECT = false: the granule's subband samples are staged in LDS by 16-byte loads and picked up from there (24 KB of LDS per
// workgroup); DIRECT = true: every lane loads its own 2 x 18 samples from global memory (8-byte loads; 14.8 KB).  Measured
// (EXPERIMENTS.md, round 4): alone on the chip the direct form is 11 % faster (configs 3 - 5, where the stream walk's
// low-footprint kernel leaves the front end no room beside it: +3.6 / +2.7 % per step); beside the resident stream walk of
// config 2 it is 0.7 % slower per step - more of its smaller workgroups fit next to the walk's waves and take issue slots
// from them.  hx_batch.hip launches the form that goes with the stream-walk kernel it chose.
template <bool DIRECT>
__device__ __forceinline__ void spec_granule(const float *__restrict__ sb, const HxStream *__restrict__ st,
                                             const HxParams *__restrict__ prm, const HxGlobalTabs *__restrict__ gt,
                                             const unsigned char *__restrict__ bt,
                                             float *__restrict__ xr, float *__restrict__ etab_out, float *__restrict__ thr_out,
                                             int *__restrict__ msbase, int NG, int SG, const int *__restrict__ nfr)
{
    // in: [ch][S[g-3] | S[g-2]][576] subband samples; the first 2 x 576 floats are reused as the
    // spectrum [ch][576] once every lane holds its inputs in registers (DIRECT: the spectrum only)
    // two granules per workgroup, one wavefront each, independent of each other but for the lookup tables they share
    __shared__ __attribute__((aligned(16))) float in_s[2][DIRECT ? 1 : 2][2][576];
    __shared__ float xtab_s[2][2][64];
    __shared__ float es_s[2][3][64];
    __shared__ SpecTabs T;
    // (the wave index is wave-uniform, which the compiler cannot see in threadIdx: through readfirstlane the granule's
    // addresses are scalar arithmetic)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sbnd = lane & 31, ch = lane >> 5;
    for (int i = threadIdx.x; i < 256; i += 128) { T.mblog[i] = gt->mblog[i]; T.mbexp_lo[i] = gt->mbexp_lo[i]; T.mbexp_hi[i] = gt->mbexp_hi[i]; }
    // Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own; neighbouring granules share a subband
    // block, so every XCD gets a contiguous piece of the grid: workgroups b and b + 8, launched together on one XCD, are
    // neighbours in the stream, and the second read of the shared block hits that L2 (speed only: any placement is correct)
    const unsigned nwg = gridDim.x, cpx = nwg >> 3;
    const unsigned wg = (blockIdx.x < (cpx << 3)) ? (blockIdx.x & 7) * cpx + (blockIdx.x >> 3) : blockIdx.x;
    const long long sg = (long long) wg * 2 + wv;                   // (s, g); S * NG is even
    const int g = (int) (sg % NG), s = (int) (sg / NG);
    const HxParams *p = prm + __builtin_amdgcn_readfirstlane(st[s].cls);      // wave-uniform: table reads become scalar loads
    float (*in)[2][576] = in_s[wv];
    // this lane's entries of the psy and band tables: requested now, needed after the transform
    PsyLane pc;
    pc.i0 = p->psyL.pstart[lane]; pc.nsum = p->psyL.nsum[lane]; pc.off = p->psyL.off[lane]; pc.cnt = p->psyL.cnt[lane];
    pc.row = p->psyL.row[lane]; pc.wabs = p->psyL.w[lane];
    const int sb_start = p->startBand_l[min(lane, 22)], sb_n = p->nBand_l[min(lane, 21)];
    const unsigned run_word = p->lane_run[lane];            // the lane's line run and its band's last lane, for the stereo metric's sums
    const int band_last = p->band_last_lane[min(lane, 21)];
    __syncthreads();        // the tables (the only workgroup barrier: from here on each wave is on its own)
    if (nfr && g >= 2 * nfr[s]) return;         // beyond the stream's count (the two waves may be of different streams: behind the barrier)
    const int nsb = p->nsb_ms0;
    const int btype = bt[sg];
    float g1[DIRECT ? 18 : 1], g2[DIRECT ? 18 : 1];
    const float *x1, *x2;
    if constexpr (DIRECT) {
        // every lane takes its subband's 18 + 18 samples straight from global memory (72 contiguous bytes per block, 8-byte
        // aligned; the wave's 64 lanes cover two contiguous 2304-byte runs per channel)
        const float2 *b1 = reinterpret_cast<const float2 *>(sb + ((long long) (s * 2 + ch) * SG + g) * 576 + sbnd * 18);
        const float2 *b2 = b1 + 288;
#pragma unroll
        for (int i = 0; i < 9; i++) { const float2 a = b1[i], b = b2[i]; g1[2 * i] = a.x; g1[2 * i + 1] = a.y; g2[2 * i] = b.x; g2[2 * i + 1] = b.y; }
        x1 = g1; x2 = g2;
    } else {
        {   // 2 x 1152 contiguous floats per channel, 16 bytes per lane and load
            float4 v[9];
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const int e = lane + 64 * k, c = e / 288, r = e - 288 * c;       // 288 float4 per channel
                v[k] = reinterpret_cast<const float4 *>(sb + ((long long) (s * 2 + c) * SG + g) * 576)[r];
            }
#pragma unroll
            for (int k = 0; k < 9; k++) reinterpret_cast<float4 *>(&in[0][0][0])[lane + 64 * k] = v[k];
        }
        HX_WAVE_SYNC();
        x1 = &in[ch][0][sbnd * 18];                    // S[g-3]
        x2 = &in[ch][1][sbnd * 18];                    // S[g-2]
    }
    float y[18], f[18];
    const bool act = sbnd < nsb;
    {
        float p1[18], p2[18];
        const bool inv = (sbnd & 1) != 0;       // odd subbands: negate odd time slots
#pragma unroll
        for (int i = 0; i < 18; i++) {
            float a = x1[i], b = x2[i];
            if (inv && (i & 1)) { a = -a; b = -b; }
            p1[i] = a; p2[i] = b;
        }
        HX_WAVE_SYNC();                         // everyone has its inputs: `in` may be overwritten
        if (!act) {
#pragma unroll
            for (int i = 0; i < 18; i++) y[i] = 0.0f;
        } else if (btype != 2) {
            const float *w = p->win[btype];
#pragma unroll
            for (int j = 0; j < 9; j++) {
                f[j] = w[26 - j] * p2[8 - j] + w[27 + j] * p2[9 + j];
                f[9 + j] = w[j] * p1[j] + w[17 - j] * p1[17 - j];
            }
            mdct_kernel<Cos9>(p, p->mdct_pre18, p->mdct_odd18, f, y);
        } else {        // short: three overlapping 12-tap windows (reference hwin.c:228-278)
            const float *w = p->win[2];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                f[q] = w[8 - q] * p1[14 - q] + w[9 + q] * p1[15 + q];
                f[3 + q] = w[q] * p1[6 + q] + w[5 - q] * p1[11 - q];
                f[6 + q] = w[8 - q] * p2[2 - q] + w[9 + q] * p2[3 + q];
                f[9 + q] = w[q] * p1[12 + q] + w[5 - q] * p1[17 - q];
                f[12 + q] = w[8 - q] * p2[8 - q] + w[9 + q] * p2[9 + q];
                f[15 + q] = w[q] * p2[q] + w[5 - q] * p2[5 - q];
            }
#pragma unroll
            for (int w = 0; w < 3; w++) mdct_kernel<Cos3>(p, p->mdct_pre6, p->mdct_odd6, f + 6 * w, y + 6 * w);
        }
    }
    // alias reduction between subband k (lane) and k+1: x[17-i] with next lane's x[i]
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float up = __shfl_down(y[i], 1, 64);            // next subband's element i
        float dn = __shfl_up(y[17 - i], 1, 64);         // previous subband's element 17-i
        float cs = p->csa[0][i], ca = p->csa[1][i];
        float a = y[17 - i], b = y[i];
        float na = a, nb = b;
        if (btype != 2) {                                   // no alias reduction on short blocks
            if (sbnd < nsb - 1) na = a * cs + up * ca;      // upper edge of this band
            else if (sbnd == nsb - 1) na = a * cs;          // last coded band: half butterfly
            if (sbnd >= 1 && sbnd < nsb) nb = b * cs - dn * ca;     // lower edge (pairs with band-1)
        }
        y[17 - i] = na;
        y[i] = nb;
    }
    float *xl = &in[0][0][0];                   // spectrum [ch][576]
    if (btype != 2) {
        float *o = xl + ch * 576 + sbnd * 18;
#pragma unroll
        for (int i = 0; i < 18; i++) o[i] = y[i];
    } else {                                    // [3 windows][192], line = 6*sb + k
        float *o = xl + ch * 576 + sbnd * 6;
#pragma unroll
        for (int w = 0; w < 3; w++)
#pragma unroll
            for (int k = 0; k < 6; k++) o[192 * w + k] = y[6 * w + k];
    }
    HX_WAVE_SYNC();
    {   // spectrum to global memory, 16 bytes per lane and store
        float4 *dst = reinterpret_cast<float4 *>(xr + sg * 1152);
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int e = lane + 64 * k;
            typedef float f4v __attribute__((ext_vector_type(4)));
            if (e < 288) __builtin_nontemporal_store(reinterpret_cast<const f4v *>(xl)[e], reinterpret_cast<f4v *>(dst) + e);     // read once, a kernel later
        }
    }
    if (btype != 2) psy_long2(xl, p, T, pc, etab_out + sg * 128, thr_out + sg * 128, xtab_s[wv]);
    else {
        const HX_LDS float *xs = (const HX_LDS float *) xl;
        HX_LDS float (*ess)[64] = (HX_LDS float (*)[64]) es_s[wv];
        const HX_GLB HxParams *pg = (const HX_GLB HxParams *) p;
        psy_short(xs, pg, (HX_GLB float *) (etab_out + sg * 128), (HX_GLB float *) (thr_out + sg * 128), ess);
        psy_short(xs + 576, pg, (HX_GLB float *) (etab_out + sg * 128 + 64), (HX_GLB float *) (thr_out + sg * 128 + 64), ess);
    }
    msmetric_unit(xl, xl + 576, p, T.mblog, msbase + sg, btype == 2, sb_start, sb_n, run_word, band_last);
}

#define HX_K4(name, direct) \
__global__ __launch_bounds__(128) void name(const float *__restrict__ sb, const HxStream *__restrict__ st, const HxParams *__restrict__ prm, \
                                           const HxGlobalTabs *__restrict__ gt, const unsigned char *__restrict__ bt, float *__restrict__ xr, \
                                           float *__restrict__ etab_out, float *__restrict__ thr_out, int *__restrict__ msbase, int NG, int SG, \
                                           const int *__restrict__ nfr) \
{ spec_granule<direct>(sb, st, prm, gt, bt, xr, etab_out, thr_out, msbase, NG, SG, nfr); }
HX_K4(k_spec, false)
HX_K4(k_spec_direct, true)

// K5a: the frame's stereo decision (joint-stereo streams), serial per stream over its granules, and the hand-over
// of the pre-echo memory between calls.  The L/R-vs-M/S metric of a granule gets a +-5000 hysteresis from the
// previous long granule; a short granule takes none and clears it (reference bitallo3.cpp:693-698,743-751); an
// MPEG-1 frame is coded M/S when its two granules' values sum to >= 0 (mp3enc.cpp:1538-1546), an MPEG-2 frame by
// its one granule.  Depends on front-end data only, so it runs here and not in the per-stream allocator walk.
// (Round 6: the kernel also rolls the stream's carries - the last three granules of subband samples to slots 0..2, the last 480
// input samples into the stream state - which was k_carry's launch: k_spec, the last reader of the subband buffer, is through
// when this kernel starts, and 63 of its 64 lanes had nothing to do.)
__global__ __launch_bounds__(64) void k_msscan(HxStream *__restrict__ st, const HxParams *__restrict__ prm, const int *__restrict__ msbase,
                                               const unsigned char *__restrict__ bt, unsigned char *__restrict__ msflag, int *__restrict__ msdec,
                                               const float *__restrict__ thr, float *__restrict__ thrprev, int NG,
                                               float *__restrict__ sb, int SG, const int16_t *__restrict__ pcm, long long nsamp,
                                               const float *__restrict__ pcmf, int pitch, const int *__restrict__ nfr)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    HxStream *ss = st + s;
    const HxParams *p = prm + __builtin_amdgcn_readfirstlane(ss->cls);
    const int nchan = p->nchan;                 // the stream's own channels; pitch: those its PCM row is laid out for
    const int lsf = !p->h_id;                   // ... and its own MPEG version: an MPEG-2 frame is one granule
    const long long g0 = (long long) s * NG;
    // The stream's granules of this call (hx_batch_frame_counts): the bound of the scan, and where the hand-overs to the next
    // call come from - the pre-echo memory from granule NGs - 1, the subband carry from slots NGs .. NGs + 2, the PCM history
    // from the last 480 of its 576 NGs samples.  NG stays the stride of the rows.  A stream that takes no frame keeps all of it.
    const int NGs = nfr ? 2 * nfr[s] : NG;
    if (NGs == 0) return;
    const long long nown = 576LL * NGs;
    if (lane == 0) {
        const int on = p->ms_flag, plain = p->alloc1;    // (the first-generation allocator's measure takes no hysteresis)
        int mem = ss->ms_memory;
        auto frame = [&](int b1, int b2, int v1, int v2, int *m1o, int *m2o) {      // one pair of granules; returns the two flags
            int m1 = 0, m2 = 0;
            if (on) {
                m1 = v1;
                if (plain) { }
                else if (b1 == 2) mem = 0; else { m1 += mem; mem = (m1 > 0) ? 5000 : -5000; }
                m2 = v2;
                if (plain) { }
                else if (b2 == 2) mem = 0; else { m2 += mem; mem = (m2 > 0) ? 5000 : -5000; }
            }
            *m1o = m1; *m2o = m2;
            const unsigned f1 = (on && (lsf ? m1 : m1 + m2) >= 0), f2 = (on && (lsf ? m2 : m1 + m2) >= 0);
            return f1 | (f2 << 8);
        };
        int g = 0;
        // eight granules per round of loads and stores (the rows are 16-byte aligned when NG % 8 == 0)
        if ((NG & 7) == 0)
            for (; g + 8 <= NGs; g += 8) {
                const int4 va = *reinterpret_cast<const int4 *>(msbase + g0 + g), vb = *reinterpret_cast<const int4 *>(msbase + g0 + g + 4);
                const uint2 bb = *reinterpret_cast<const uint2 *>(bt + g0 + g);
                int4 da, db;
                const unsigned fa = frame(bb.x & 255, (bb.x >> 8) & 255, va.x, va.y, &da.x, &da.y);
                const unsigned fb = frame((bb.x >> 16) & 255, bb.x >> 24, va.z, va.w, &da.z, &da.w);
                const unsigned fc = frame(bb.y & 255, (bb.y >> 8) & 255, vb.x, vb.y, &db.x, &db.y);
                const unsigned fd = frame((bb.y >> 16) & 255, bb.y >> 24, vb.z, vb.w, &db.z, &db.w);
                *reinterpret_cast<int4 *>(msdec + g0 + g) = da;
                *reinterpret_cast<int4 *>(msdec + g0 + g + 4) = db;
                *reinterpret_cast<uint2 *>(msflag + g0 + g) = make_uint2(fa | (fb << 16), fc | (fd << 16));
            }
        for (; g < NGs; g += 2) {
            int m1, m2;
            const unsigned f = frame(bt[g0 + g], bt[g0 + g + 1], msbase[g0 + g], msbase[g0 + g + 1], &m1, &m2);
            msdec[g0 + g] = m1; msdec[g0 + g + 1] = m2;
            msflag[g0 + g] = (unsigned char) (f & 1); msflag[g0 + g + 1] = (unsigned char) (f >> 8);
        }
        ss->ms_memory = mem;
    }
    // pre-echo memory ("ecsave", reference spdsmr.c:112-117,283-298): this call's first granule is clamped against
    // the stream's carried values, which then become the doubled unclamped thresholds of this call's last granule
    // (long), or its doubled window-2 sums in entries 0..11 (short)
    const float *last = thr + (g0 + NGs - 1) * 128;
    const int lastbt = bt[g0 + NGs - 1];
    for (int i = lane; i < 128; i += 64) {
        const float old = (&ss->thr_prev[0][0])[i];
        thrprev[(long long) s * 128 + i] = old;
        float nw = old;
        if (lastbt != 2) nw = 2.0f * last[i];
        else if ((i & 63) < 12) nw = 2.0f * last[(i & 64) + 24 + (i & 63)];
        (&ss->thr_prev[0][0])[i] = nw;
    }
    // the carries into the next call
    for (int ch = 0; ch < 2; ch++) {
        float *base = sb + (long long) (s * 2 + ch) * SG * 576;
        for (int e = lane; e < 576; e += 64)
            for (int k = 0; k < 3; k++) base[k * 576 + e] = base[(NGs + k) * 576 + e];
        const int16_t *src = pcm + (long long) s * nsamp * pitch + ch;
        for (int i = lane; i < 480 && ch < nchan; i += 64) {
            const long long n = nown - 480 + i;
            // fewer than 480 new samples never happens (a frame is 1152), so all come from this batch
            ss->pcm_hist[ch][i] = pcmf ? pcmf[(long long) s * nsamp * pitch + n * nchan + ch] : (float) src[nchan * n];
        }
    }
    if (lane == 0) ss->frames_in += NGs / 2;
}
