// hx_prep.hip - the last front-end kernel of the batched MP3 encoder for MI355X (gfx950):
//   k_prep       K5b what the allocator's granule start needs that does not depend on its carried state: signs, band
//                    energies, band maxima of x^(3/4), zero-gain steps, masks (bitallo3.cpp:816-1066, spdsmr.c:275-318)
// Each lane evaluates its unit with the reference's operation order, so results are bit-identical.
// Built with LLVM's iterative-ilp scheduling strategy, which suits its long straight-line arithmetic
// (k_prep 1.50 -> 1.36 ms): hx_units.tab.
#include "hx_dev.h"

// K5b: everything the allocator does at the start of a long-block granule that does not depend on its carried
// state, one wavefront per (stream, granule): magnitudes and signs of the lines in the representation the frame
// is coded in (L / R, or M = L + R, S = L - R: reference l3math.c:449-470,905-930), band energies in line order
// (bitallo3.cpp:816-864,902-985), x^(3/4) of every line with the band maxima and the zero-gain steps
// (:878-896, pow34.c:132-186), and the masking thresholds after pre-echo control (spdsmr.c:275-318).  The
// short-block granules are skipped (their allocator starts from the raw spectrum).
#define PREP_GPB 4      // granules (wavefronts) per workgroup: they share one copy of the lookup tables
__global__ __launch_bounds__(64 * PREP_GPB) void k_prep(const float *__restrict__ xr, float *__restrict__ xmag_dbg, float *__restrict__ x34o, unsigned *__restrict__ sgn,
                                             HxBandPrep *__restrict__ band, const HxStream *__restrict__ st,
                                             const HxParams *__restrict__ prm, const HxGlobalTabs *__restrict__ gt,
                                             const unsigned char *__restrict__ bt, const unsigned char *__restrict__ msflag,
                                             const float *__restrict__ etab, const float *__restrict__ thr,
                                             const float *__restrict__ thrprev, int NG, long long nunits, const int *__restrict__ nfr)
{
    // Per wave only the squares that the band lanes add up live in LDS (one pair of channels at a time: L / R, then
    // M / S); magnitudes, x^(3/4) and signs stay in the registers of the lane that owns the lines, from the load
    // to the store.  The gather tables are staged once per workgroup.
    __shared__ __attribute__((aligned(16))) float sq[PREP_GPB][2][576];
    __shared__ int xmax[PREP_GPB][2][22];
    __shared__ float t_exp[256], t_a[16], t_b[16];
    __shared__ int t_mblog[256];
    for (int i = threadIdx.x; i < 256; i += 64 * PREP_GPB) { t_exp[i] = gt->pow34_exp[i]; t_mblog[i] = gt->mblog[i]; }
    if (threadIdx.x < 16) { t_a[threadIdx.x] = gt->pow34_a[threadIdx.x]; t_b[threadIdx.x] = gt->pow34_b[threadIdx.x]; }
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane < 44) xmax[wv][lane / 22][lane % 22] = 0;
    __syncthreads();
    const long long unit = (long long) blockIdx.x * PREP_GPB + wv;      // (s, g)
    if (unit >= nunits) return;
    const int g = (int) (unit % NG), s = (int) (unit / NG);
    if (nfr && g >= 2 * nfr[s]) return;         // beyond the stream's count (behind the barrier: the four waves may be of different streams)
    const int btype = bt[unit];
    if (btype == 2) return;
    // (from here on the wave works alone: LDS hand-overs inside a wave need no workgroup barrier)
    const HxParams *p = prm + __builtin_amdgcn_readfirstlane(st[s].cls);
    if (p->alloc1) return;      // the first-generation allocator starts from the raw spectrum
    const int ms = msflag[unit];
    const int two = p->nchan == 2;
    const int nsf0 = p->nsf[0];
    // lines that get magnitudes / x^(3/4), bands that get energies / maxima (reference: nbmax, nbmax2 / nbmax3 ...)
    const int nl_mag0 = ms ? (p->hf_flag ? p->startBand_l[22] : p->nbmax[0]) : p->nbmax3[0];
    const int nl_mag1 = ms ? nl_mag0 : (two ? p->nbmax3[1] : 0);
    const int nl_p0 = ms ? p->nbmax2[0] : p->nbmax3[0], nl_p1 = two ? (ms ? p->nbmax2[1] : p->nbmax3[1]) : 0;
    const int nb_e0 = ms ? nsf0 : p->nsf3[0], nb_e1 = ms ? nsf0 : (two ? p->nsf3[1] : 0);
    const int nb_z0 = ms ? p->nsf2[0] : p->nsf3[0], nb_z1 = two ? (ms ? p->nsf2[1] : p->nsf3[1]) : 0;
    const float *x = xr + unit * 1152;
    float (*sqw)[576] = sq[wv];
    // lane l owns lines 4 (l + 64 k) .. + 3 of both channels, k = 0..2 (144 groups of four per channel)
    float a0[3][4], a1[3][4];           // magnitudes in the coded representation
    unsigned s0[3], s1[3];              // sign bytes
    {
        float4 lv[3], rv[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int e = min(lane + 64 * k, 143);
            lv[k] = reinterpret_cast<const float4 *>(x)[e];
            rv[k] = reinterpret_cast<const float4 *>(x + 576)[e];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int e = lane + 64 * k;
            const float l4[4] = {lv[k].x, lv[k].y, lv[k].z, lv[k].w}, r4[4] = {rv[k].x, rv[k].y, rv[k].z, rv[k].w};
            float t0[4], t1[4];
            s0[k] = s1[k] = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int j = 4 * e + c;
                const float l = l4[c], r = r4[c];
                a0[k][c] = l; a1[k][c] = r; t0[c] = t1[c] = 0.0f;
                if (ms) {
                    if (j < nl_mag0) {
                        t0[c] = l * l;
                        t1[c] = r * r;
                        float m = (l + r), d = (l - r);
                        if (m < 0.0f) { s0[k] |= 1u << (8 * c); m = -m; }
                        if (d < 0.0f) { s1[k] |= 1u << (8 * c); d = -d; }
                        a0[k][c] = m; a1[k][c] = d;
                    }
                } else {
                    if (j < nl_mag0) { float v = l; if (!(v >= 0.0f)) { s0[k] |= 1u << (8 * c); v = -v; } a0[k][c] = v; t0[c] = v * v; }
                    if (j < nl_mag1) { float v = r; if (!(v >= 0.0f)) { s1[k] |= 1u << (8 * c); v = -v; } a1[k][c] = v; t1[c] = v * v; }
                }
            }
            if (e < 144) {
                reinterpret_cast<float4 *>(sqw[0])[e] = make_float4(t0[0], t0[1], t0[2], t0[3]);
                reinterpret_cast<float4 *>(sqw[1])[e] = make_float4(t1[0], t1[1], t1[2], t1[3]);
            }
        }
    }
    HX_WAVE_SYNC();
    // band energies: lane (ch, sfb) adds its band's squares in line order - L / R first, then (joint stereo) M / S
    const int ch = lane >> 5, i = lane & 31;
    const int cbw = (i < 22) ? p->look_log_cbwmb[i] : 0;
    const bool eband = i < (ch ? nb_e1 : nb_e0);
    const int b0 = eband ? p->startBand_l[i] : 0, bn = eband ? p->nBand_l[i] : 0;
    float e_lr = 0.0f;
    int n0 = 0, n0ms = 0;
    if (eband) {
        e_lr = band_sum(&sqw[ch][b0], bn, 0.0f);
        n0 = hx_mblog(t_mblog, e_lr) - cbw;
    }
    if (ms) {
        HX_WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int e = lane + 64 * k;
            if (e < 144) {
                // (lines past nl_mag0 were left raw above; their squares are never summed)
                reinterpret_cast<float4 *>(sqw[0])[e] = make_float4(a0[k][0] * a0[k][0], a0[k][1] * a0[k][1], a0[k][2] * a0[k][2], a0[k][3] * a0[k][3]);
                reinterpret_cast<float4 *>(sqw[1])[e] = make_float4(a1[k][0] * a1[k][0], a1[k][1] * a1[k][1], a1[k][2] * a1[k][2], a1[k][3] * a1[k][3]);
            }
        }
        HX_WAVE_SYNC();
        if (eband) n0ms = hx_mblog(t_mblog, band_sum(&sqw[ch][b0], bn, 0.0f)) - cbw;
    }
    // x^(3/4) of the coded magnitudes and the band maxima (bit patterns of non-negative floats order like integers)
    float q0[3][4], q1[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int e = lane + 64 * k;
        unsigned bl = 0;
        if (e < 144) bl = reinterpret_cast<const unsigned *>(p->band_of_line)[e];       // the four lines' bands
        // The band maximum of x^(3/4) is the x^(3/4) of the band's largest magnitude: the piecewise-linear fit is monotone
        // over every non-negative float (checked exhaustively: tools/check_pow34_monotone.cpp).  So the lines contribute
        // their magnitudes (sign bit off: lines past the magnitude range are raw, and the fit ignores the sign), and the
        // band lane evaluates the fit once - 44 evaluations per granule instead of 1152.  The lines' own x^(3/4) is only
        // formed for the tests' tap (the allocator's helper wave computes it for itself).
        // A lane's four lines are two pairs, and a pair never straddles a band or the end of a coded range (bands start on even
        // lines and have even widths): one LDS atomic per pair - per four lines when both pairs are in one band - instead of one
        // per line.  (Atomics of a wave on one address are served one lane after the other: in a wide band that was up to 40
        // passes per instruction, 24 instructions per lane.)
        {
            const int b0 = bl & 255, b2 = (bl >> 16) & 255, j0 = 4 * e, j2 = 4 * e + 2;
            int m00 = max(__float_as_int(a0[k][0]) & 0x7FFFFFFF, __float_as_int(a0[k][1]) & 0x7FFFFFFF);
            const int m02 = max(__float_as_int(a0[k][2]) & 0x7FFFFFFF, __float_as_int(a0[k][3]) & 0x7FFFFFFF);
            int m10 = max(__float_as_int(a1[k][0]) & 0x7FFFFFFF, __float_as_int(a1[k][1]) & 0x7FFFFFFF);
            const int m12 = max(__float_as_int(a1[k][2]) & 0x7FFFFFFF, __float_as_int(a1[k][3]) & 0x7FFFFFFF);
            // (inside / outside the coded ranges: part of what makes a group - with -HF the range ends inside the last band's run
            // of the line-to-band table, which maps everything above band 20 to band 21)
            const int in0 = (j0 < nl_p0) | ((j0 < nl_p1) << 1), in2 = (j2 < nl_p0) | ((j2 < nl_p1) << 1);
            const bool one = b0 == b2 && in0 == in2;
            if (one) { m00 = max(m00, m02); m10 = max(m10, m12); }
            // ... and per pair or four of neighbouring lanes whose lines lie in one band and on one side of the coded ranges' ends
            // (they are then also all below line 576 or all above): the group's first lane brings the maximum of the group
            bool issue = true;
            {
                const int key = one ? (b0 | (in0 << 8)) : -1 - lane;       // (a lane whose lines straddle two bands joins no group)
#define PREP_QP(v, ctrl) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xf, 0xf, true)
                const bool pair = PREP_QP(key, 0xB1) == key;                            // quad_perm [1,0,3,2]: the lane beside this one
                if (pair) { m00 = max(m00, PREP_QP(m00, 0xB1)); m10 = max(m10, PREP_QP(m10, 0xB1)); }
                const bool quad = pair && PREP_QP((int) pair, 0x4E) != 0 && PREP_QP(key, 0x4E) == key;      // quad_perm [2,3,0,1]: the other pair
                if (quad) { m00 = max(m00, PREP_QP(m00, 0x4E)); m10 = max(m10, PREP_QP(m10, 0x4E)); }
#undef PREP_QP
                issue = quad ? (lane & 3) == 0 : (pair ? (lane & 1) == 0 : true);
            }
            if (issue && e < 144 && j0 < nl_p0) atomicMax(&xmax[wv][0][b0], m00);
            if (issue && e < 144 && j0 < nl_p1) atomicMax(&xmax[wv][1][b0], m10);
            if (!one) {
                if (e < 144 && j2 < nl_p0) atomicMax(&xmax[wv][0][b2], m02);
                if (e < 144 && j2 < nl_p1) atomicMax(&xmax[wv][1][b2], m12);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = 4 * e + c;
            q0[k][c] = q1[k][c] = 0.0f;
            if (x34o) {
                if (e < 144 && j < nl_p0) q0[k][c] = hx_pow34(t_a, t_b, t_exp, a0[k][c]);
                if (e < 144 && j < nl_p1) q1[k][c] = hx_pow34(t_a, t_b, t_exp, a1[k][c]);
            }
        }
    }
    HX_WAVE_SYNC();
    int gz = 0;
    float xm = 0.0f;
    if (i < 22) xm = hx_pow34(t_a, t_b, t_exp, __int_as_float(xmax[wv][ch][i]));
    if (i < (ch ? nb_z1 : nb_z0)) gz = max(0, hx_round((0.017716950f * hx_mblog(t_mblog, xm) + (104.585000f - 100.0f + 8.0f))));
    // masking threshold of the band: the two partitions' thresholds, each clamped against twice the previous
    // granule's unless this is a stop block, weighted by the partitions' energies
    int mmb = 0;
    if (i < 21) {
        const float2 th = reinterpret_cast<const float2 *>(thr + unit * 128 + ch * 64)[i];
        const float2 en = reinterpret_cast<const float2 *>(etab + unit * 128 + ch * 64)[i];
        const float2 pv = reinterpret_cast<const float2 *>((g == 0 ? thrprev + (long long) s * 128 : thr + (unit - 1) * 128) + ch * 64)[i];
        float s1v = th.x, s2v = th.y;
        const float t1 = (g == 0) ? pv.x : 2.0f * pv.x, t2 = (g == 0) ? pv.y : 2.0f * pv.y;
        if (btype != 3) {
            if (s1v > t1) { const float f = 0.1f * s1v; s1v = t1; if (s1v < f) s1v = f; }
            if (s2v > t2) { const float f = 0.1f * s2v; s2v = t2; if (s2v < f) s2v = f; }
        }
        float emax = en.x;
        if (emax < en.y) emax = en.y;
        mmb = hx_mblog(t_mblog, (en.x * s1v + en.y * s2v) / emax);
    }
    HxBandPrep *bp = band + unit;
    if (i < 22) {
        bp->xsxx[ch][i] = e_lr; bp->x34max[ch][i] = xm; bp->n0[ch][i] = n0; bp->n0ms[ch][i] = n0ms;
        bp->gzero[ch][i] = gz; bp->maskmb[ch][i] = mmb;
    }
    {   // The signs to their buffer, straight from the owning lanes.  Magnitudes and x^(3/4) are not stored: the allocator's
        // helper wave forms them again from the spectrum it fetches, in time it would otherwise spend waiting - cheaper
        // than 4.8 GB of stores and as many loads per launch.  (xmag_dbg, x34o: the tests' taps.)
        float4 *dq = reinterpret_cast<float4 *>(x34o + unit * 1152);     // (x34o: the tests' tap; the allocator's helper wave computes x^(3/4) again)
        unsigned *ds = sgn + unit * (2 * HX_SGN_WORDS);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int e = lane + 64 * k;
            if (e < 144) {
                if (xmag_dbg) {
                    float4 *dx = reinterpret_cast<float4 *>(xmag_dbg + unit * 1152);
                    dx[e] = make_float4(a0[k][0], a0[k][1], a0[k][2], a0[k][3]);
                    dx[144 + e] = make_float4(a1[k][0], a1[k][1], a1[k][2], a1[k][3]);
                }
                if (x34o) {
                    dq[e] = make_float4(q0[k][0], q0[k][1], q0[k][2], q0[k][3]);
                    dq[144 + e] = make_float4(q1[k][0], q1[k][1], q1[k][2], q1[k][3]);
                }
            }
            // signs as one bit per line, line order: a lane's four lines are a nibble (its sign bytes' low bits), eight
            // neighbouring lanes a word - OR over the group of eight on the DPP path, the group's first lane stores it
            unsigned w0 = ((s0[k] & 1u) | ((s0[k] >> 7) & 2u) | ((s0[k] >> 14) & 4u) | ((s0[k] >> 21) & 8u)) << (4 * (lane & 7));
            unsigned w1 = ((s1[k] & 1u) | ((s1[k] >> 7) & 2u) | ((s1[k] >> 14) & 4u) | ((s1[k] >> 21) & 8u)) << (4 * (lane & 7));
            w0 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w0, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
            w1 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w1, 0xB1, 0xf, 0xf, true);
            w0 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w0, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
            w1 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w1, 0x4E, 0xf, 0xf, true);
            w0 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w0, 0x141, 0xf, 0xf, true);     // row_half_mirror: the other quad of the eight
            w1 |= (unsigned) __builtin_amdgcn_update_dpp(0, (int) w1, 0x141, 0xf, 0xf, true);
            if ((lane & 7) == 0 && e < 144) { ds[e >> 3] = w0; ds[HX_SGN_WORDS + (e >> 3)] = w1; }
        }
    }
}
