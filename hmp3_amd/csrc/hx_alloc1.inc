// hx_alloc1.inc - the first-generation allocator (reference class CBitAllo1, bitallo1.cpp:100-1813), compiled into
// the k_alloc1 / k_alloc1_lsf kernels (HX_A1): joint stereo with an intensity part and dual channel, long blocks
// only, CBR only - the low-bitrate corner the newer allocator does not cover (mp3enc.cpp:696-766).
//
// One scalefactor band per lane (lane = 32 ch + sfb): a band lane walks its own lines in order, so every float
// sum has the reference's order; the bands' gain searches run side by side; integer totals are wave reductions.
// The few sums that run over the bands themselves (the mean noise-to-mask level) are added by one lane in the
// reference's (channel, band) order.  Arithmetic follows the reference expression by expression.  bitallo1.cpp is C++:
// its log10 / log / sqrt calls on float arguments are libm's log10f / logf / sqrtf (smr_adj, smr_adj_joint,
// compute_x34, fnc_noise2, fnc_noise2_cb - checked in the object code), and the arithmetic around them is float
// where every operand is.  logf and log10f are not correctly rounded in libm, so they are restated (hx_libm32.h).
//
// Working set in LDS: the line arrays of AllocLds (xr, x34, ix, signx), the per-band arrays of the long-block
// union, and the A1 members below.  Channel index = data channel; in dual-channel mode the reference runs its
// object on one channel at a time at index 0 - here that channel keeps its own index and the carried values
// (gain steps, bit-estimate feedback) are loaded and stored around the call.

#define HX_HD __device__ __forceinline__
#include "hx_libm32.h"

struct A1Ctx { int c0, nch, ms, is; };      // channels [c0, c0 + nch), M/S coding, intensity part present

#define A1_CH (LANE >> 5)
#define A1_I (LANE & 31)
// lane owns band A1_I of channel A1_CH and the channel takes part in this call
#define A1_BAND(cx) (A1_CH >= (cx).c0 && A1_CH < (cx).c0 + (cx).nch && A1_I < p->nsf[A1_CH])

__device__ __forceinline__ float a1_mask_db(const HxParams *gp, float sig, float mask, float xsxx, int i)
{
    const float r = sig / (mask * (0.1f + 0.0001f * xsxx));
    if (r < 1.0e-10f) return 100.0f;
    return hx_a1_mask_db_of(r, gp->a1_log_cbw[i]);
}

// the factor that brings an intensity band's L + R to the pair's energy, before its clamp (a1_smr's intensity bands): e0, e1 the
// energies of L and R, r that of L + R; at the MPEG-1 rates and at the MPEG-2 ones
__device__ __forceinline__ float a1_is_scale(float e0, float e1, float r)
{
    // (the inner square root is sqrtf: correctly rounded, so the double one rounded to float is the same value)
    return (float) (sqrt(((double) (e0 + e1) + 2.0 * (double) (float) sqrt((double) (e0 * e1))) / (double) r));
}
__device__ __forceinline__ float a1_is_scale_lsf(float e0, float e1, float r)
{
    const float a = (e0 > e1) ? e0 : e1;
    return (float) (sqrt((double) (a / r)));
}

// signal and mask per scalefactor band from the psy kernel's partition data, with pre-echo control (reference
// spdsmr.c:275-318, long blocks of type 0): sig = the band's two partition energies, mask = their thresholds
// weighted by the energies.  Bands the model does not reach keep the encoder's initial 100 / 100.
__device__ void a1_sigmask(AllocLds &L, const AllocPrm *p, const float *etab, const float *thr, const float *esave_prev, int esave_doubled)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, m = LANE & 31;
    if (m < NB) {
        float sig = 100.0f, mask = 100.0f;
        if (m < 21 && 2 * m < p->npart_l) {
            const float2 th = reinterpret_cast<const float2 *>(thr + ch * 64)[m];
            const float2 en = reinterpret_cast<const float2 *>(etab + ch * 64)[m];
            const float2 pv = reinterpret_cast<const float2 *>(esave_prev + ch * 64)[m];
            float s1 = th.x, s2 = th.y;
            const float t1 = esave_doubled ? pv.x : 2.0f * pv.x, t2 = esave_doubled ? pv.y : 2.0f * pv.y;
            if (s1 > t1) { const float f = 0.1f * s1; s1 = t1; if (s1 < f) s1 = f; }
            if (s2 > t2) { const float f = 0.1f * s2; s2 = t2; if (s2 < f) s2 = f; }
            float emax = en.x;
            if (emax < en.y) emax = en.y;
            mask = (en.x * s1 + en.y * s2) / emax;
            sig = en.x + en.y;
        }
        L.a_sig[ch][m] = sig;
        L.a_smask[ch][m] = mask;
    }
    HX_WAVE_SYNC();
}

// signs, magnitudes, band energies, M/S and intensity processing, masks in dB (bitallo1.cpp:634-907)
__device__ void a1_smr(AllocLds &L, const AllocPrm *p, const HxParams *gp, const A1Ctx cx)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    const int nsf_st = cx.is ? p->nsf[1] : 0;       // bands below it are coded per channel (or M/S); from it on by intensity
    if (!cx.is || !cx.ms) {     // per-channel bands: sign and magnitude of every line, energy in line order
        if (A1_BAND(cx) && (!cx.is || i < nsf_st)) {
            float e = 1.0e-12f;
            const int k0 = L.startBand[i], n = L.nBand[i];
            for (int k = k0; k < k0 + n; k++) {
                float v = L.xr[ch][k];
                unsigned char sg = 0;
                if (v < 0.0f) { sg = 1; v = -v; }
                L.signx[ch][k] = sg;
                L.xr[ch][k] = v;
                e += v * v;
            }
            L.xsxx[ch][i] = e;
        }
    } else if (ch == 0 && i < nsf_st) {     // M/S bands: (L + R) / sqrt 2, (L - R) / sqrt 2; energies of L and R
        float e0 = 1.0e-12f, e1 = 1.0e-12f;
        const int k0 = L.startBand[i], n = L.nBand[i];
        const float c707 = gp->a1_c707;
        for (int k = k0; k < k0 + n; k++) {
            const float l = L.xr[0][k], r = L.xr[1][k];
            e0 += l * l;
            e1 += r * r;
            const float a = c707 * l, b = c707 * r;
            float m = a + b, d = a - b;
            unsigned char s0 = 0, s1 = 0;
            if (m < 0.0f) { s0 = 1; m = -m; }
            if (d < 0.0f) { s1 = 1; d = -d; }
            L.signx[0][k] = s0; L.signx[1][k] = s1;
            L.xr[0][k] = m; L.xr[1][k] = d;
        }
        L.xsxx[0][i] = e0; L.xsxx[1][i] = e1;
    }
    HX_WAVE_SYNC();
    if (cx.is && cx.ms && ch == 0 && i >= 5 && i < nsf_st) {   // thin out the side channel: pairs weaker than a share of the band pair go
        const int k0 = L.startBand[i], n = L.nBand[i];
        const float ss = gp->a1_sparse[i];
        for (int k = k0; k < k0 + n; k += 2) {
            const float a = L.xr[1][k] * L.xr[1][k] + L.xr[1][k + 1] * L.xr[1][k + 1];
            const float b = ss * (a + L.xr[0][k] * L.xr[0][k] + L.xr[0][k + 1] * L.xr[0][k + 1]);
            if (a < b) L.xr[1][k] = L.xr[1][k + 1] = 0.0f;
        }
    }
    if (cx.is && ch == 0 && i >= nsf_st && i < p->nsf[0]) {   // intensity bands: L + R in channel 0, rescaled to the pair's energy
        float e0 = 1.0e-12f, e1 = 1.0e-12f, r = 1.0f;
        const int k0 = L.startBand[i], n = L.nBand[i];
        for (int k = k0; k < k0 + n; k++) {
            e0 += L.xr[0][k] * L.xr[0][k];
            e1 += L.xr[1][k] * L.xr[1][k];
            float v = L.xr[0][k] + L.xr[1][k];
            r += v * v;
            unsigned char sg = 0;
            if (v < 0.0f) { sg = 1; v = -v; }
            L.signx[0][k] = sg;
            L.xr[0][k] = v;
        }
        if (!HX_LSF) {
            r = a1_is_scale(e0, e1, r);
            if (r > 1.5f) r = 1.5f;
        } else {
            r = a1_is_scale_lsf(e0, e1, r);
            if (r > 1.2f) r = 1.2f;
        }
        for (int k = k0; k < k0 + n; k++) L.xr[0][k] = r * L.xr[0][k];
        L.xsxx[0][i] = e0; L.xsxx[1][i] = e1;
        // the band's intensity position rides in the right channel's scalefactor
        int pos;
        if (e0 <= e1) {
            pos = gp->a1_is_pos[(int) (32.0f * e0 / e1 + 0.5f)];
            if (HX_LSF && pos != 0) pos -= 1;
        } else {
            pos = gp->a1_is_pos[(int) (32.0f * e1 / e0 + 0.5f)];
            if (!HX_LSF) pos = 6 - pos;
        }
        L.sf[1][i] = pos;
        const float sg = L.a_sig[0][i] + L.a_sig[1][i], mk = L.a_smask[0][i] + L.a_smask[1][i];
        L.a_mask[0][i] = a1_mask_db(gp, sg, mk, e0 + e1, i);
    }
    HX_WAVE_SYNC();
    if (A1_BAND(cx) && (!cx.is || i < nsf_st)) L.a_mask[ch][i] = a1_mask_db(gp, L.a_sig[ch][i], L.a_smask[ch][i], L.xsxx[ch][i], i);
    HX_WAVE_SYNC();
    if (cx.is && cx.ms && i < nsf_st) {
        const float m = 0.5f * (L.a_mask[0][i] + L.a_mask[1][i]);
        HX_WAVE_SYNC();
        L.a_mask[ch][i] = m;
    }
    HX_WAVE_SYNC();
}

// x^(3/4) of the coded lines, band maxima, zero-gain steps (bitallo1.cpp:589-631); returns the largest x^(3/4)
__device__ float a1_x34(AllocLds &L, const AllocPrm *p, const HxParams *gp, const A1Ctx cx)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    float m = 0.0f;
    if (A1_BAND(cx)) {
        const int k0 = L.startBand[i], n = L.nBand[i];
        for (int k = k0; k < k0 + n; k++) {
            const float q = pow34(L, L.xr[ch][k]);
            L.x34[ch][k] = q;
            if (m < q) m = q;
        }
        L.x34max[ch][i] = m;
        int gz = 0;
        if (!(m < gp->a1_gz0)) gz = hx_a1_gz_of(gp->a1_gz1, gp->a1_gz2, m);
        L.gzero[ch][i] = gz;
        L.gmin[ch][i] = max(0, gz - GMIN_OFFSET);
    }
    const int mm = hx_wave_max(__float_as_int(m));      // x^(3/4) >= 0: the bit patterns order like the values
    HX_WAVE_SYNC();
    return __int_as_float(mm);
}

__device__ __forceinline__ void a1_ixmax(AllocLds &L, const AllocPrm *p, const A1Ctx cx)
{
    HX_LANE_DECL;
    if (A1_BAND(cx)) L.ixmax[A1_CH][A1_I] = (int) ((0.5f - 0.0946f) + L.x34max[A1_CH][A1_I] * L.look_34igain[L.gsf[A1_CH][A1_I]]);
    HX_WAVE_SYNC();
}

__device__ __forceinline__ int a1_bit_est(AllocLds &L, const AllocPrm *p, const HxParams *gp, const A1Ctx cx)
{
    HX_LANE_DECL;
    int n = 0;
    if (A1_BAND(cx)) {
        const int ixm = L.ixmax[A1_CH][A1_I];
        const int bits = ixm < 256 ? gp->a1_bits[ixm] : (ixm < 512 ? 16 * 11 : (ixm < 2048 ? 16 * 13 : 16 * 15));
        n = L.nBand[A1_I] * bits;
    }
    return hx_wave_sum(n) >> 4;
}

// move all gains until the bit estimate meets the target (bitallo1.cpp:959-1133)
__device__ int a1_bit_seek(AllocLds &L, const AllocPrm *p, const HxParams *gp, const A1Ctx cx, int target, float dGdB)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    const bool band = A1_BAND(cx);
    a1_ixmax(L, p, cx);
    int nbits = a1_bit_est(L, p, gp, cx);
    int delta = nbits - target;
    if (delta > 0) {
        for (int it = 0; it < 10; it++) {
            if (delta <= 0) break;
            int dG = (int) (dGdB * delta);
            if (dG < 1) dG = 1;
            if (band) L.gsf[ch][i] = min(L.gsf[ch][i] + dG, L.gzero[ch][i]);
            HX_WAVE_SYNC();
            a1_ixmax(L, p, cx);
            nbits = a1_bit_est(L, p, gp, cx);
            delta = nbits - target;
        }
        return nbits;
    }
    int mindelta = target >> 2;
    if (mindelta < 100) mindelta = 100;
    delta = -delta;
    if (delta < mindelta) return nbits;
    // (the reference's loop shares its counter with the band loop inside it: it runs once unless the last channel
    // has fewer than nine bands)
    const int nlast = p->nsf[cx.c0 + cx.nch - 1];
    for (int it = 0; it < 10; it = nlast + 1) {
        int dG = (int) (dGdB * delta);
        if (dG < 1) dG = 1;
        int g = 0;
        if (band) { g = max(L.gsf[ch][i] - dG, 0); L.gsf[ch][i] = g; }
        const int gz_flag = hx_wave_or(g);
        HX_WAVE_SYNC();
        a1_ixmax(L, p, cx);
        nbits = a1_bit_est(L, p, gp, cx);
        delta = target - nbits;
        if (delta < mindelta) break;
        if (gz_flag == 0) break;
    }
    return nbits;
}

__device__ __forceinline__ float a1_noise_of(const float *tab, int ixm, int gsf)
{
    if (ixm < 256) return tab[ixm] + 1.505f * gsf;
    ixm = min(ixm >> 5, 255);
    return tab[512 + ixm] + 1.505f * gsf;
}

// noise of band (ch, i) at its current gain: from the band's largest value (stage 1) or line by line (stage 2)
// tab = [f_ix | f_ixmax | f_big_ix | f_big_ixmax] staged in LDS
__device__ __forceinline__ void a1_noise_cb(AllocLds &L, const HxParams *gp, const float *tab, int stage2, int ch, int i)
{
    const int gsf = L.gsf[ch][i];
    if (!stage2) {
        const int ixm = (int) ((0.5f - 0.0946f + 0.002f) + L.x34max[ch][i] * L.look_34igain[gsf]);
        L.ixmax[ch][i] = ixm;
        L.a_noise[ch][i] = a1_noise_of(tab + 256, ixm, gsf);
        return;
    }
    if (gsf == L.a_lastGsf[ch][i]) return;
    L.a_lastGsf[ch][i] = gsf;
    const float igain = L.look_34igain[gsf];
    const int k0 = L.startBand[i], n = L.nBand[i];
    float sum = 0.0f;
    for (int k = k0; k < k0 + n; k++) {
        int ixm = (int) ((0.5f - 0.0946f) + L.x34[ch][k] * igain);
        if (ixm < 256) sum += tab[ixm];
        else sum += tab[512 + min(ixm >> 5, 255)];
    }
    L.a_noise[ch][i] = 10.0f * hx_log10f(sum) - gp->a1_log_cbw[i] + 1.505f * gsf;
}

// every band moves its gain until its noise-to-mask distance equals the mean one (bitallo1.cpp:1291-1395)
__device__ int a1_noise_seek(AllocLds &L, const AllocPrm *p, const HxParams *gp, const float *tab, const A1Ctx cx, int stage2)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    const bool band = A1_BAND(cx);
    if (LANE == 0) {        // mean over the bands that can still move, added in (channel, band) order
        int n = 0;
        float asum = 0.0f;
        for (int c = cx.c0; c < cx.c0 + cx.nch; c++)
            for (int b = 0; b < p->nsf[c]; b++)
                if (L.gsf[c][b] > 0 && L.gsf[c][b] < L.gzero[c][b]) { asum += L.a_noise[c][b] - L.a_mask[c][b]; n++; }
        L.tmp[0] = n;
        if (n > 1) { const float a = asum / n; L.a_alpha = a; L.tmp[1] = __float_as_int(a); }
    }
    HX_WAVE_SYNC();
    if (L.tmp[0] <= 1) return 0;
    const float a = __int_as_float(L.tmp[1]);
    int dgmax = 0;
    if (band) {
        const float mask = L.a_mask[ch][i];
        const int gz = L.gzero[ch][i];
        float dn = L.a_noise[ch][i] - mask - a;
        if (dn > 1.0) {
            if (L.gsf[ch][i] > 0) {
                float dn0 = dn;
                int gsf0 = L.gsf[ch][i];
                const int gsf00 = gsf0;
                for (int it = 0; it < 50; it++) {
                    if (L.gsf[ch][i] <= 0) break;
                    const int dg = (int) (0.5f * dn + 0.5f);
                    if (dg <= 0) break;
                    L.gsf[ch][i] = max(L.gsf[ch][i] - dg, 0);
                    a1_noise_cb(L, gp, tab, stage2, ch, i);
                    dn = L.a_noise[ch][i] - mask - a;
                    if (dn < -1.0f) { dn = dn0 = 0.5f * dn0; L.gsf[ch][i] = gsf0; continue; }
                    dn0 = dn;
                    gsf0 = L.gsf[ch][i];
                }
                dgmax = gsf00 - L.gsf[ch][i];
            }
        } else if (dn < -1.0f) {
            if (L.gsf[ch][i] < gz) {
                float dn0 = dn;
                int gsf0 = L.gsf[ch][i];
                const int gsf00 = gsf0;
                for (int it = 0; it < 50; it++) {
                    if (L.gsf[ch][i] >= gz) break;
                    const int dg = (int) (-0.5f * dn);
                    if (dg <= 0) break;
                    L.gsf[ch][i] = min(L.gsf[ch][i] + dg, gz);
                    a1_noise_cb(L, gp, tab, stage2, ch, i);
                    dn = L.a_noise[ch][i] - mask - a;
                    if (dn > 1.0f) { dn = dn0 = 0.5f * dn0; L.gsf[ch][i] = gsf0; continue; }
                    dn0 = dn;
                    gsf0 = L.gsf[ch][i];
                }
                dgmax = L.gsf[ch][i] - gsf00;
            }
        }
    }
    dgmax = hx_wave_max(max(dgmax, 0));
    HX_WAVE_SYNC();
    return dgmax;
}

// global gain, scalefactors, scalefac_scale / preflag of every channel of the call (bitallo1.cpp:1427-1690);
// returns the smallest global gain (100 for a silent channel)
__device__ int a1_scale_factors(AllocLds &L, const AllocPrm *p, const A1Ctx cx)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    const bool band = A1_BAND(cx);
    int gsf = 0, act = 0;
    if (band) {
        gsf = max(L.gsf[ch][i], L.gmin[ch][i]);
        act = L.ixmax[ch][i] > 0;
    }
    const int Gtmp = hx_half_max((band && act) ? gsf : -1);
    int sf = 0, scale = 0, pre = 0, Gout = Gtmp;
    if (Gtmp < 0) {     // nothing to code in this channel
        Gout = hx_half_max(band ? L.gzero[ch][i] : -1);
        if (band) { sf = 0; gsf = L.gzero[ch][i]; }
    } else {
        if (band && act) sf = Gtmp - gsf;
        const int pt = pretab(i);
        const int pre2 = (i >= 11 && i < 21) ? 15 + 2 * pt : 0, pre4 = (i >= 11 && i < 21) ? 31 + 4 * pt : 0;
        // which scale / pre-emphasis the scalefactors need: conditions over the channel's bands
        const bool lo = band && i < 11, hi = band && i >= 11;
        scale = hx_half_or((lo && sf > 31) ? 1 : 0);
        if (HX_LSF) {
            if (!scale) scale = hx_half_or((hi && sf > 15) ? 1 : 0);
        } else {
            if (!scale) scale = hx_half_or((hi && sf > pre2) ? 1 : 0);
            const int sh = scale ? 2 : 1;
            pre = hx_half_or((hi && sf > (scale ? 31 : 15)) ? 1 : 0);
            if (pre && hx_half_or((hi && (sf >> sh) < pt) ? 1 : 0)) pre = 0;       // a negative scalefactor would result
        }
        if (band) {
            const int cap = lo ? (scale ? 63 : 31) : (pre ? (scale ? pre4 : pre2) : (scale ? 31 : 15));
            if (sf > cap) sf = cap;
            sf &= scale ? ~3 : ~1;
            gsf = min(Gtmp - sf, L.gzero[ch][i]);
        }
    }
    if (band) { L.gsf[ch][i] = gsf; L.sf[ch][i] = sf; }
    if (i == 0 && ch >= cx.c0 && ch < cx.c0 + cx.nch) { L.G[ch] = Gout; L.preemp[ch] = pre; L.scale[ch] = scale; }
    const int in = (i == 0 && ch >= cx.c0 && ch < cx.c0 + cx.nch) ? (Gtmp < 0 ? 100 : Gtmp) : 999;
    const int gmin = -hx_wave_max(-in);
    HX_WAVE_SYNC();
    return gmin;
}

// the Huffman bits of cx's channels, one after the other on the master wave (a1_quant_count; the test tap k_debug_count_*)
__device__ __forceinline__ int a1_count_channels(AllocLds &L, const AllocPrm *p, const A1Ctx cx)
{
    int bits = 0;
    for (int c = cx.c0; c < cx.c0 + cx.nch; c++) bits += count_bits_ch(L, p, c, p->nsf[c]);
    return bits;
}

// quantise the bands whose gain changed since the last time, count the Huffman bits of every channel
__device__ int a1_quant_count(AllocLds &L, const AllocPrm *p, const A1Ctx cx)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    a1_ixmax(L, p, cx);
    if (A1_BAND(cx) && L.gsf[ch][i] != L.a_lastGsf[ch][i]) {
        L.a_lastGsf[ch][i] = L.gsf[ch][i];
        const int k0 = L.startBand[i], n = L.nBand[i];
        if (L.ixmax[ch][i] <= 0) { for (int k = k0; k < k0 + n; k++) L.ix[ch][k] = 0; }
        else {
            const float igain = L.look_34igain[L.gsf[ch][i]];
            for (int k = k0; k < k0 + n; k++) L.ix[ch][k] = (int) ((0.5f - 0.0946f) + L.x34[ch][k] * igain);
        }
    }
    HX_WAVE_SYNC();
    const int bits = a1_count_channels(L, p, cx);
    HX_WAVE_SYNC();
    return bits;
}

// CBitAllo1::BitAllo with allo_2 (bitallo1.cpp:214-382, 1693-1811) for the channels of cx.  In: L.xr (raw spectrum),
// L.a_sig / L.a_smask (psy model per band).  Out: L.ix, L.signx, L.gr[igr][ch], L.sfout[igr][ch].
__device__ void bitallo1(AllocLds &L, const AllocPrm *p, const HxParams *gp, const A1Ctx cx, int igr,
                         int min_bits_arg, int target_bits_arg, int max_bits)
{
    HX_LANE_DECL;
    const int ch = A1_CH, i = A1_I;
    const bool band = A1_BAND(cx), mych = ch >= cx.c0 && ch < cx.c0 + cx.nch;
    const float *tab = &L.term[0][0];               // the four noise tables, staged by the kernel prologue
    float dBG = 0.0f;
    for (int c = cx.c0; c < cx.c0 + cx.nch; c++) dBG += (float) L.startBand[p->nsf[c]];
    dBG = 0.25f * dBG;
    const float dGdB = 1.0f / dBG;
    const int min_bits = max(min_bits_arg, 0);
    int target_bits = max(target_bits_arg - (target_bits_arg >> 4), min_bits);
    if (LANE == 0) L.block_type = 0;
    if (mych && i < NB) { L.ixmax[ch][i] = 0; L.sf[ch][i] = (cx.is && ch == 1) ? L.sf[ch][i] : 0; }
    HX_WAVE_SYNC();
    a1_smr(L, p, gp, cx);
    const float x34mm = a1_x34(L, p, gp, cx);
    if (x34mm < 3.0f) {     // nothing worth coding in this granule
        if (LANE < 2 && LANE >= cx.c0 && LANE < cx.c0 + cx.nch) {
            HxGr *g = &L.gr[igr][LANE];
            g->global_gain = 0; g->window_switching_flag = 0; g->block_type = 0; g->mixed_block_flag = 0;
            g->preflag = g->scalefac_scale = 0;
            g->table_select[0] = g->table_select[1] = g->table_select[2] = 0;
            g->big_values = g->region0_count = g->region1_count = g->count1table_select = 0;
            g->aux_nquads = g->aux_bits = g->aux_not_null = 0;
            g->aux_nreg[0] = g->aux_nreg[1] = g->aux_nreg[2] = 0;
        }
        if (mych && i < NB) L.sfout[igr][ch][i] = 0;
        HX_WAVE_SYNC();
        return;
    }
    if (LANE == 0) {
        L.a_calls++;
        if (L.a_calls <= 20) L.a_running = 1.0f / L.a_calls;
    }
    // the bit estimate is off by a slowly varying amount: a running correction (bitadjust) is taken out of the target
    const int bslot = cx.nch == 1 ? cx.c0 : 0;
    int bitadjust = L.a_bitadjust[bslot];
    int target0_min = max(target_bits >> 1, min_bits), target0_max = (target_bits + max_bits) >> 1;
    if (bitadjust > (target_bits >> 1)) bitadjust = target_bits >> 1;
    const int target0 = target_bits - bitadjust;
    target0_min -= bitadjust;
    target0_max -= bitadjust;
    if (band) L.gsf[ch][i] = min(L.gsf[ch][i], L.gzero[ch][i]);        // start from the previous granule's gains
    if (mych && i < NB) L.a_lastGsf[ch][i] = -9999;
    HX_WAVE_SYNC();
    // stage 1: noise estimated from each band's largest quantised value
    int nbits = a1_bit_seek(L, p, gp, cx, target0, dGdB);
    for (int it = 0; it < 4; it++) {
        if (band) L.a_noise[ch][i] = a1_noise_of(tab + 256, L.ixmax[ch][i], L.gsf[ch][i]);
        HX_WAVE_SYNC();
        const int dsf = a1_noise_seek(L, p, gp, tab, cx, 0);
        if (dsf <= 0) break;
        nbits = a1_bit_seek(L, p, gp, cx, target0, dGdB);
        if (dsf < 2) break;
    }
    // stage 2: noise estimated line by line; the bit target follows the noise level reached
    for (int it = 0; it < 4; it++) {
        if (band) a1_noise_cb(L, gp, tab, 1, ch, i);
        HX_WAVE_SYNC();
        const int dsf = a1_noise_seek(L, p, gp, tab, cx, 1);
        if (dsf <= 0) break;
        int target = (int) (target0 + 0.5f * dBG * (L.a_alpha - L.a_ave));
        target = target > target0_max ? target0_max : (target < target0_min ? target0_min : target);
        nbits = a1_bit_seek(L, p, gp, cx, target, dGdB);
        if (dsf < 2) break;
    }
    if (mych && i < NB) L.a_lastGsf[ch][i] = -9999;
    HX_WAVE_SYNC();
    a1_scale_factors(L, p, cx);
    int bits = a1_quant_count(L, p, cx);
    bitadjust = bitadjust + ((bits - nbits - bitadjust) >> 3);
    {
        int tmp = min_bits - bits;
        if (tmp > 0) bitadjust = bitadjust - (min(tmp, 200) >> 2);
    }
    for (int j = 0; j < 3; j++) {       // spend more if below the minimum
        if ((min_bits - bits) < 50) break;
        int dG = (int) (dGdB * (min_bits - bits));
        if (dG < 1) dG = 1;
        int g = 0;
        if (band) { g = max(L.gsf[ch][i] - dG, 0); L.gsf[ch][i] = g; }
        const int gz_flag = hx_wave_or(g);
        HX_WAVE_SYNC();
        a1_scale_factors(L, p, cx);
        bits = a1_quant_count(L, p, cx);
        if (gz_flag == 0) break;
    }
    for (int j = 0; j < 100; j++) {     // give back if above the maximum
        if (bits <= max_bits) break;
        int dG = (int) (dGdB * (bits - max_bits));
        if (dG < 1) dG = 1;
        if (band) L.gsf[ch][i] += dG;
        HX_WAVE_SYNC();
        const int GG = a1_scale_factors(L, p, cx);
        bits = a1_quant_count(L, p, cx);
        if (GG >= 100) break;
    }
    if (LANE == 0) {
        L.a_bitadjust[bslot] = bitadjust;
        L.a_ave = L.a_ave + L.a_running * (L.a_alpha - L.a_ave);
    }
    // scalefactors as transmitted (bitallo1.cpp:547-586)
    if (mych && i < NB) {
        int s = 0;
        if (band) {
            s = (L.ixmax[ch][i] <= 0) ? 0 : L.sf[ch][i];
            s >>= L.scale[ch] ? 2 : 1;
            if (L.preemp[ch] && i >= 11) s -= pretab(i);
        } else if (cx.is && ch == 1 && i < p->nsf[0]) s = L.sf[1][i];      // intensity position
        L.sfout[igr][ch][i] = (i < 21) ? s : 0;
    }
    HX_WAVE_SYNC();
    if (cx.is && LANE == 0) {   // below the intensity part, trailing silent bands of the right channel carry "no intensity"
        for (int b = p->nsf[1] - 1; b >= 0; b--) {
            if (L.ixmax[1][b] > 0) break;
            L.sfout[igr][1][b] = gp->a1_ill_is_pos;
        }
    }
    if (LANE < 2 && LANE >= cx.c0 && LANE < cx.c0 + cx.nch) {
        const int c = LANE;
        HxGr *g = &L.gr[igr][c];
        g->global_gain = min(L.G[c] + (4 * 32 + 14), 255);
        g->window_switching_flag = 0; g->block_type = 0; g->mixed_block_flag = 0;
        g->preflag = L.preemp[c];
        g->scalefac_scale = L.scale[c];
        g->aux_bits = L.huff_bits[c];
        g->aux_not_null = (cx.is && c == 1) ? 1 : L.huff_bits[c];      // the right channel's scalefactors carry the intensity positions
        huffsel_to_gr(L, c, g);
    }
    HX_WAVE_SYNC();
}

#if !HX_LSF && !HX_TAP
// ---- k_debug_math (tests only; hx_batch_debug_math): the device math of the kernels on arguments of the caller's ----
// Lane i evaluates function fn (HxDebugMath) on in[i] (in[n + i], in[2 n + i]: the further operands) and stores out[i];
// all values are 32-bit patterns.  Every case calls the function the kernels call - this unit carries the allocator group's
// flags, the ones each of them is built with in the product - on the batch's own tables.  Built here once, not in the
// MPEG-2 twin of this unit.
__global__ __launch_bounds__(256) void k_debug_math(int fn, const unsigned *in, long long n, unsigned *out, const HxGlobalTabs *gt, const HxParams *gp)
{
    __shared__ unsigned short mblog16[256];     // the mB-log table as the low-footprint layout stages it (hx_alloc3.inc)
    mblog16[threadIdx.x] = (unsigned short) (gt->mblog[threadIdx.x] + 38227);
    __syncthreads();
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned u = in[i];
    const float x = hx_bits2f(u);
    unsigned r = 0;
    switch (fn) {
    case HX_DM_LOGF: r = hx_f2bits(hx_logf(x)); break;
    case HX_DM_LOG10F: r = hx_f2bits(hx_log10f(x)); break;
    case HX_DM_A1_MASK_DB: r = hx_f2bits(hx_a1_mask_db_of(x, hx_bits2f(in[n + i]))); break;
    case HX_DM_A1_GZ: r = (unsigned) hx_a1_gz_of(gp->a1_gz1, gp->a1_gz2, x); break;
    case HX_DM_DBLOG: r = hx_f2bits(dblog(x)); break;
    case HX_DM_DUAL_G: r = (unsigned) dual_gain_step(x); break;
    case HX_DM_IS_SCALE: r = hx_f2bits(a1_is_scale(x, hx_bits2f(in[n + i]), hx_bits2f(in[2 * n + i]))); break;
    case HX_DM_IS_SCALE_LSF: r = hx_f2bits(a1_is_scale_lsf(x, hx_bits2f(in[n + i]), hx_bits2f(in[2 * n + i]))); break;
    case HX_DM_DIV: r = hx_f2bits(x / hx_bits2f(in[n + i])); break;
    case HX_DM_MBLOG: r = (unsigned) hx_mblog(gt->mblog, x); break;
    case HX_DM_MBLOG16: r = (unsigned) hx_mblog16(mblog16, x); break;
    case HX_DM_MBEXP: r = hx_f2bits(hx_mbexp(gt->mbexp_lo, gt->mbexp_hi, (int) u)); break;
    case HX_DM_POW34: r = hx_f2bits(hx_pow34(gt->pow34_a, gt->pow34_b, gt->pow34_exp, x)); break;
    case HX_DM_ROUND: r = (unsigned) hx_round(x); break;
    }
    out[i] = r;
}
#endif
