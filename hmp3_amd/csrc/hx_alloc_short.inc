// hx_alloc_short.inc - short-block (3 windows x 192 lines) allocator of the K6 kernel
// (reference CBitAlloShort bitallos.cpp:202-1503, bitallosc.cpp:296-487, cnts.c:95-303).
// Short granules are rare (a few per cent), so the band-parallel phases simply run channel by
// channel with lane = 16*window + sfb; line-parallel phases are the same as for long blocks.
// The spectrum stays in window-major [3][192] order while allocating and is reordered to the
// sfb-major bitstream order once at the end (and on a scratch copy for every bit count).

// scratch copy of channel ch's lines in bitstream order: the channel's term buffer; in the low-footprint layout, where the
// lines themselves occupy the first half of that buffer, one half of its second half
#if HX_SLIM
#define S_SCRATCH(ch) (reinterpret_cast<ix_t *>(&L.term[1][0]) + 576 * (ch))
#else
#define S_SCRATCH(ch) (reinterpret_cast<ix_t *>(&L.term[(ch)][0]))
#endif
#define SW (LANE >> 4)
#define SI (LANE & 15)

// noise of every band of channel ch whose s_geval >= 0 (reference l3math.c:512-541)
__device__ void s_noise_sweep(AllocLds &L, const AllocPrm *p, int ch)
{
    HX_LANE_DECL;
    const int nb = p->nbmax_s;
    for (int t = LANE; t < 576; t += 64) {
        int w = t / 192, j = t - 192 * w;
        if (j < nb) {
            int g = L.s_geval[w][L.sband_of_line[j]];
            if (g >= 0) {
                float igain = LK_IGAIN(g), gain = LK_GAIN(g);
                float tmp = (igain * L.x34[ch][t] + (0.0f - 0.0946f));
                int qx = (int) (tmp + copysignf(0.5f, tmp));
                float xhat;
                if (qx >= 0 && qx < 256) xhat = gain * L.look_ix43[qx];
                else xhat = (float) (gain * ((qx >= 0 && qx < HX_POW43_N) ? L.pow43[qx] : pow((double) qx, (4.0 / 3.0))));
                tmp = L.xr[ch][t] - xhat;
                L.term[ch][t] = tmp * tmp;
            }
        }
    }
    HX_WAVE_SYNC();
    if (SW < 3 && SI < p->nsfs && L.s_geval[SW][SI] >= 0) {
        float sxx = band_sum(&L.term[ch][192 * SW + L.startBand_s[SI]], L.nBand_s[SI], 0.0f);
        L.s_tmpn[SW][SI] = MBLOG(1.0e-12f + sxx) - L.logcbw_s[SI];
    }
    HX_WAVE_SYNC();
}

// reference bitallos.cpp:695-741
__device__ void s_adjust_nt(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const bool band = SW < 3 && SI < p->nsfs;
    int a = 0, na = 0;
    for (int ch = 0; ch < p->nchan; ch++)
        if (band && L.s_snr[ch][SW][SI] > 0) { a += L.s_NT[ch][SW][SI]; na++; }
    a = hx_wave_sum(a);
    na = hx_wave_sum(na) + 1;
    a = a / na;
    if (a > 500)
        for (int ch = 0; ch < p->nchan; ch++)
            if (band && L.s_snr[ch][SW][SI] > 0) L.s_NT[ch][SW][SI] = (L.s_NT[ch][SW][SI] + a) >> 1;
    HX_WAVE_SYNC();
}

__device__ void s_pow34_gzero(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const int nb = p->nbmax_s;
    for (int t = LANE; t < 1152; t += 64) {
        int c = t / 576, r = t - 576 * c, j = r % 192;
        if (j < nb) L.x34[c][r] = pow34(L, L.xr[c][r]);
    }
    HX_WAVE_SYNC();
    if (SW < 3 && SI < p->nsfs)
        for (int ch = 0; ch < p->nchan; ch++) {
            const float *y = &L.x34[ch][192 * SW + L.startBand_s[SI]];
            float m = 0.0f;
            for (int j = 0; j < L.nBand_s[SI]; j++) if (y[j] > m) m = y[j];
            L.s_x34max[ch][SW][SI] = m;
            int gz = max(0, hx_round((0.017716950f * MBLOG(m) + (104.585000f - 100.0f + 8.0f))));
            L.s_gzero[ch][SW][SI] = gz;
            L.s_gmin[ch][SW][SI] = max(0, gz - GMIN_OFFSET);
        }
    HX_WAVE_SYNC();
}

// reference bitallos.cpp:475-570 (L/R) and :573-692 (M/S)
__device__ void s_startup(AllocLds &L, const AllocPrm *p, int ms, int MNR)
{
    HX_LANE_DECL;
    const int nb = p->nbmax_s;
    const bool band = SW < 3 && SI < p->nsfs;
    // squares of the L/R lines
    for (int t = LANE; t < 1152; t += 64) {
        int c = t / 576, r = t - 576 * c, j = r % 192;
        unsigned char sg = 0;
        if (j < nb) {
            float x = L.xr[c][r];
            if (!ms) {
                if (!(x >= 0.0f)) { sg = 1; x = -x; }
#if !HX_SLIM
                L.signx[c][r] = sg;
#endif
                L.xr[c][r] = x;
            }
            L.term[c][r] = x * x;
        }
#if HX_SLIM
        // (the 64 lines of a round share their channel and their word of the sign bits: 576 = 9 x 64)
        const unsigned long long sm = __ballot(sg != 0);
        if (!ms && LANE == 0) L.sgnbits[c][r >> 6] = sm;
#endif
    }
    HX_WAVE_SYNC();
    if (band)
        for (int ch = 0; ch < p->nchan; ch++)
            L.s_xsxx[ch][SW][SI] = band_sum(&L.term[ch][192 * SW + L.startBand_s[SI]], L.nBand_s[SI], 0.0f);
    HX_WAVE_SYNC();
    float ssum = 0.0f, sdif = 0.0f;
    if (ms) {
        for (int r = LANE; r < 576; r += 64) {
            int j = r % 192;
            unsigned char s0 = 0, s1 = 0;
            if (j < nb) {
                float l = L.xr[0][r], rr = L.xr[1][r];
                float x0 = (l + rr), x1 = (l - rr);
                if (x0 < 0.0f) { s0 = 1; x0 = -x0; }
                if (x1 < 0.0f) { s1 = 1; x1 = -x1; }
#if !HX_SLIM
                L.signx[0][r] = s0; L.signx[1][r] = s1;
#endif
                L.xr[0][r] = x0; L.xr[1][r] = x1;
                L.term[0][r] = x0 * x0;
                L.term[1][r] = x1 * x1;
            }
#if HX_SLIM
            const unsigned long long m0 = __ballot(s0 != 0), m1 = __ballot(s1 != 0);
            if (LANE == 0) { L.sgnbits[0][r >> 6] = m0; L.sgnbits[1][r >> 6] = m1; }
#endif
        }
        HX_WAVE_SYNC();
        if (band) {
            ssum = band_sum(&L.term[0][192 * SW + L.startBand_s[SI]], L.nBand_s[SI], 0.0f);
            sdif = band_sum(&L.term[1][192 * SW + L.startBand_s[SI]], L.nBand_s[SI], 0.0f);
        }
    }
    int act = 0;
    if (band) {
        const int cbw = L.logcbw_s[SI], n = L.nBand_s[SI];
        if (!ms) {
            for (int ch = 0; ch < p->nchan; ch++) {
                int n0 = MBLOG(L.s_xsxx[ch][SW][SI]) - cbw, nt, snr;
                if (n0 < -2000) { nt = n0 + 1000; snr = -1000; }
                else {
                    nt = drop_guard(n0, (L.s_maskmb[ch][SW][SI] - cbw) - MNR);
                    snr = n0 - nt;
                    act += n;
                }
                L.s_Noise0[ch][SW][SI] = n0; L.s_NT[ch][SW][SI] = nt; L.s_snr[ch][SW][SI] = snr;
            }
        } else {
            int N0L = MBLOG(L.s_xsxx[0][SW][SI]) - cbw, N0R = MBLOG(L.s_xsxx[1][SW][SI]) - cbw, NTL, NTR;
            if (N0L < -2000) NTL = 10000;
            else { NTL = drop_guard(N0L, (L.s_maskmb[0][SW][SI] - cbw) - MNR); act += n; }
            if (N0R < -2000) NTR = 10000;
            else { NTR = drop_guard(N0R, (L.s_maskmb[1][SW][SI] - cbw) - MNR); act += n; }
            int Nsum = MBLOG(ssum) - cbw, Ndiff = MBLOG(sdif) - cbw;
            int xNT = min(NTR, NTL) + 300, nt0 = xNT, nt1 = xNT;
            if (Ndiff < xNT) nt0 = logsubber(L, xNT, Ndiff) - 200;
            if (Nsum < xNT) nt1 = logsubber(L, xNT, Nsum) - 200;
            L.s_Noise0[0][SW][SI] = Nsum; L.s_Noise0[1][SW][SI] = Ndiff;
            L.s_NT[0][SW][SI] = nt0; L.s_NT[1][SW][SI] = nt1;
            L.s_snr[0][SW][SI] = Nsum - nt0; L.s_snr[1][SW][SI] = Ndiff - nt1;
        }
    }
    act = hx_wave_sum(act);
    if (LANE == 0) L.activeBands = act;
    HX_WAVE_SYNC();
    s_adjust_nt(L, p);
    s_pow34_gzero(L, p);
}

// reference bitallos.cpp:744-769
__device__ void s_seek_initial(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    if (SW < 3 && SI < p->nsfs)
        for (int ch = 0; ch < p->nchan; ch++) {
            float g4 = 0.017716950f * MBLOG(L.s_x34max[ch][SW][SI]) + (88.411238f - 100.0f + 8.0f);
            float d = (1.00f / 110.5f) * (1800 - (2 * 8) * SI - (L.s_Noise0[ch][SW][SI] - L.s_NT[ch][SW][SI]));
            float g = g4 + d;
            int gs = hx_round(g);
            gs = min(gs, L.s_gzero[ch][SW][SI]);
            gs = max(gs, L.s_gmin[ch][SW][SI]);
            L.s_gsf[ch][SW][SI] = gs;
        }
    HX_WAVE_SYNC();
}

// reference bitallos.cpp:772-898: gain walk, all bands of a channel in the same sweep
__device__ void s_seek_actual(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const bool band = SW < 3 && SI < p->nsfs;
    for (int ch = 0; ch < p->nchan; ch++) {
        int mode = 0, s = 0, t = 0, NTarget = 0, absmin = 0, tnmin = 0, smin = 0, iter = 0, niter = 0;
        if (band) {
            NTarget = L.s_NT[ch][SW][SI];
            s = L.s_gsf[ch][SW][SI];
            if (L.s_Noise0[ch][SW][SI] > NTarget) mode = 1;
            else { L.s_gsf[ch][SW][SI] = L.s_gzero[ch][SW][SI] + 5; L.s_Noise[ch][SW][SI] = L.s_Noise0[ch][SW][SI]; }
        }
        if (SW < 3) L.s_geval[SW][SI] = (mode == 1) ? s : -1;
        HX_WAVE_SYNC();
        while (__any(mode != 0)) {
            s_noise_sweep(L, p, ch);
            if (mode == 1) {
                int noise = L.s_tmpn[SW][SI], dn = noise - NTarget;
                absmin = abs(dn); tnmin = noise; smin = s; iter = 0;
                if (dn > 100) { t = s - 1; niter = min(t, 20); mode = (niter > 0) ? 2 : 0; }
                else if (dn < -100) { t = s + 1; niter = 20; mode = 3; }
                else mode = 0;
                if (mode == 0) { L.s_gsf[ch][SW][SI] = smin; L.s_Noise[ch][SW][SI] = tnmin; }
            } else if (mode == 2 || mode == 3) {
                int tn = L.s_tmpn[SW][SI], ad = abs(tn - NTarget);
                if (ad < absmin) { absmin = ad; tnmin = tn; smin = t; }
                iter++;
                bool stop = (mode == 2) ? (tn <= NTarget) : (tn >= NTarget);
                if (stop || iter >= niter) mode = 0;
                else t += (mode == 2) ? -1 : 1;
                if (mode == 0) { L.s_gsf[ch][SW][SI] = smin; L.s_Noise[ch][SW][SI] = tnmin; }
            }
            if (SW < 3) L.s_geval[SW][SI] = (mode != 0) ? t : -1;
            HX_WAVE_SYNC();
        }
    }
}

__device__ __forceinline__ int seg16_max(int v)
{
    // rotate inside the 16-lane DPP row: row_ror:8, 4, 2, 1
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
    return v;
}

// per-window gain (subblock_gain, steps of 8) and scalefactors (reference bitallos.cpp:1142-1276)
__device__ void s_scale_factors(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const bool band = SW < 3 && SI < p->nsfs;
    for (int ch = 0; ch < p->nchan; ch++) {
        int gsf = 0, gz = 0, act = 0;
        if (band) {
            gsf = max(L.s_gsf[ch][SW][SI], L.s_gmin[ch][SW][SI]);
            gz = L.s_gzero[ch][SW][SI];
            act = (gsf < gz) ? -1 : 0;
        }
        int Gw = seg16_max((band && act) ? gsf : -1);      // per window; lanes of window 3 give -1
        int G0 = __builtin_amdgcn_readlane(Gw, 0), G1 = __builtin_amdgcn_readlane(Gw, 16), G2 = __builtin_amdgcn_readlane(Gw, 32);
        int GG = max(max(G0, G1), G2);
        int sub = 0, G = Gw, sf = 0;
        if (Gw >= 0) {
            sub = min((GG - Gw) & (~7), 7 * 8);
            G = GG - sub;
            if (band && act) sf = G - gsf;
        } else if (band) gsf = gz;
        int sp0 = hx_wave_or((band && act && Gw >= 0) ? ((SI < 6 ? 31 : 15) - sf) : 0);
        const int scale = (sp0 >= 0) ? 0 : 1;
        if (band && Gw >= 0) {
            int noise = L.s_Noise[ch][SW][SI], nt = L.s_NT[ch][SW][SI];
            if (scale == 0) {
                if (noise > nt) sf++;
                sf = min(G, sf);
                sf &= (~1);
            } else {
                int s = sf & (~3), d = sf - s;
                int dN = noise - nt + 150 * d;
                if (dN > 250) { s = s + 4; s = min(G, s) & (~3); }
                sf = s;
            }
            int up = (SI < 6) ? (scale ? 60 : 30) : (scale ? 28 : 14);
            if (sf > up) sf = up; else if (sf < 0) sf = 0;
            if (act) {
                gsf = G - sf;
                if (gsf >= gz) { gsf = gz; sf = 0; }
            }
        }
        if (band) { L.s_gsf[ch][SW][SI] = gsf; L.s_sf[ch][SW][SI] = sf; L.s_active[ch][SW][SI] = act; }
        if (SW < 3 && SI == 0) { L.s_G[ch][SW] = G; L.s_subgain[ch][SW] = sub; }
        if (LANE == 0) { L.s_GG[ch] = GG; L.scale[ch] = scale; }
    }
    HX_WAVE_SYNC();
}

// reference bitallos.cpp:943-998: opt = first rounding offset replaced by -0.30
__device__ void s_do_quant(AllocLds &L, const AllocPrm *p, int opt)
{
    HX_LANE_DECL;
    const int nb = p->nbmax_s;
    if (SW < 3 && SI < 16) { L.s_ixmax[0][SW][SI] = 0; L.s_ixmax[1][SW][SI] = 0; }
    HX_WAVE_SYNC();
    for (int t = LANE; t < 1152; t += 64) {
        int c = t / 576, r = t - 576 * c, w = r / 192, j = r - 192 * w;
        if (j < nb) {
            int b = L.sband_of_line[j];
            float igain = LK_IGAIN(L.s_gsf[c][w][b]);
            int q;
            if (opt) {
                float tt = igain * L.x34[c][r] + (0.5f - 0.4375f);
                int iq = (int) tt;
                if (iq > 31) iq = 31;
                if (iq < 0) iq = 0;
                q = (int) (tt - (iq == 0 ? -.30f : L.quant_off[iq]));
            } else q = (int) (igain * L.x34[c][r] + (0.5f - 0.0946f));
            IX(c)[r] = q;
            if (q > 0) atomicMax(&L.s_ixmax[c][w][b], q);
        }
    }
    HX_WAVE_SYNC();
}

// reorder channel ch from [3][192] to sfb-major bitstream order into dst (int[576]); lines past
// the coded bands are zero
__device__ void s_reorder_ix(AllocLds &L, const AllocPrm *p, int ch, ix_t *dst)
{
    HX_LANE_DECL;
    const int nb = p->nbmax_s;
    for (int t = LANE; t < 576; t += 64) dst[t] = 0;
    HX_WAVE_SYNC();
    for (int t = LANE; t < 576; t += 64) {
        int w = t / 192, j = t - 192 * w;
        if (j < nb) {
            int b = L.sband_of_line[j], sb = L.startBand_s[b];
            dst[3 * sb + w * L.nBand_s[b] + (j - sb)] = IX(ch)[t];
        }
    }
    HX_WAVE_SYNC();
}

// reference bitallosc.cpp:296-428 on the reordered spectrum (pairs never straddle windows
// because every short sfb width is even)
__device__ int s_count_bits_ch(AllocLds &L, const AllocPrm *p, int ch)
{
    HX_LANE_DECL;
    ix_t *ixr = S_SCRATCH(ch);
    s_reorder_ix(L, p, ch, ixr);
    const int ncb = p->nsfs;
    int cb1, cb2, i;
    for (i = ncb - 1; i >= 0; i--) if (L.s_ixmax[ch][0][i] > 0 || L.s_ixmax[ch][1][i] > 0 || L.s_ixmax[ch][2][i] > 0) break;
    cb2 = i + 1;
    for (; i >= 0; i--) if (L.s_ixmax[ch][0][i] > 1 || L.s_ixmax[ch][1][i] > 1 || L.s_ixmax[ch][2][i] > 1) break;
    cb1 = max(i + 1, 3);
    cb2 = max(cb2, cb1);
    int r0 = 0, r1 = 0;
    for (i = 0; i < 3; i++) for (int w = 0; w < 3; w++) r0 = max(r0, L.s_ixmax[ch][w][i]);
    for (; i < cb1; i++) for (int w = 0; w < 3; w++) r1 = max(r1, L.s_ixmax[ch][w][i]);
    Cand c0 = candidates(L, r0), c1 = candidates(L, r1);
    const int n0 = 3 * L.startBand_s[3], nbig3 = 3 * L.startBand_s[cb1], nend = 3 * L.startBand_s[cb2];
    int r0a = 0, r0b = 0, r1a = 0, r1b = 0;
    for (int j = 2 * LANE; j < nbig3; j += 128) {
        const int x = ixr[j], y = ixr[j + 1];
        if (j < n0) acc_pair(L, c0, x, y, r0a, r0b);
        else acc_pair(L, c1, x, y, r1a, r1b);
    }
    const int nquads = ((nend - nbig3) + 3) >> 2;
    int qa = 0, qb = 0;
    for (int q = LANE; q < nquads; q += 64) {
        const ix_t *v = ixr + nbig3 + 4 * q;
        int pop = v[0] + v[1] + v[2] + v[3];
        qa += L.quada_len[((v[0] << 3) + (v[1] << 2) + (v[2] << 1) + v[3]) & 15] + pop;
        qb += 4 + pop;
    }
    r0a = hx_wave_sum(r0a); r0b = hx_wave_sum(r0b); r1a = hx_wave_sum(r1a); r1b = hx_wave_sum(r1b);
    int bits = 0, qidx = 0;
    const int tab0 = pick_table(c0, r0a, r0b, n0 > 0, &bits);
    const int tab1 = pick_table(c1, r1a, r1b, nbig3 - n0 > 0, &bits);
    qa = hx_wave_sum(qa);
    qb = hx_wave_sum(qb);
    if (nquads > 0) { if (qa < qb) { bits += qa; qidx = 0; } else { bits += qb; qidx = 1; } }
    if (LANE == 0) {
        L.hs_table[ch][0] = tab0; L.hs_table[ch][1] = tab1; L.hs_table[ch][2] = 0; L.hs_table[ch][3] = qidx;
        L.hs_cbreg[ch][0] = 3; L.hs_cbreg[ch][1] = cb1; L.hs_cbreg[ch][2] = cb2;
        L.hs_nbig[ch] = L.startBand_s[cb1]; L.hs_nquads[ch] = nquads; L.hs_bits[ch] = bits;
        L.huff_bits[ch] = bits;
    }
    HX_WAVE_SYNC();
    return bits;
}

__device__ int s_requant_count(AllocLds &L, const AllocPrm *p, int opt)
{
    s_scale_factors(L, p);
    s_do_quant(L, p, opt);
    int bits = s_count_bits_ch(L, p, 0);
    if (p->nchan == 2) bits += s_count_bits_ch(L, p, 1);
    return bits;
}

__device__ void s_bump_gsf(AllocLds &L, const AllocPrm *p, int delta, int only_over)
{
    HX_LANE_DECL;
    if (SW < 3 && SI < p->nsfs)
        for (int ch = 0; ch < p->nchan; ch++) {
            if (only_over && L.huff_bits[ch] <= PART23) continue;
            int g = L.s_gsf[ch][SW][SI];
            L.s_gsf[ch][SW][SI] = (delta < 0) ? max(g - 1, 0) : min(127, g + 1);
        }
    HX_WAVE_SYNC();
}

// CBitAlloShort::BitAllo (reference bitallos.cpp:202-369) for one granule, both channels.
// Inputs L.xr ([3][192] per channel), L.s_maskmb.  Outputs L.ix / L.signx in bitstream order,
// L.gr[igr][*], L.sfout_s.  Out of line: the frame loop's code stays small (short granules are the minority).
__device__ __noinline__ void bitallo_short(AllocLds &L, const AllocPrm *p, int igr, int min_bits, int target_bits,
                              int max_bits, int bit_pool, int ms, int MNR, sfo_t (*sfs)[3][12])
{
    HX_LANE_DECL;
    const int maxBits = min(4000 * p->nchan, max_bits);
    int minT = max(min_bits, 0);
    int maxT = target_bits + ((614 * bit_pool) >> 10);
    maxT = (maxBits + maxT) >> 1;
    maxT = min(maxBits, maxT);
    s_startup(L, p, ms, MNR);
    HxGr *g0 = &L.gr[igr][0];
    if (L.activeBands <= 0) {
        if (LANE < 2) {
            HxGr *g = g0 + LANE;
            g->global_gain = 0; g->window_switching_flag = 1; g->block_type = 2; g->mixed_block_flag = 0;
            g->preflag = g->scalefac_scale = 0;
            g->table_select[0] = g->table_select[1] = g->table_select[2] = 0;
            g->subblock_gain[0] = g->subblock_gain[1] = g->subblock_gain[2] = 0;
            g->big_values = g->region0_count = g->region1_count = g->count1table_select = 0;
            g->aux_nquads = g->aux_bits = g->aux_not_null = 0;
            g->aux_nreg[0] = g->aux_nreg[1] = g->aux_nreg[2] = 0;
        }
        for (int t = LANE; t < 72; t += 64) sfs[t / 36][(t % 36) / 12][t % 12] = 0;
        HX_WAVE_SYNC();
        return;
    }
    if (MNR < -200) minT = max(minT, (3 * target_bits) >> 2);
    s_seek_initial(L, p);
    s_seek_actual(L, p);
    int bits = s_requant_count(L, p, 1);
    if (bits < minT)
        for (int k = 0; k < 10; k++) {
            s_bump_gsf(L, p, -1, 0);
            bits = s_requant_count(L, p, 1);
            if (bits >= minT) break;
        }
    if (bits > maxT) {
        const int f = (250 * 1024) / (L.activeBands + 10);
        int deltaN = max((f * (bits - maxT)) >> 10, 40);
        for (int k = 0; k < 10; k++) {
            if (SW < 3 && SI < p->nsfs) { L.s_NT[0][SW][SI] += deltaN; L.s_NT[1][SW][SI] += deltaN; }
            HX_WAVE_SYNC();
            s_seek_actual(L, p);
            bits = s_requant_count(L, p, 0);
            if (bits <= maxT) break;
            deltaN = max((f * (bits - maxT)) >> 10, 40);
        }
    }
    if (bits > maxBits)
        for (int k = 0; k < 100; k++) {
            s_bump_gsf(L, p, 1, 0);
            bits = s_requant_count(L, p, 0);
            if (bits <= maxBits) break;
        }
    if (bits > PART23 && (L.huff_bits[0] > PART23 || L.huff_bits[1] > PART23))
        for (int k = 0; k < 100; k++) {
            s_bump_gsf(L, p, 1, 1);
            bits = s_requant_count(L, p, 0);
            if ((L.huff_bits[0] <= PART23) && (L.huff_bits[1] <= PART23)) break;
        }
    // side information
    if (LANE < 2) {
        const int c = LANE;
        HxGr *g = g0 + c;
        int GG = max(L.s_GG[c] - (ms ? 2 : 0), 0);
        g->global_gain = min(GG + (4 * 32 + 14), 255);
        g->window_switching_flag = 1; g->block_type = 2; g->mixed_block_flag = 0; g->preflag = 0;
        g->scalefac_scale = L.scale[c];
        g->aux_bits = L.huff_bits[c];
        g->aux_not_null = L.huff_bits[c];
        for (int w = 0; w < 3; w++) g->subblock_gain[w] = L.s_subgain[c][w] >> 3;
        if (L.hs_bits[c] <= 0) {
            g->table_select[0] = g->table_select[1] = g->table_select[2] = 0;
            g->big_values = g->region0_count = g->region1_count = 0;
            g->aux_nreg[0] = g->aux_nreg[1] = g->aux_nreg[2] = 0;
            g->aux_nquads = 0; g->count1table_select = 0;
        } else {
            g->table_select[0] = L.hs_table[c][0]; g->table_select[1] = L.hs_table[c][1]; g->table_select[2] = 0;
            g->count1table_select = L.hs_table[c][3];
            g->big_values = 3 * (L.hs_nbig[c] >> 1);
            g->region0_count = g->region1_count = 0;
            int n0 = L.startBand_s[3], n1 = L.startBand_s[L.hs_cbreg[c][1]], n2 = L.startBand_s[L.hs_cbreg[c][2]];
            if (n2 > L.hs_nbig[c]) n2 = L.hs_nbig[c];
            if (n1 > n2) n1 = n2;
            if (n0 > n1) n0 = n1;
            n2 = n2 - n1; n1 = n1 - n0;
            g->aux_nreg[0] = 3 * (n0 >> 1); g->aux_nreg[1] = 3 * (n1 >> 1); g->aux_nreg[2] = 3 * (n2 >> 1);
            g->aux_nquads = L.hs_nquads[c];
        }
    }
    // scalefactors out (>> 1 or >> 2), zero past the coded bands
    for (int t = LANE; t < 72; t += 64) {
        int c = t / 36, w = (t % 36) / 12, i = t % 12;
        sfs[c][w][i] = (i < p->nsfs) ? (L.s_sf[c][w][i] >> (L.scale[c] == 0 ? 1 : 2)) : 0;
    }
    HX_WAVE_SYNC();
    // spectrum and signs to bitstream order: only up to the end of the count1 region is kept
    for (int ch = 0; ch < p->nchan; ch++) {
        ix_t *tmp = S_SCRATCH(ch);
        s_reorder_ix(L, p, ch, tmp);
        const int nend = 3 * L.startBand_s[L.hs_cbreg[ch][2]];
        unsigned char *stmp = (unsigned char *) &L.x34[ch][0];     // x34 is dead after the last quantisation
        for (int t = LANE; t < 576; t += 64) stmp[t] = 0;
        HX_WAVE_SYNC();
        for (int t = LANE; t < 576; t += 64) {
            int w = t / 192, j = t - 192 * w;
            if (j < p->nbmax_s) {
                int b = L.sband_of_line[j], sb = L.startBand_s[b];
#if HX_SLIM
                stmp[3 * sb + w * L.nBand_s[b] + (j - sb)] = (unsigned char) ((L.sgnbits[ch][t >> 6] >> (t & 63)) & 1);
#else
                stmp[3 * sb + w * L.nBand_s[b] + (j - sb)] = L.signx[ch][t];
#endif
            }
        }
        HX_WAVE_SYNC();
        for (int t = LANE; t < 576; t += 64) {
            IX(ch)[t] = (t < nend) ? tmp[t] : 0;
#if !HX_SLIM
            L.signx[ch][t] = stmp[t];       // (the low-footprint layout hands the signs over from where they are)
#endif
        }
        HX_WAVE_SYNC();
    }
}

// short scalefactors (reference l3pack.c:218-288): 12 sfb x 3 windows, slen1 below sfb 6
__device__ int pack_sf_short(AllocLds &L, int pos, sfo_t (*sfs)[12], int not_null, int *sc_out, int *field)
{
    HX_LANE_DECL;
    *sc_out = 0;
    if (!not_null) return pos;
    const int f = LANE, i = f / 3, w = f - 3 * i;
    const bool on = f < 36;
    int v = on ? sfs[w][i] : 0;
    int m1 = hx_wave_max((on && i < 6) ? v : 0), m2 = hx_wave_max((on && i >= 6) ? v : 0);
    int s1, s2;
    *sc_out = sf_compress(m1, m2, &s1, &s2);
    int len = on ? (i < 6 ? s1 : s2) : 0;
    *field = len ? ((len << 8) | v) : 0;
    return pos + hx_wave_sum(len);
}
