// hx_alloc2.inc - second half of the K6 allocator kernel (included by hx_alloc.hip):
// -HF band handling, rate loop, scalefactor refinement, MNR feedback, bitstream packing and
// reservoir / frame assembly (the kernel entry point is in hx_alloc3.inc).

// ---- -HF support (reference bitallo3.cpp:1635-1737, 2421-2563) ----
__device__ HX_HFN void clear_hf(AllocLds &L, int nch)
{
    HX_LANE_DECL;
    for (int ch = 0; ch < nch; ch++)
        for (int j = LANE; j < L.nBand[21]; j += 64) IX(ch)[L.startBand[21] + j] = 0;
    HX_WAVE_SYNC();
}

// quantise band 21 at the global gain with the first rounding offset replaced (l3math.c:698-727)
__device__ HX_HFN void quant_hf_ch(AllocLds &L, int ch, int sparse)
{
    HX_LANE_DECL;
    const int o = L.startBand[21], n = L.nBand[21];
    if (LANE == 0) L.ixmax[ch][21] = 0;
    HX_WAVE_SYNC();
    const float igain = LK_IGAIN(L.G[ch]);
    for (int j = LANE; j < n; j += 64) {
        float t = igain * L.x34[ch][o + j] + (0.5f - 0.4375f);
        int iq = (int) t;
        if (iq > 31) iq = 31;
        if (iq < 0) iq = 0;
        int q = (int) (t - (iq == 0 ? -.30f : L.quant_off[iq]));
        IX(ch)[o + j] = q;
        if (q > 0) atomicMax(&L.ixmax[ch][21], q);
    }
    HX_WAVE_SYNC();
    if (sparse) {       // sparse_quad_counted(qx, n, 4): serial, rare
        if (LANE == 0) {
            ix_t *qx = IX(ch) + o;
            int c = 0, scnt = 0;
            for (int i = 0; i < n; i++) c += qx[i];
            c = (4 * c) >> 4;
            if (c > 0)
                for (int i = n - 4; i >= 0; i -= 4) {
                    int m = qx[i] + qx[i + 1] + qx[i + 2] + qx[i + 3];
                    if (m == 1) {
                        qx[i] = qx[i + 1] = qx[i + 2] = qx[i + 3] = 0;
                        scnt++;
                        if (scnt >= c) break;
                    }
                }
        }
        HX_WAVE_SYNC();
    }
}

// can band 21 ride on the global gain?  uniform result; lane 0 applies the gsf clamp
__device__ HX_HFN int hf_adjust_ch(AllocLds &L, const AllocPrm *p, int ch, int *gsf_hf_out)
{
    HX_LANE_DECL;
    int res = 0, gout = -1;
    if (L.gzero[ch][21] > 8) {
        int gmax0 = 0, gmax1 = 0;
        for (int i = 0; i < 11; i++) if (L.gsf[ch][i] < L.gzero[ch][i] && L.gsf[ch][i] > gmax0) gmax0 = L.gsf[ch][i];
        for (int i = 11; i < p->nsf[ch]; i++) if (L.gsf[ch][i] < L.gzero[ch][i] && L.gsf[ch][i] > gmax1) gmax1 = L.gsf[ch][i];
        int gtar = max(0, L.gzero[ch][21] - 5), gtar2 = max(0, L.gzero[ch][21] - 7), gmax = max(gmax0, gmax1);
        if (gtar >= gmax) { gout = gtar2; res = 1; }
        else if (gmax0 > gmax1) {
            int gset = max(gtar, gmax1);
            if (L.gzero[ch][21] > gset) {
                HX_WAVE_SYNC();     // everyone has read gsf before lane 0 edits it
                if (LANE == 0)
                    for (int i = 0; i < 11; i++)
                        if (L.gsf[ch][i] < L.gzero[ch][i] && L.gsf[ch][i] > gset) L.gsf[ch][i] = gset;
                res = 1;
            }
        }
    }
    HX_WAVE_SYNC();
    *gsf_hf_out = gout;
    return res;
}

__device__ HX_HFN void hf_adjust(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    int g0 = -1, g1 = -1;
    int r0 = hf_adjust_ch(L, p, 0, &g0);
    int r1 = hf_adjust_ch(L, p, 1, &g1);
    if (LANE == 0) {
        L.gsf_hf_stereo[0] = g0; L.gsf_hf_stereo[1] = g1;
        if (r0) L.hf_quant_stereo[0] = 1;
        if (r1) L.hf_quant_stereo[1] = 1;
        L.hf_quant = L.hf_quant_stereo[0] | L.hf_quant_stereo[1];
    }
    HX_WAVE_SYNC();
}

__device__ HX_HFN void hf_adjust_ms(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    int g0 = -1;
    int r0 = hf_adjust_ch(L, p, 0, &g0);
    if (LANE == 0 && r0) { L.hf_quant = 1; if (g0 >= 0) L.gsf_hf = g0; }
    HX_WAVE_SYNC();
}

__device__ HX_HFN void hf_reset_lr(AllocLds &L)
{
    HX_LANE_DECL;
    if (LANE == 0) {
        L.hf_quant = 0;
        L.hf_quant_stereo[0] = L.hf_quant_stereo[1] = 0;
        L.gsf_hf_stereo[0] = L.gsf_hf_stereo[1] = -1;
        L.ixmax[0][21] = L.ixmax[1][21] = 0;
    }
    HX_WAVE_SYNC();
}
__device__ HX_HFN void hf_reset_ms(AllocLds &L, int both)
{
    HX_LANE_DECL;
    if (LANE == 0) {
        L.hf_quant = 0;
        L.ixmax[0][21] = 0;
        if (both) L.ixmax[1][21] = 0;
        L.gsf_hf = -1;
    }
    HX_WAVE_SYNC();
}

// ---- trade_dual (L/R only; reference bitallo3.cpp:2216-2306): flatten isolated peaks ----
__device__ HX_COLD float dblog(float x) { return (float) (10.0 * log10((double) x)); }
// the gain step (before its + 8) at which a band whose largest x^(3/4), scaled by the target's factor, is x quantises to the target
__device__ __forceinline__ int dual_gain_step(float x)
{
    float xg = 1.7717f * dblog(x);
    return (int) (xg + 1.0f);
}

__device__ void trade_dual(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, i = LANE & 31;
    if (i < p->nsf[ch]) {       // l3math.c:753-793
        float t = LK_IGAIN(L.gsf[ch][i]) * L.x34max[ch][i] + (0.5f - 0.4375f);
        int iq = (int) t;
        if (iq > 31) iq = 31;
        L.ixmax[ch][i] = (int) (t - L.quant_off[iq]);
        L.ix10xmax[ch][i] = (int) (10.0f * (t - L.quant_off[iq]) + (0.5f - 5.0f));
    }
    HX_WAVE_SYNC();
    if (i == 0) {       // one lane per channel runs the short serial scan
        // target_table = {0, 1, 2, 3, 3, 5, 5, 7, 7, 7, 7, 15, 15, 15, 15, 15} as nibbles; of the rounding offsets qo[16] =
        // {0.09460, 0.02799, 0.01671, 0.01192, 0.00927, 0.00758, 0.00641, 0.00556, ..., 0.00269} only the entries a
        // target can index are left.  (As arrays they were two dependent loads from global memory per L/R granule.)
        const unsigned long long target_nibbles = 0xFFFFF77775533210ull;
        int b, g, k0, k1;
        for (b = p->nsf[ch] - 1; b >= 11; b--) {
            if (L.ix10xmax[ch][b] > 16) break;
            if (L.ixmax[ch][b] == 2) {
                g = dual_gain_step(L.x34max[ch][b] * (1.0f / (1.5f + 0.02799f)));
                L.gsf[ch][b] = g + 8;
            }
        }
        k1 = b + 1;
        k0 = (3 * k1) >> 2;
        if (k0 < 11) k0 = 11;
        if (k1 >= 9 && k0 < k1) {
            int ixmax0 = 0;
            for (b = k0; b < k1; b++) if (L.ixmax[ch][b] > ixmax0) ixmax0 = L.ixmax[ch][b];
            if (ixmax0 > 2) {
                float fetot = 0, feixmax = 0;
                for (b = k0; b < k1; b++) {
                    float ftmp = p->rnBand_l[b] * L.xsxx[ch][b];
                    fetot += ftmp;
                    feixmax += ftmp * L.ix10xmax[ch][b];
                }
                float eixmax = feixmax / (1.0f + fetot);
                int ixtarget = (int) (0.1f * eixmax + 0.65f);
                if (ixtarget < 2) ixtarget = 2;
                if (ixmax0 > ixtarget && ixtarget <= 15) {
                    ixtarget = (int) ((target_nibbles >> (4 * ixtarget)) & 15);
                    const float qo = (ixtarget == 2) ? 0.01671f : (ixtarget == 3) ? 0.01192f : (ixtarget == 5) ? 0.00758f : (ixtarget == 7) ? 0.00556f : 0.00269f;
                    float factor = 1.0f / ((ixtarget + 0.5f) + qo);
                    for (b = k0; b < k1; b++)
                        if (L.ixmax[ch][b] > ixtarget) {
                            g = dual_gain_step(L.x34max[ch][b] * factor);
                            L.gsf[ch][b] = g + 8;
                        }
                }
            }
        }
    }
    HX_WAVE_SYNC();
}

// ---- rate loop pieces ----
// HF: 1 = the step towards more bits, with the HF handling and the table-offset quantiser (increase_bits); 0 = plain
// (decrease_bits, limit_bits).  A template parameter, so each copy holds its own quantiser only, with a literal opt.
template <int HF>
__device__ HX_RATE int requant_count(AllocLds &L, const AllocPrm *p, int ms)
{
    HX_LANE_DECL;
    if (HF) {
        if (ms) {
            hf_reset_ms(L, 0);
            // (without -HF nothing ever writes the lines of band 21 beyond what the quantiser below rewrites: clearing
            // them - reference bitallo3.cpp:2673 clear_hf_main - changes nothing)
            if (p->hf_flag) { clear_hf(L, 1); hf_adjust_ms(L, p); }
            scale_factors(L, p, 1);
            if (!L.hf_quant) return quant_count_bits(L, p, 1, 1, p->nsf2);     // one hand-over to the helper wave instead of two
            do_quant(L, p, 1);
            if (LANE == 0) L.ixmax[0][21] = 0;
            HX_WAVE_SYNC();
            quant_hf_ch(L, 0, 0);
            return count_bits(L, p, p->nsf2);
        }
        if (p->hf_flag & 2) { hf_reset_lr(L); hf_adjust(L, p); }
        scale_factors(L, p, 0);
        // (1 | 2: lines past the coded range stay as they are.  The reference does not clear band 21 on this path
        // - bitallo3.cpp:2636-2668 - so the lines of an earlier -HF pass survive a pass without one, out of the counted
        // range except for the last quadruple, which can reach up to three lines into them)
        if (!L.hf_quant) return quant_count_bits(L, p, 1 | 2, 0, p->nsf3);
        do_quant(L, p, 1 | 2);
        if (L.hf_quant_stereo[0]) quant_hf_ch(L, 0, 1);
        if (L.hf_quant_stereo[1]) quant_hf_ch(L, 1, 1);
        return count_bits(L, p, p->nsf3);
    }
    scale_factors(L, p, 0);
    return quant_count_bits(L, p, 0, 0, p->nsf2);
}

// reference bitallo3.cpp:2569-2722
__device__ HX_RATE int increase_bits(AllocLds &L, const AllocPrm *p, int bits0, int ms)
{
    HX_LANE_DECL;
    const int thres = L.minTargetBits - (L.minTargetBits >> 4);
    if (bits0 > thres) return bits0;
    const int ch = LANE >> 5, i = LANE & 31;
    const bool band = i < p->nsf[ch];
    int g = band ? L.gsf[ch][i] : 0, bits = bits0;
    for (int k = 0; k < 10; k++) {
        if (band) { g = max(g - 1, L.gmin[ch][i]); L.gsf[ch][i] = g; }
        HX_WAVE_SYNC();
        bits = requant_count<1>(L, p, ms);
        if (bits >= thres) break;
    }
    if (bits > L.maxTargetBits) {       // went too far: step back once
        if (band) L.gsf[ch][i] = g + 1;
        HX_WAVE_SYNC();
        bits = requant_count<1>(L, p, ms);
    }
    return bits;
}

// reference bitallo3.cpp:2814-2855
__device__ HX_RATE int decrease_bits(AllocLds &L, const AllocPrm *p, int bits0)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, i = LANE & 31;
    const bool band = i < p->nsf[ch];
    const int f = (250 * 1024) / (L.activeBands + 10);
    int deltaN = max((f * (bits0 - L.maxTargetBits)) >> 10, 40), bits = bits0, dmnr = 0;
    for (int k = 0; k < 10; k++) {
        dmnr += deltaN;
        if (band) L.NT[ch][i] += deltaN;
        HX_WAVE_SYNC();
        seek_actual(L, p);
        bits = requant_count<0>(L, p, 0);
        if (bits <= L.maxTargetBits) break;
        deltaN = max((f * (bits - L.maxTargetBits)) >> 10, 40);
    }
    if (LANE == 0) L.deltaMNR = dmnr;
    HX_WAVE_SYNC();
    return bits;
}

// reference bitallo3.cpp:2725-2773
__device__ HX_RATE int limit_bits(AllocLds &L, const AllocPrm *p, int part23)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, i = LANE & 31;
    const bool band = i < p->nsf[ch];
    int bits = 0;
    for (int k = 0; k < 100; k++) {
        if (band && !(part23 && L.huff_bits[ch] <= PART23)) L.gsf[ch][i] = min(127, L.gsf[ch][i] + 1);
        HX_WAVE_SYNC();
        bits = requant_count<0>(L, p, 0);
        if (part23) { if ((L.huff_bits[0] <= PART23) && (L.huff_bits[1] <= PART23)) break; }
        else if (bits <= L.maxBits) break;
    }
    return bits;
}

// squared quantised / original magnitudes of channel c's lines (inverse_sf2's sums run over them)
__device__ __forceinline__ void isf2_lines(AllocLds &L, const AllocPrm *p, int c)
{
    HX_LANE_DECL;
    const int nl = p->nbmax[c];
    float q[9], x[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int j = LANE + 64 * k;
        q[k] = L.look_ix43[min((unsigned) IX(c)[j], 255u)];
        x[k] = L.xr[c][j];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int j = LANE + 64 * k;
#if HX_SLIM
        if (j < nl) { L.x34[c][j] = q[k] * q[k]; L.xr[c][j] = x[k] * x[k]; }       // (the term buffer holds the lines; the spectrum is dead behind this)
#else
        if (j < nl) { L.term[c][j] = q[k] * q[k]; L.x34[c][j] = x[k] * x[k]; }
#endif
    }
}

// The lane's share of inverse_sf2's two band sums of channel c - squares of the quantised magnitudes (x^(4/3) of the
// line's value: a selected band only holds 0, 1 and 2, so the table always covers it) and of the original ones - over its run
// of lines (hx_dev.h, "certified band sums").
// (all RUNW_MAX / 2 pairs whatever the class's run width, as in sweep_load: a guard on the run-time W would split the
// loop into blocks that each wait for their own line words and then for their own table reads)
__device__ __forceinline__ void isf2_run(AllocLds &L, const LaneRun &q, int c, float *sq, float *sx)
{
    float tq[RUNW_MAX], tx[RUNW_MAX];
#pragma unroll
    for (int k = 0; k < RUNW_MAX; k += 2) {
        const int j = min(q.start + k, 576 - 2);
#if HX_SLIM
        const unsigned w = *reinterpret_cast<const unsigned *>(IX(c) + j);
        const unsigned i0 = w & 0xFFFFu, i1 = w >> 16;
#else
        const int2 w = *reinterpret_cast<const int2 *>(IX(c) + j);
        const unsigned i0 = (unsigned) w.x, i1 = (unsigned) w.y;
#endif
        const float2 x = *reinterpret_cast<const float2 *>(&L.xr[c][j]);
        const float q0 = L.look_ix43[min(i0, 255u)], q1 = L.look_ix43[min(i1, 255u)];
        const bool in = k < q.cnt;
        tq[k] = in ? q0 * q0 : 0.0f; tq[k + 1] = in ? q1 * q1 : 0.0f;
        tx[k] = in ? x.x * x.x : 0.0f; tx[k + 1] = in ? x.y * x.y : 0.0f;
    }
    *sq = (((tq[0] + tq[1]) + (tq[2] + tq[3])) + ((tq[4] + tq[5]) + (tq[6] + tq[7]))) + (tq[8] + tq[9]);
    *sx = (((tx[0] + tx[1]) + (tx[2] + tx[3])) + ((tx[4] + tx[5]) + (tx[6] + tx[7]))) + (tx[8] + tx[9]);
}

// inverse_sf2 for one channel, run by one wave (band lane = sfb): the two sums of a selected band feed mbLogC(sxx / sqq)
// only, so every lane adds the squares of its run of lines, a segmented scan leaves the band totals in the band's last lane,
// and the band lane certifies the quotient's bucket; a band whose interval straddles a bucket boundary is added strictly
// (squares line-parallel into LDS, the band lane adds them in line order).
__device__ void isf2_ch(AllocLds &L, const AllocPrm *p, int ch)
{
    HX_LANE_DECL;
    const int i = LANE, ib = min(i, NB - 1);
    const int ixm = L.ixmax[ch][ib];
    const bool sel = (i < p->nsf[ch]) && ((ixm == 1) || (ixm == 2));
    if (!__any(sel)) return;
    const int W = p->run_w;
    const LaneRun q = lane_run(L);
    const int last4 = 4 * (int) L.band_last[ib];
    float sqq, sxx;
    isf2_run(L, q, ch, &sqq, &sxx);
    sqq = hx_lane_read(last4, hx_seg_scan(sqq, q.d, LANE));
    sxx = hx_lane_read(last4, hx_seg_scan(sxx, q.d, LANE));
    bool strict = false;
    if (sel) strict = (p->oflags & 8) || !hx_cert_mblog_ratio(sxx, sqq, hx_cert_delta(L.nBand[ib], W));
    if (__builtin_expect(__any(strict), 0)) {
        // (x34 is dead after the last quantisation and serves as scratch; every line below nbmax gets its terms, selected
        // band or not: unread garbage is cheaper than a predicate)
        if (LANE == 0) atomicAdd(&L.nstrict, 1);
        isf2_lines(L, p, ch);
        HX_WAVE_SYNC();
        if (strict) {
#if HX_SLIM
            band_sum2(&L.x34[ch][L.startBand[ib]], &L.xr[ch][L.startBand[ib]], L.nBand[ib], &sqq, &sxx);
#else
            band_sum2(&L.term[ch][L.startBand[ib]], &L.x34[ch][L.startBand[ib]], L.nBand[ib], &sqq, &sxx);
#endif
        }
    }
    if (sel) {
        int t = 54 * MBLOG(sxx / sqq) + (8 << 13);
        int sh = L.scale[ch] ? 14 : 13;
        int s = (((L.G[ch] << 13) - t + (1 << sh)) & (~((1 << (sh + 1)) - 1))) >> 13;
        s = min(s, L.up[ch][ib]);
        s = max(s, L.lo[ch][ib]);
        L.sf[ch][ib] = s;
    }
}

// reference bitallo3.cpp:1471-1536 with l3math.c:1088-1114
__device__ void inverse_sf2(AllocLds &L, const AllocPrm *p)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, i = LANE & 31;
    const bool sel = (i < p->nsf[ch]) && ((L.ixmax[ch][i] == 1) || (L.ixmax[ch][i] == 2));
    if (i < NB) L.geval[ch][i] = sel ? 1 : -1;
    if (!__any(sel)) { HX_WAVE_SYNC(); return; }
    HX_WAVE_SYNC();
    const bool two = p->nbmax[1] > 0;
    if (two) HELPER_POST(HCMD_ISF2, 0);             // channel 1 on the helper wave
    isf2_ch(L, p, 0);
    if (two) HELPER_JOIN();
    HX_WAVE_SYNC();
}

// reference bitallo3.cpp:2948-3046 (ms = 0) / 3048-3149 (ms = 1)
__device__ int allocate(AllocLds &L, const AllocPrm *p, int ms)
{
    HX_LANE_DECL;
    int bits, bits0;
    if (p->hf_flag) {
        if (ms) hf_reset_ms(L, 1); else hf_reset_lr(L);
        clear_hf(L, 2);
    }
    PROF(HX_PROF_SEEK_INITIAL, seek_initial(L, p));
    PROF(HX_PROF_SEEK_ACTUAL, seek_actual(L, p));
    if (ms) { if (p->hf_flag) hf_adjust_ms(L, p); }
    else { PROF(HX_PROF_TRADE_DUAL, trade_dual(L, p)); if (p->hf_flag & 2) hf_adjust(L, p); }
    PROF(HX_PROF_SCALE_FACTORS, scale_factors(L, p, ms));
    PROF(HX_PROF_BIG_LUCKY, big_lucky_noise(L, p));
    if (!L.hf_quant) PROF(HX_PROF_QUANT_COUNT, bits0 = bits = quant_count_bits(L, p, 1, ms, ms ? p->nsf2 : p->nsf3));
    else {
        PROF(HX_PROF_DO_QUANT, do_quant(L, p, 1));
        if (ms) {
            if (LANE == 0) L.ixmax[0][21] = 0;
            HX_WAVE_SYNC();
            if (L.hf_quant) quant_hf_ch(L, 0, 0);
            PROF(HX_PROF_QUANT_COUNT, bits0 = bits = count_bits(L, p, p->nsf2));
        } else {
            if (L.hf_quant) { if (L.hf_quant_stereo[0]) quant_hf_ch(L, 0, 1); if (L.hf_quant_stereo[1]) quant_hf_ch(L, 1, 1); }
            PROF(HX_PROF_QUANT_COUNT, bits0 = bits = count_bits(L, p, p->nsf3));
        }
    }
    if (bits < L.minTargetBits && L.MNR < 2000) PROF(HX_PROF_INCREASE_BITS, bits = increase_bits(L, p, bits, ms));
    if (ms) hf_reset_ms(L, 0);
    else if (p->hf_flag) hf_reset_lr(L);
    if (bits > L.maxTargetBits) { clear_hf(L, ms ? 1 : 2); PROF(HX_PROF_DECREASE_BITS, bits = decrease_bits(L, p, bits)); }
    if (bits > L.maxBits) { clear_hf(L, ms ? 1 : 2); bits = limit_bits(L, p, 0); }
    if (bits > PART23 && (L.huff_bits[0] > PART23 || L.huff_bits[1] > PART23)) { clear_hf(L, ms ? 1 : 2); bits = limit_bits(L, p, 1); }
    PROF(HX_PROF_INVERSE_SF2, inverse_sf2(L, p));
    return bits0;
}

// reference bitallo3.cpp:2897-2944 (lane 0; mixed float/double arithmetic as written there)
__device__ void mnr_feedback(AllocLds &L, const AllocPrm *p, int activeBands, int bits)
{
    HX_LANE_DECL;
    if (LANE == 0 && L.call_count > 10) {
        float deltaNB = 150.0f / (0.20f * (activeBands + 10));
        int mnr = (int) (0.05 * deltaNB * (bits - L.TargetBits));
        int mnr2 = (int) (0.05 * deltaNB * max((bits - L.maxBits), 0));
        int dPool = max(L.TargetBits - bits, 0);
        int dBits = (((2044 + 8 * 5) - L.PoolBits) >> 4) - dPool;
        dBits = max(dBits, 0);
        dBits = min(dBits, 200);
        int mnrp = (int) (deltaNB * dBits);
        int mnr0 = (int) (0.2 * deltaNB * max((L.minTargetBits - bits), 0));
        int dmnr = mnr + mnr2 + mnrp - mnr0;
        int maxdmnr = max(L.MNR - p->initialMNR, L.TargetBits >> 3);
        dmnr = min(dmnr, maxdmnr);
        if (L.deltaMNR) dmnr = max(dmnr, (L.deltaMNR >> 1));
        int M = L.MNR - dmnr;
        M = min(M, 2000);
        if (bits > (L.TargetBits + 2000)) M = min(M, p->initialMNR);
        L.MNR = M;
    }
    HX_WAVE_SYNC();
}

// reference bitalloc.cpp:758-811
__device__ void huffsel_to_gr(AllocLds &L, int ch, HxGr *g)
{
    if (L.hs_bits[ch] <= 0) {
        g->table_select[0] = g->table_select[1] = g->table_select[2] = 0;
        g->big_values = g->region0_count = g->region1_count = 0;
        g->aux_nreg[0] = g->aux_nreg[1] = g->aux_nreg[2] = 0;
        g->aux_nquads = 0;
        g->count1table_select = 0;
        return;
    }
    g->table_select[0] = L.hs_table[ch][0];
    g->table_select[1] = L.hs_table[ch][1];
    g->table_select[2] = L.hs_table[ch][2];
    g->count1table_select = L.hs_table[ch][3];
    g->big_values = L.hs_nbig[ch] >> 1;
    g->region0_count = L.hs_cbreg[ch][0] - 1;
    g->region1_count = max((L.hs_cbreg[ch][1] - L.hs_cbreg[ch][0]) - 1, 0);
    int n0 = L.startBand[L.hs_cbreg[ch][0]], n1 = L.startBand[L.hs_cbreg[ch][1]], n2 = L.startBand[L.hs_cbreg[ch][2]];
    if (n2 > L.hs_nbig[ch]) n2 = L.hs_nbig[ch];
    if (n1 > n2) n1 = n2;
    if (n0 > n1) n0 = n1;
    n2 = n2 - n1;
    n1 = n1 - n0;
    g->aux_nreg[0] = n0 >> 1;
    g->aux_nreg[1] = n1 >> 1;
    g->aux_nreg[2] = n2 >> 1;
    g->aux_nquads = L.hs_nquads[ch];
}

// CBitAllo3::BitAllo for one long-block granule, both channels (reference bitallo3.cpp:484-678).
// Inputs: L.xr, L.maskmb; outputs L.ix, L.signx, L.gr[igr][*], L.sfout[igr][*].
// fetch_g / fetch_next >= -1: granule number and successor for the helper wave's HCMD_FETCH order, which goes out as soon
// as the lines are final (the rest of this function does not touch them); returns whether it went out.
__device__ bool bitallo_long(AllocLds &L, const AllocPrm *p, int igr, int block_type,
                             int min_bits, int target_bits, int max_bits, int bit_pool, int ms, const BandIn &bin, int fetch_g, int fetch_next)
{
    HX_LANE_DECL;
    if (LANE == 0) {
        L.block_type = block_type;
        L.call_count++;
        L.deltaMNR = 0;
        if (block_type == 1) {
            if (L.MNR > p->initialMNR) { L.MNR = (L.MNR + p->initialMNR) >> 1; L.MNR = min(L.MNR, p->initialMNR + 500); }
        } else if (block_type == 3) {
            L.MNR = (L.MNR + p->initialMNR) >> 1;
            L.MNR = min(L.MNR, p->initialMNR + 500);
        }
        int maxBits = min(4000 * p->nchan, max_bits);
        int minT = max(min_bits, 0);
        if (p->vbr_flag == 0) {
            L.PoolFraction = min(L.PoolFraction + 50, 614);
            if (block_type != 0) L.PoolFraction = 0;
        }
        int tbits = ((L.PoolFraction * bit_pool) >> 10);
        if (p->vbr_flag == 0) tbits = min(tbits, max((2050 - 500) + p->initialMNR - L.MNR, 200));
        int maxT = min(maxBits, target_bits + tbits);
        if (L.MNR < -200) minT = max(minT, (3 * target_bits) >> 2);
        maxT = max(minT, maxT);
        minT = min(minT, maxT - 100);
        L.maxBits = maxBits; L.minTargetBits = minT; L.maxTargetBits = maxT;
        L.TargetBits = target_bits; L.PoolBits = bit_pool;
    }
    if (!HX_SLIM && block_type == 3) for (int j = LANE; j < 1152; j += 64) IX(0)[j] = 0;     // (low-footprint layout: the quantiser writes every line)
    HX_WAVE_SYNC();
    PROF(HX_PROF_STARTUP, startup_prepped(L, p, ms, bin));

    HxGr *g0 = &L.gr[igr][0];
    if (L.activeBands <= 0) {
        if (LANE < 2) {
            HxGr *g = g0 + LANE;
            g->global_gain = 0;
            g->window_switching_flag = (block_type != 0);
            g->block_type = block_type;
            g->mixed_block_flag = 0;
            g->preflag = g->scalefac_scale = 0;
            g->table_select[0] = g->table_select[1] = g->table_select[2] = 0;
            g->big_values = g->region0_count = g->region1_count = g->count1table_select = 0;
            g->aux_nquads = g->aux_bits = g->aux_not_null = 0;
            g->aux_nreg[0] = g->aux_nreg[1] = g->aux_nreg[2] = 0;
        }
        if (LANE < 44) L.sfout[igr][LANE / 22][LANE % 22] = 0;
        HX_WAVE_SYNC();
        return false;
    }
    int fb = allocate(L, p, ms);
    // The quantised lines are final and the spectrum is dead: the helper wave takes the lines out and fetches the next
    // granule's operands while the feedback, the scalefactor output and the side-information fields are done here.
    // (order word 3: block type | channel c's segment is not empty << (8 + c))
    if (LANE == 0) { L.cmdw[2] = fetch_g; L.cmdw[3] = block_type | ((L.huff_bits[0] != 0) << 8) | ((L.huff_bits[1] != 0) << 9); }
    HELPER_POST(HCMD_FETCH, fetch_next);
    if (p->vbr_flag == 0) mnr_feedback(L, p, L.activeBands, fb);

    // output_sf (reference bitallo3.cpp:760-812)
    {
        const int ch = LANE >> 5, i = LANE & 31;
        if (i < NB) {
            int s = 0;
            if (i < p->nsf[ch]) {
                s = L.sf[ch][i] >> (L.scale[ch] == 0 ? 1 : 2);
                if (L.preemp[ch] && i >= 11) s -= pretab(i);
            }
            L.sfout[igr][ch][i] = (i < 21) ? s : 0;
        }
    }
    if (LANE < 2) {
        const int c = LANE;
        HxGr *g = g0 + c;
        int G = L.G[c] - (ms ? 2 : 0);
        g->global_gain = min(G + (4 * 32 + 14), 255);
        g->window_switching_flag = (block_type != 0);
        g->block_type = block_type;
        g->mixed_block_flag = 0;
        g->preflag = L.preemp[c];
        g->scalefac_scale = L.scale[c];
        g->aux_bits = L.huff_bits[c];
        g->aux_not_null = L.huff_bits[c];
        huffsel_to_gr(L, c, g);
    }
    HX_WAVE_SYNC();
    return true;
}

// ---- packing (reference l3pack.c:157-214, 421-558, 946-1119) ----
__device__ __forceinline__ int sf_compress(int sfmax1, int sfmax2, int *slen1, int *slen2)
{
    // The ISO tables as nibble-packed immediates (indexed local arrays would be memory loads):
    // comp[s1][s2] = {0,1,2,3},{5,5,6,7},{8,8,9,10},{4,11,12,13},{14,14,14,15};
    // slen[sc] = (0,0)(0,1)(0,2)(0,3)(3,0)(1,1)(1,2)(1,3)(2,1)(2,2)(2,3)(3,1)(3,2)(3,3)(4,2)(4,3)
    // s = bits needed for the group's largest value (only its bit length matters), capped at 4 / 3
    const int s1 = min(32 - __clz(sfmax1), 4), s2 = min(32 - __clz(sfmax2), 3);
    // comp rows for s1 = 0..4 as 16-bit immediates, picked with selects (a variable 64-bit shift costs more)
    const unsigned row = s1 == 0 ? 0x3210u : (s1 == 1 ? 0x7655u : (s1 == 2 ? 0xA988u : (s1 == 3 ? 0xDCB4u : 0xFEEEu)));
    const int sc = (int) ((row >> (4 * s2)) & 15);
    const unsigned l1 = sc < 8 ? 0x11130000u : 0x44333222u, l2 = sc < 8 ? 0x32103210u : 0x32321321u;
    *slen1 = (int) ((l1 >> (4 * (sc & 7))) & 15);
    *slen2 = (int) ((l2 >> (4 * (sc & 7))) & 15);
    return sc;
}

// A transmitted scalefactor as k_pack gets it: value (low byte, two's complement) | length << 8 | 0x8000 if negative.
// The first-generation allocator can leave negative ones (an empty band's 0 minus the pre-emphasis table entry,
// reference bitallo1.cpp:547-586), which the reference's bit writer ORs into its buffer unmasked; k_pack reproduces that.
__device__ __forceinline__ int sf_field(int len, int v, bool sent)
{
    return sent ? ((len << 8) | (v & 255) | (v < 0 ? 0x8000 : 0)) : 0;
}

// scalefactors of a long granule; use_scfsi = all granules of the frame are long.
// Returns the new bit position; *sc_out = scalefac_compress; *field = this lane's transmitted
// scalefactor as (length << 8) | value, 0 if none (k_pack writes the bits).
__device__ int pack_sf_long(AllocLds &L, int pos, int igr, int ch, int use_scfsi, int not_null, int *sc_out, int *field)
{
    HX_LANE_DECL;
    const sfo_t *sf = L.sfout[igr][ch];
    int scfsi = 0, sc = 0;
    // band group of scalefactor i: 0:[0,6) 1:[6,11) 2:[11,16) 3:[16,21)
    const int i = LANE;
    const int grp = (i < 6) ? 0 : (i < 11 ? 1 : (i < 16 ? 2 : 3));
    if (use_scfsi) {
        if (igr == 0) { if (i < 21) L.sf_save[ch][i] = sf[i]; }
        else {
            const int d = (i < 21) ? (L.sf_save[ch][i] - sf[i]) : 0;
            const unsigned diff = (unsigned) __ballot(d != 0);      // bit i: scalefactor i changed
            scfsi = ((diff & 0x3Fu) ? 0 : 8) | ((diff & 0x7C0u) ? 0 : 4) | ((diff & 0xF800u) ? 0 : 2) | ((diff & 0x1F0000u) ? 0 : 1);
        }
    }
    if (not_null || !use_scfsi) {
        if (!use_scfsi && !not_null) { *sc_out = 0; if (LANE == 0) L.scfsi[ch] = 0; return pos; }
        const bool sent = (i < 21) && !(scfsi & (8 >> grp));
        // slen depends on the bit length of a group's largest value only, which is the bit length of the OR of its values:
        // one wave reduction for both halves
        const int sfp = sent ? max(sf[i], 0) : 0;       // (a group's largest value: negative ones do not count)
        const int ors = hx_wave_or(grp < 2 ? sfp : sfp << 8);
        int s1, s2;
        sc = sf_compress(ors & 255, ors >> 8, &s1, &s2);
        int len = sent ? (grp < 2 ? s1 : s2) : 0;
        *field = sf_field(len, sent ? sf[i] : 0, sent);
        pos += hx_wave_sum(len);
    }
    if (LANE == 0) L.scfsi[ch] = use_scfsi ? scfsi : 0;
    *sc_out = sc;
    return pos;
}

// short blocks (reference spdsmr.c:109-182): mpre = [3][12] spread sums of this granule from the
// psy kernel; es = previous short granule's doubled window-2 sums (used only when the previous
// granule was short too)
__device__ HX_COLD void compute_mask_short(AllocLds &L, const AllocPrm *p, const float *mpre, const float *es,
                                   int es_doubled, int block_type_prev)
{
    HX_LANE_DECL;
    const int ch = LANE >> 5, i = LANE & 31;
    const int mpart = (p->psyS.npart + 1) >> 1;
    if (i < 12) {
        int mb0 = 0, mb1 = 0, mb2 = 0;
        if (i < mpart) {
            const float *m = mpre + ch * 64;
            float k0 = m[i], k1 = m[12 + i], k2 = m[24 + i];
            float m0 = es_doubled ? es[ch * 64 + i] : 2.0f * es[ch * 64 + 24 + i];
            float m1 = 2.0f * k0, m2 = 2.0f * k1, tmp;
            if (block_type_prev == 2 && k0 > m0) { tmp = 0.1f * k0; k0 = (m0 > tmp) ? m0 : tmp; }
            if (k1 > m1) { tmp = 0.1f * k1; k1 = (m1 > tmp) ? m1 : tmp; }
            if (k2 > m2) { tmp = 0.1f * k2; k2 = (m2 > tmp) ? m2 : tmp; }
            mb0 = MBLOG(k0);
            mb1 = MBLOG(k1 + 0.1f * k0);
            mb2 = MBLOG(k2 + 0.1f * k1);
        }
        L.s_maskmb[ch][0][i] = mb0; L.s_maskmb[ch][1][i] = mb1; L.s_maskmb[ch][2][i] = mb2;
    }
    HX_WAVE_SYNC();
}

// 32-byte stereo side information (reference l3pack.c:1123-1187), whole wave: lanes 0..3 build
// the 59-bit block of one (granule, channel) in a register, lane 4 the scfsi bits; 32 lanes
// store the bytes.
__device__ void build_side(AllocLds &L, const AllocPrm *p, unsigned *sidew, const HxGr (*gr)[2], const int *scfsi, int main_data_begin)
{
    HX_LANE_DECL;
    if (LANE < 10) sidew[LANE] = 0;
    HX_WAVE_SYNC();
    if (LANE < 5) {
        unsigned long long v = 0;
        int pos, n;
        auto put = [&](unsigned x, int k) { v = (v << k) | x; };
        const int mono = p->nchan == 1;     // 17 bytes: 9 + 5 + 4 bits, then one 59-bit block per granule
        if (LANE < 4) {
            const HxGr *g = mono ? &gr[LANE & 1][0] : &gr[LANE >> 1][LANE & 1];
            put(g->part2_3_length, 12);
            put(g->big_values, 9);
            put(g->global_gain, 8);
            put(g->scalefac_compress, 4);
            put(g->window_switching_flag, 1);
            if (g->window_switching_flag) {
                put(g->block_type, 2);
                put(g->mixed_block_flag, 1);
                put(g->table_select[0], 5);
                put(g->table_select[1], 5);
                put(g->subblock_gain[0], 3);
                put(g->subblock_gain[1], 3);
                put(g->subblock_gain[2], 3);
            } else {
                put(g->table_select[0], 5);
                put(g->table_select[1], 5);
                put(g->table_select[2], 5);
                put(g->region0_count, 4);
                put(g->region1_count, 3);
            }
            put(g->preflag, 1);
            put(g->scalefac_scale, 1);
            put(g->count1table_select, 1);
            pos = mono ? 18 + 59 * LANE : 20 + 59 * LANE; n = (mono && LANE >= 2) ? 0 : 59;
        } else {        // main_data_begin (9), private bits (3), scfsi
            put((unsigned) main_data_begin, 9);
            put(0, mono ? 5 : 3);
            put(scfsi[0], 4);
            if (!mono) put(scfsi[1], 4);
            pos = 0; n = mono ? 18 : 20;
        }
        // OR the n-bit field (n <= 64) into the MSB-first words, up to three words touched
        if (n > 0) {
            const int wi = pos >> 5, o = pos & 31;
            const unsigned long long top = (n + o > 64) ? (v >> (n + o - 64)) : (v << (64 - n - o));
            const unsigned w0 = (unsigned) (top >> 32), w1 = (unsigned) top;
            if (w0) atomicOr(&sidew[wi], w0);
            if (w1) atomicOr(&sidew[wi + 1], w1);
            if (n + o > 64) { const unsigned w2 = (unsigned) (v << (96 - n - o)); if (w2) atomicOr(&sidew[wi + 2], w2); }
        }
    }
    HX_WAVE_SYNC();
}
// ... and as bytes at dst (the packet outputs; a frame's own side information leaves through the outbox)
__device__ HX_COLD void pack_side(AllocLds &L, const AllocPrm *p, unsigned char *dst, int main_data_begin)
{
    HX_LANE_DECL;
    build_side(L, p, L.sidew, L.gr, L.scfsi, main_data_begin);
    if (LANE < p->side_bytes) dst[LANE] = (unsigned char) (L.sidew[LANE >> 2] >> (24 - 8 * (LANE & 3)));
}

// ---- MPEG-2 LSF variants (one granule per frame) ----
// slen of one scalefactor group from its maximum, capped at 4 / 4 / 3 / 3 (reference l3pack.c:636-667)
__device__ __forceinline__ int lsf_slen(int sfmax, int cap)
{
    int n = 1, sl;
    sfmax++;
    for (sl = 0; sl < cap; sl++) { if (sfmax <= n) break; n += n; }
    return sl;
}

// Scalefactors of an MPEG-2 granule without intensity stereo (reference l3pack.c:561-729 long,
// :732-930 short): four groups of 6/5/5/5 long or 3/3/3/3 short bands, nothing shared between
// granules, 9-bit scalefac_compress.  sfs = the short scalefactors [window][sfb] when bt == 2.
__device__ HX_COLD int pack_sf_lsf(AllocLds &L, int pos, int igr, int ch, int bt, int *sc_out, int *field)
{
    const sfo_t (*sfs)[12] = L.sfs[ch];     // (taken from L here: as a pointer argument of this out-of-line function it was a generic pointer, its reads FLAT)
    HX_LANE_DECL;
    int v = 0, grp = 0;
    bool on;
    if (bt == 2) {      // transmission order: sfb-major, the three windows of a band together
        const int i = LANE / 3, w = LANE - 3 * i;
        on = LANE < 36;
        v = on ? sfs[w][i] : 0;
        grp = i / 3;
    } else {
        on = LANE < 21;
        v = on ? L.sfout[igr][ch][LANE] : 0;
        grp = (LANE < 6) ? 0 : (LANE < 11 ? 1 : (LANE < 16 ? 2 : 3));
    }
    const int s1 = lsf_slen(hx_wave_max((on && grp == 0) ? v : 0), 4), s2 = lsf_slen(hx_wave_max((on && grp == 1) ? v : 0), 4);
    const int s3 = lsf_slen(hx_wave_max((on && grp == 2) ? v : 0), 3), s4 = lsf_slen(hx_wave_max((on && grp == 3) ? v : 0), 3);
    const int len = on ? (grp == 0 ? s1 : (grp == 1 ? s2 : (grp == 2 ? s3 : s4))) : 0;
    *field = sf_field(len, v, on);
    *sc_out = s4 + (s3 << 2) + ((s2 + 5 * s1) << 4);
    return pos + hx_wave_sum(len);
}

// The right channel of an MPEG-2 joint-stereo granule with intensity coding (reference l3pack.c:561-729, is_chan
// branch): three groups of 7 bands; bands from nsf_stereo on carry intensity positions, a scalefactor of 999 marks
// "no intensity" and goes out as the group's all-ones value, which a real position must therefore never take (the
// group's length grows by one if it would).
__device__ HX_COLD int pack_sf_lsf_is(AllocLds &L, int pos, int igr, int nsf_stereo, int *sc_out, int *field)
{
    HX_LANE_DECL;
    const bool on = LANE < 21;
    const int grp = LANE < 7 ? 0 : (LANE < 14 ? 1 : 2);
    int v = on ? L.sfout[igr][1][LANE] : 0;
    const bool ill = on && v >= 999;
    const int m0 = hx_wave_max((on && !ill && grp == 0) ? v : 0), m1 = hx_wave_max((on && !ill && grp == 1) ? v : 0);
    const int m2 = hx_wave_max((on && !ill && grp == 2) ? v : 0);
    const int im1 = hx_wave_max((on && !ill && grp == 1 && LANE >= nsf_stereo) ? v : -1);
    const int im2 = hx_wave_max((on && !ill && grp == 2 && LANE >= nsf_stereo) ? v : -1);
    const int s0 = lsf_slen(m0, 4);
    int s1 = lsf_slen(m1, 4), s2 = lsf_slen(m2, 3);
    if (im1 == ((1 << s1) - 1)) s1++;
    if (im2 == ((1 << s2) - 1)) s2++;
    const int len = on ? (grp == 0 ? s0 : (grp == 1 ? s1 : s2)) : 0;
    if (ill) v = (1 << len) - 1;
    *field = sf_field(len, v, on);
    const int sc = s2 + 6 * s1 + 36 * s0;
    *sc_out = sc + sc + 1;
    return pos + hx_wave_sum(len);
}

// MPEG-2 side information of granule igr (reference l3pack.c:1189-1246): 8-bit main_data_begin,
// 2 private bits (1 for mono), one 63-bit block per channel; 17 bytes, 9 for mono.
// box: whose staging words and side-information fields - -1 = the allocator's own (L.sidew, L.gr: packet outputs), 0 / 1 = that
// outbox's (the helper wave, a granule later).  Chosen in here rather than passed as pointers: this function is out of line,
// pointer arguments into LDS would be generic pointers and their accesses FLAT instructions, which the wave-local hand-overs
// (HX_WAVE_SYNC: DS instructions in issue order, no wait) do not order (tools/check_lds_flat.py).
__device__ HX_COLD void build_side_lsf(AllocLds &L, const AllocPrm *p, int box, int igr, int main_data_begin)
{
    HX_LANE_DECL;
    unsigned *sidew = (box < 0) ? L.sidew : L.ob[box & 1].sidew;
    const HxGr (*gr)[2] = (box < 0) ? L.gr : L.ob[box & 1].gr;
    if (LANE < 10) sidew[LANE] = 0;
    HX_WAVE_SYNC();
    const int mono = p->nchan == 1, h = mono ? 9 : 10;
    if (LANE < p->nchan) {
        const HxGr *g = &gr[igr][LANE];
        unsigned long long v = 0;
        auto put = [&](unsigned x, int k) { v = (v << k) | x; };
        put(g->part2_3_length, 12);
        put(g->big_values, 9);
        put(g->global_gain, 8);
        put(g->scalefac_compress, 9);
        put(g->window_switching_flag, 1);
        if (g->window_switching_flag) {
            put(g->block_type, 2);
            put(g->mixed_block_flag, 1);
            put(g->table_select[0], 5);
            put(g->table_select[1], 5);
            put(g->subblock_gain[0], 3);
            put(g->subblock_gain[1], 3);
            put(g->subblock_gain[2], 3);
        } else {
            put(g->table_select[0], 5);
            put(g->table_select[1], 5);
            put(g->table_select[2], 5);
            put(g->region0_count, 4);
            put(g->region1_count, 3);
        }
        put(g->scalefac_scale, 1);
        put(g->count1table_select, 1);
        const int pos = h + 63 * LANE, wi = pos >> 5, o = pos & 31, n = 63;
        const unsigned long long top = (n + o > 64) ? (v >> (n + o - 64)) : (v << (64 - n - o));
        const unsigned w0 = (unsigned) (top >> 32), w1 = (unsigned) top;
        if (w0) atomicOr(&sidew[wi], w0);
        if (w1) atomicOr(&sidew[wi + 1], w1);
        if (n + o > 64) { const unsigned w2 = (unsigned) (v << (96 - n - o)); if (w2) atomicOr(&sidew[wi + 2], w2); }
    }
    if (LANE == 4) atomicOr(&sidew[0], (unsigned) main_data_begin << 24);
    HX_WAVE_SYNC();
}
__device__ HX_COLD void pack_side_lsf(AllocLds &L, const AllocPrm *p, unsigned char *dst, int igr, int main_data_begin)
{
    HX_LANE_DECL;
    build_side_lsf(L, p, -1, igr, main_data_begin);
    if (LANE < p->side_bytes) dst[LANE] = (unsigned char) (L.sidew[LANE >> 2] >> (24 - 8 * (LANE & 3)));
}
