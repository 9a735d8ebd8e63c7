// hx_alloc3.inc - K6 entry point: one wavefront per stream walks the batch's frames
// (reference mp3enc.cpp:1492-1597 encode_jointB, :2106-2333 CBR/VBR frame drivers).

// Arguments used once per frame or less are re-read from the kernarg segment where they are needed instead of staying in
// (spilled) scalar registers for the whole kernel.
#define COLD(field) (((const __attribute__((address_space(4))) AllocArgs *) __builtin_amdgcn_kernarg_segment_ptr())->field)
// The stream constants of the frame loop are read from LDS (L.P) in the section that uses them - a frame's budget, its
// placement - a handful of reads in flight together; as scalar registers held over the whole loop they, too, ended up in
// VGPR lanes and from there in scratch.
#define RFL(x) __builtin_amdgcn_readfirstlane(x)

// *_Packet entry points (reference mp3enc.cpp:3066-3074, :2944-2951): the frame as a self-contained
// packet - header with the nominal bitrate index, side info with main_data_begin 0, unpadded main
// data (header and side information here, the main data by k_pack).  Kept out of line: rarely used, and
// inlining it shifts the hot loop's code layout.
__device__ __noinline__ void emit_packet(AllocLds &L, const AllocPrm *p, unsigned char *q, int *nbytes, int pad, int ms, int raw_bytes, int hdr, int lsf_igr)
{
    HX_LANE_DECL;
    if (LANE < 4) {
        unsigned char h = p->head[LANE];
        if (LANE == 2 && pad) h |= 2;
        if (LANE == 3) h = (unsigned char) ((h & 0xCF) | ((ms + ms + (HX_A1 ? p->is_flag : 0)) << 4));
        q[LANE] = h;
    }
    if (lsf_igr >= 0) pack_side_lsf(L, p, q + 4, lsf_igr, 0);
    else pack_side(L, p, q + 4, 0);
    if (LANE == 0) *nbytes = hdr + raw_bytes;       // the main data bytes follow from k_pack
}

// scalefactors of one granule / channel in the layout of the stream type; returns the new bit position
// The scalefactor bits themselves are written by k_pack: here they are sized, and every transmitted field goes to
// sfdst[0..39] as (length << 8) | value in transmission order.
template <int LSF>
__device__ __forceinline__ int pack_sf_any(AllocLds &L, int pos, int igr, int ch, int bt, int use_scfsi, int not_null, int *sc, unsigned short *sfdst)
{
    HX_LANE_DECL;
    *sc = 0;
    int field = 0;
    if (LSF) {
        if (not_null) {
            if (HX_A1 && ch == 1 && L.P.is_flag) pos = pack_sf_lsf_is(L, pos, igr, L.P.nsf[1], sc, &field);
            else pos = pack_sf_lsf(L, pos, igr, ch, bt, sc, &field);
        }
    }
    else if (bt == 2) { pos = pack_sf_short(L, pos, L.sfs[ch], not_null, sc, &field); if (LANE == 0) L.scfsi[ch] = 0; }
    else pos = pack_sf_long(L, pos, igr, ch, use_scfsi, not_null, sc, &field);
    if (LANE < 40) sfdst[LANE] = (unsigned short) field;
    return pos;
}

// One (granule, channel) for k_pack: the record (into the outbox) ...
__device__ __forceinline__ void seg_out(AllocLds &L, HxSegOut *so, const HxGr *gg, int start_bit)
{
    HX_LANE_DECL;
    if (LANE == 0) {
        const int nq = max(gg->aux_nquads, 0);       // (the region split can leave -1 quads: none)
        so->start_bit = start_bit; so->huff_bits = gg->aux_bits;
        so->nreg01 = gg->aux_nreg[0] | (gg->aux_nreg[1] << 16); so->nreg2_quads = gg->aux_nreg[2] | (nq << 16);
        so->tabs = gg->table_select[0] | (gg->table_select[1] << 8) | (gg->table_select[2] << 16) | (gg->count1table_select << 24);
        so->not_null = gg->aux_not_null ? 1 : 0;
    }
}

// Both channels of a long granule (MPEG-1, second-generation allocator) sized and handed over in one pass: lanes
// 0..31 work on channel 0, lanes 32..63 on channel 1 (pack_sf_long + seg_out, half a wave each).  Returns the
// bits of the two segments; a channel's first bit is the sum of the sizes before it.
__device__ __forceinline__ int handover_long2(AllocLds &L, Outbox &ob, int pos, int igr, int use_scfsi, int nchan)
{
    HX_LANE_DECL;
    const int c = LANE >> 5, i = LANE & 31;
    HxGr *gg = &L.gr[igr][c];
    const bool chan = c < nchan;
    const int nn = chan ? gg->aux_not_null : 0, ab = gg->aux_bits;
    const int sfv = (chan && i < 21) ? L.sfout[igr][c][i] : 0;
    const int grp = (i < 6) ? 0 : (i < 11 ? 1 : (i < 16 ? 2 : 3));
    int scfsi = 0;
    if (use_scfsi) {
        if (igr == 0) { if (chan && i < 21) L.sf_save[c][i] = sfv; }
        else {
            const int d = (chan && i < 21) ? (L.sf_save[c][i] - sfv) : 0;
            const unsigned long long bal = __ballot(d != 0);
            const unsigned diff = c ? (unsigned) (bal >> 32) : (unsigned) bal;      // bit i: scalefactor i changed
            scfsi = ((diff & 0x3Fu) ? 0 : 8) | ((diff & 0x7C0u) ? 0 : 4) | ((diff & 0xF800u) ? 0 : 2) | ((diff & 0x1F0000u) ? 0 : 1);
        }
    }
    const bool sent = nn && (i < 21) && !(scfsi & (8 >> grp));
    const int ors = hx_half_or(sent ? (grp < 2 ? sfv : sfv << 8) : 0);
    int s1, s2;
    int sc = sf_compress(ors & 255, ors >> 8, &s1, &s2);
    const int len = sent ? (grp < 2 ? s1 : s2) : 0;
    const int sfbits = hx_half_sum(len);
    if (!nn) sc = 0;
    const int bits = nn ? sfbits + ab : 0;
    const int bits0 = __builtin_amdgcn_readlane(bits, 0), bits1 = __builtin_amdgcn_readlane(bits, 32);
    const int start = c ? pos + bits0 : pos;
    ob.seg[c].sf[i] = (unsigned short) (len ? ((len << 8) | sfv) : 0);
    if (i < 8) ob.seg[c].sf[32 + i] = 0;
    if (i == 0 && chan) {
        L.scfsi[c] = use_scfsi ? scfsi : 0;
        HxSegOut *so = &ob.seg[c];
        const int nq = max(gg->aux_nquads, 0);
        so->start_bit = start; so->huff_bits = ab;
        so->nreg01 = gg->aux_nreg[0] | (gg->aux_nreg[1] << 16); so->nreg2_quads = gg->aux_nreg[2] | (nq << 16);
        so->tabs = gg->table_select[0] | (gg->table_select[1] << 8) | (gg->table_select[2] << 16) | (gg->count1table_select << 24);
        so->not_null = nn ? 1 : 0;
        gg->scalefac_compress = sc; gg->part2_3_length = bits;
    }
    return bits0 + bits1;
}

// 16- and 8-byte register values as native vectors: copies of HIP's uint4 / uint2 structs between address spaces are memcpy
// calls to the compiler, and a memcpy from LDS into a local object pins that object in the wave's scratch memory (the
// helper wave's line and record hand-over went through scratch that way: 16 KB written and re-read per frame).
typedef unsigned int hx_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int hx_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ hx_u4 mk_u4(unsigned a, unsigned b, unsigned c, unsigned d) { hx_u4 v; v.x = a; v.y = b; v.z = c; v.w = d; return v; }

// The helper wave empties granule g's outbox: into registers before it reports back, to memory after.
// (the frame record travels as four 16-byte pieces and the slot as one 8-byte piece: copied as structs they went through the
// wave's scratch memory - a 64-byte memcpy from LDS into a stack object and another one out of it, per granule)
static_assert(sizeof(HxFrameOut) == 64 && sizeof(HxSlot) == 8, "OutRegs carries the frame record as four hx_u4 and the slot as one hx_u2");
struct OutRegs { hx_u4 seg, f0, f1, f2, f3; hx_u2 slot; int opos, frm_index, slot_index, has_frame; };
__device__ __forceinline__ void outbox_gather(AllocLds &L, int g, OutRegs &r)
{
    HX_LANE_DECL;
    const Outbox &ob = L.ob[g & 1];
    r.seg = reinterpret_cast<const hx_u4 *>(&ob.seg[0])[min(LANE, 13)];
    r.has_frame = ob.has_frame;
    r.opos = ob.opos; r.frm_index = ob.frm_index; r.slot_index = ob.slot_index;
    r.f0 = reinterpret_cast<const hx_u4 *>(&ob.frm)[0]; r.f1 = reinterpret_cast<const hx_u4 *>(&ob.frm)[1];
    r.slot = *reinterpret_cast<const hx_u2 *>(&ob.slot);
    // the frame's first four slots from the ring (entries past the newest pending frame are never used by the packer):
    // HxFrameOut::near[4] = the record's last 32 bytes
    const int q0 = ob.ring_p0 & 31, q1 = (ob.ring_p0 + 1) & 31, q2 = (ob.ring_p0 + 2) & 31, q3 = (ob.ring_p0 + 3) & 31;
    r.f2 = mk_u4((unsigned) L.r_off[q0], L.r_mf[q0], (unsigned) L.r_off[q1], L.r_mf[q1]);
    r.f3 = mk_u4((unsigned) L.r_off[q2], L.r_mf[q2], (unsigned) L.r_off[q3], L.r_mf[q3]);
}
template <int LSF>
__device__ __forceinline__ void outbox_store(AllocLds &L, const AllocArgs &a, int s, int g, const OutRegs &r)
{
    HX_LANE_DECL;
    const long long unit = (long long) s * a.NG + g;
    if (LANE < 7 * L.P.nchan) reinterpret_cast<hx_u4 *>(a.seg + unit * 2)[LANE] = r.seg;
    if (r.has_frame) {      // (the box is this wave's until the master fills it again, two granules on)
        Outbox &ob = L.ob[g & 1];
        if (LSF) build_side_lsf(L, &L.P, g & 1, ob.part, ob.mdb);
        else build_side(L, &L.P, ob.sidew, ob.gr, ob.scfsi, ob.mdb);
        const int fpc = COLD(fpc);                  // frame records per stream: the stride (AllocArgs::fpc)
        unsigned char *o = a.out + (long long) s * a.out_stride + r.opos;
        const int k = max(LANE - 4, 0);
        const unsigned byte = (LANE < 4) ? ob.head[LANE] : ((ob.sidew[min(k >> 2, 9)] >> (24 - 8 * (k & 3))) & 255);
        if (LANE < 4 + L.P.side_bytes) o[LANE] = (unsigned char) byte;
        if (LANE == 0) {
            hx_u4 *fd = reinterpret_cast<hx_u4 *>(&a.frm[(long long) s * fpc + r.frm_index]);
            fd[0] = r.f0; fd[1] = r.f1; fd[2] = r.f2; fd[3] = r.f3;
            *reinterpret_cast<hx_u2 *>(&a.slots[(long long) s * (fpc + HX_SLOTS_EXTRA) + r.slot_index]) = r.slot;
        }
    }
}

// ... and its quantised lines as int16 (eight per lane and store); short-block granules also store their signs,
// which the allocator has put into bitstream order.  Run by the helper wave while the master goes on: the lines are
// picked up before the helper reports back (the master's next granule overwrites them), stored after.
struct LinesRegs { hx_u4 a, b; unsigned sg; int on; };
// 32 sign bytes (0 / 1 each, lines 32 w .. 32 w + 31 of the bitstream order) -> one word, bit per line: four bytes of a
// word gather in its top nibble under a multiplication whose partial products do not meet (bits 28 .. 31 get one term each)
__device__ __forceinline__ unsigned sign_word(const hx_u4 lo, const hx_u4 hi)
{
    const unsigned M = 0x10204080u;
    return ((lo.x * M) >> 28) | (((lo.y * M) >> 28) << 4) | (((lo.z * M) >> 28) << 8) | (((lo.w * M) >> 28) << 12)
         | (((hi.x * M) >> 28) << 16) | (((hi.y * M) >> 28) << 20) | (((hi.z * M) >> 28) << 24) | (((hi.w * M) >> 28) << 28);
}
__device__ __forceinline__ void lines_gather(AllocLds &L, int on, int ch, int bt, LinesRegs &r)
{
    HX_LANE_DECL;
    r.on = on;
#if HX_SLIM
    // the lines are int16 already; a short granule's reordered signs lie in the x34 buffer
    const hx_u4 *src = reinterpret_cast<const hx_u4 *>(IX(ch));
    r.a = src[LANE]; r.b = src[min(LANE + 64, 71)];
    if (bt == 2) { const hx_u4 *sb = reinterpret_cast<const hx_u4 *>(&L.x34[ch][0]); const int w = min(LANE, 17); r.sg = sign_word(sb[2 * w], sb[2 * w + 1]); }
#else
    const int4 *src = reinterpret_cast<const int4 *>(IX(ch));
    int4 v[4];
    v[0] = src[2 * LANE]; v[1] = src[2 * LANE + 1];
    v[2] = src[2 * min(LANE + 64, 71)]; v[3] = src[2 * min(LANE + 64, 71) + 1];
    r.a = mk_u4((unsigned) (v[0].x & 0xFFFF) | ((unsigned) v[0].y << 16), (unsigned) (v[0].z & 0xFFFF) | ((unsigned) v[0].w << 16),
                     (unsigned) (v[1].x & 0xFFFF) | ((unsigned) v[1].y << 16), (unsigned) (v[1].z & 0xFFFF) | ((unsigned) v[1].w << 16));
    r.b = mk_u4((unsigned) (v[2].x & 0xFFFF) | ((unsigned) v[2].y << 16), (unsigned) (v[2].z & 0xFFFF) | ((unsigned) v[2].w << 16),
                     (unsigned) (v[3].x & 0xFFFF) | ((unsigned) v[3].y << 16), (unsigned) (v[3].z & 0xFFFF) | ((unsigned) v[3].w << 16));
    if (bt == 2 || HX_A1) {     // (the first-generation allocator takes the signs itself, too)
        const hx_u4 *sb = reinterpret_cast<const hx_u4 *>(&L.signx[ch][0]);
        const int w = min(LANE, 17);
        r.sg = sign_word(sb[2 * w], sb[2 * w + 1]);
    }
#endif
}
__device__ __forceinline__ void lines_store(const AllocArgs &a, long long unit, int ch, int bt, const LinesRegs &r)
{
    HX_LANE_DECL;
    if (!r.on) return;
    hx_u4 *dst = reinterpret_cast<hx_u4 *>(a.ixq + (unit * 2 + ch) * 576);
    dst[LANE] = r.a;
    if (LANE < 8) dst[64 + LANE] = r.b;
    if (bt == 2 || HX_A1) {
        unsigned *sd = a.sgn_w + (unit * 2 + ch) * HX_SGN_WORDS;
        if (LANE < 18) sd[LANE] = r.sg;
    }
}

// A granule's operands - magnitudes (or the raw spectrum of a short block), x^(3/4) and the band lanes'
// start values - travel from global memory straight into LDS (global_load_lds, 16 bytes per lane, no registers
// in between).  The helper wave issues the requests and waits for them: on the master wave every reload of a
// spilled register in between would wait for the whole queue (vector memory loads return in order).
__device__ __forceinline__ void granule_fetch(AllocLds &L, const AllocArgs &a, long long unit)
{
    HX_LANE_DECL;
    const float *sx = a.xr + unit * 1152;
#pragma unroll
    for (int k = 0; k < 4; k++) glds16(sx + 4 * (LANE + 64 * k), &L.xr[0][0] + 256 * k);
    if (LANE < 32) glds16(sx + 4 * (LANE + 256), &L.xr[0][0] + 1024);
    const unsigned char *bd = reinterpret_cast<const unsigned char *>(a.band + unit);
    glds16(bd + 16 * LANE, BAND_LANDING);
    if (LANE < (int) (sizeof(HxBandPrep) / 16) - 64) glds16(bd + 16 * (64 + LANE), reinterpret_cast<unsigned char *>(BAND_LANDING) + 1024);
}

// A long granule's spectrum as fetched -> magnitudes in the representation the frame is coded in (L / R, or M = L + R,
// S = L - R: reference l3math.c:449-470,905-930), exactly as k_prep formed them for its band energies and x^(3/4)
// (same line ranges; the lines above them stay as they are).  Run by the helper wave on the freshly landed lines.
__device__ __forceinline__ void xr_to_coded(AllocLds &L, int ms)
{
    HX_LANE_DECL;
    const int two = L.P.nchan == 2;
    const int nl0 = ms ? (L.P.hf_flag ? L.startBand[22] : L.P.nbmax[0]) : L.P.nbmax3[0];
    const int nl1 = ms ? nl0 : (two ? L.P.nbmax3[1] : 0);
    float l[9], r[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { l[k] = L.xr[0][LANE + 64 * k]; r[k] = L.xr[1][LANE + 64 * k]; }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int j = LANE + 64 * k;
        float o0 = l[k], o1 = r[k];
        if (ms) {
            if (j < nl0) {
                float m = (l[k] + r[k]), d = (l[k] - r[k]);
                if (m < 0.0f) m = -m;
                if (d < 0.0f) d = -d;
                o0 = m; o1 = d;
            }
        } else {
            if (j < nl0) { float v = l[k]; if (!(v >= 0.0f)) v = -v; o0 = v; }
            if (j < nl1) { float v = r[k]; if (!(v >= 0.0f)) v = -v; o1 = v; }
        }
        L.xr[0][j] = o0; L.xr[1][j] = o1;
    }
}

// x^(3/4) of a long granule's coded magnitudes (reference pow34.c:132-186; the lines k_prep took its band maxima from).
// Run by the helper wave behind the master's back: the master meets it again at its first work order of the granule
// (the gain search), the first reader of these lines.
__device__ __forceinline__ void x34_from_coded(AllocLds &L, int ms)
{
    HX_LANE_DECL;
    const int nl0 = ms ? L.P.nbmax2[0] : L.P.nbmax3[0], nl1 = ms ? L.P.nbmax2[1] : L.P.nbmax3[1];   // (mono: channel 1 has none)
    float a[9], b[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { a[k] = L.xr[0][LANE + 64 * k]; b[k] = L.xr[1][LANE + 64 * k]; }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int j = LANE + 64 * k;
        L.x34[0][j] = (j < nl0) ? pow34(L, a[k]) : 0.0f;
        L.x34[1][j] = (j < nl1) ? pow34(L, b[k]) : 0.0f;
    }
}

// The helper wave: serves the master's work orders until it says stop (HCMD_EXIT).
template <int LSF>
__device__ __forceinline__ void helper_serve(const AllocArgs &a, AllocLds &L)
{
    for (;;) {
        HX_LANE_DECL;       // (per order: nothing derived from the lane number is carried around the loop and over the calls in it)
        WG_BARRIER();
        const int4 order = *reinterpret_cast<const int4 *>(&L.cmdw[0]);     // command and its three arguments
        const int cmd = order.x;
        // most frequent orders first
        if (cmd == HCMD_SEEK) seek_actual_ch(L, &L.P, 1);
        else if (cmd == HCMD_COUNT_BITS) count_bits_ch(L, &L.P, 1, order.y);
        else if (cmd == HCMD_LUCKY) { if (__builtin_expect(order.z, 0)) lucky_eval_big(L, order.y, 1, 2); else lucky_eval(L, order.y, 1, 2); }
        else if (cmd == HCMD_QUANT) quant_lines(L, &L.P, order.y, 1);
        else if (cmd == HCMD_QUANT_COUNT) { quant_lines(L, &L.P, order.y, 1); HX_WAVE_SYNC(); count_bits_ch(L, &L.P, 1, order.z); }
        else if (cmd == HCMD_ISF2) isf2_ch(L, &L.P, 1);
        else if (cmd == HCMD_FETCH) {
            // The next granule's operands into LDS; the finished granule's lines and the granule before's outbox to
            // k_pack.  Only the loads are waited for: what goes out is picked up into registers, the helper reports
            // back, and the stores are issued behind the master's back.
            const int s = L.cur_s;      // the stream the master is walking (it changes between two orders only)
            int nbt = 2, nms = 0;
            if (order.y >= 0) {
                granule_fetch(L, a, (long long) s * a.NG + order.y);
                nbt = a.bt[(long long) s * a.NG + order.y]; nms = a.msflag[(long long) s * a.NG + order.y];
            }
            // (the order behind the stream's last granule - nothing to fetch, no lines - carries that granule's number in word 3)
            const int gl = order.z, gf = (gl >= 0) ? gl - 1 : ((order.y < 0) ? order.w : -1);
            // (defined on every path: left undefined where nothing is gathered, the compiler carried the previous order's
            // 38 registers around the helper's loop and saved them over every call in it)
            LinesRegs lr0 = {}, lr1 = {};
            OutRegs orr = {};
            const int two = L.P.nchan == 2;
            const int gbt = order.w & 255;      // (order word 3: block type | channel c's segment is not empty << (8 + c))
            if (gl >= 0) { lines_gather(L, (order.w >> 8) & 1, 0, gbt, lr0); if (two) lines_gather(L, (order.w >> 9) & 1, 1, gbt, lr1); }
            if (gf >= 0) outbox_gather(L, gf, orr);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            const bool long_gr = !HX_A1 && nbt != 2;
            if (long_gr) {
                xr_to_coded(L, nms);
                if (!two) x34_from_coded(L, nms);       // (a mono stream's master never meets the helper before it reads them)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            WG_BARRIER();
            if (gl >= 0) {
                const long long unit = (long long) s * a.NG + gl;
                lines_store(a, unit, 0, gbt, lr0);
                if (two) lines_store(a, unit, 1, gbt, lr1);
            }
            if (gf >= 0) outbox_store<LSF>(L, a, s, gf, orr);
            if (long_gr && two) { x34_from_coded(L, nms); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
            continue;
        }
        else if (cmd == HCMD_EXIT) return;
        WG_BARRIER();
    }
}

// Tables and the stream's carried state into LDS (the profile build also clears the stream's profile and starts its clock).
__device__ __forceinline__ void stage_stream(const AllocArgs &a, AllocLds &L, const HxStream *ss, const HxParams *gp, const HxGlobalTabs *gt)
{
    HX_LANE_DECL;
#if HX_SLIM
    for (int i = LANE; i < 256; i += 64) { L.look_ix43[i] = gp->look_ix43[i]; L.mblog[i] = (unsigned short) (gt->mblog[i] + 38227); }
    if (LANE < 4) L.gain4[LANE] = gp->look_gain[8 + LANE];
    if (LANE < 16) L.igain16[LANE] = gp->look_34igain[8 + LANE];
    if (LANE < 18) L.sgnbits[LANE / 9][LANE % 9] = 0;
#else
    for (int i = LANE; i < 256; i += 64) { L.look_ix43[i] = gp->look_ix43[i]; L.mblog[i] = gt->mblog[i]; L.pow34_exp[i] = gt->pow34_exp[i]; }
    for (int i = LANE; i < 128; i += 64) { L.look_gain[i] = gp->look_gain[i]; L.look_34igain[i] = gp->look_34igain[i]; }
#endif
    for (int i = LANE; i < 1408; i += 64) L.huff_len[i] = gt->huff_len[i];
    for (int i = LANE; i < 288; i += 64) L.band_of_pair[i] = gp->band_of_line[2 * i];
    L.lane_run[LANE] = gp->lane_run[LANE];
    if (LANE < 24) L.band_last[LANE] = gp->band_last_lane[LANE];
    for (int i = LANE; i < 192; i += 64) L.sband_of_line[i] = gp->sband_of_line[i];
    if (LANE < 16) {
        L.nBand_s[LANE] = (LANE < 13) ? gp->nBand_s[LANE] : 0;
        L.startBand_s[LANE] = (LANE < 14) ? gp->startBand_s[LANE] : 192;
        L.logcbw_s[LANE] = gp->look_log_cbwmb_s[LANE];
    }
    for (int i = LANE; i < 84; i += 64) L.logsub[i] = (HX_SLIM ? (short) gt->logsub[i] : gt->logsub[i]);
    if (LANE < 32) L.quant_off[LANE] = gt->quant_off[LANE];
    if (LANE < 32) {
        const int dim = (LANE >= 16) ? 16 : gt->huff_dim[LANE], lin = (LANE >= 16) ? gt->huff_lin[LANE] : 0;
        L.tabpk[LANE] = gt->huff_off[LANE] | (dim << 12) | (lin << 20);
    }
    if (LANE < 19) L.candpk[LANE] = cand_pack(candidates_chain(cand_class_rep(LANE)));
    if (LANE < 16) {
        L.pow34_a[LANE] = gt->pow34_a[LANE]; L.pow34_b[LANE] = gt->pow34_b[LANE];
        L.quada_len[LANE] = gt->quada_len[LANE];
    }
    if (LANE < 24) L.startBand[LANE] = gp->startBand_l[LANE];
    if (LANE < NB) { L.nBand[LANE] = gp->nBand_l[LANE]; L.logcbw[LANE] = gp->look_log_cbwmb[LANE]; L.taper[LANE] = gp->taperNT[LANE]; }
#if !HX_SLIM
    for (int i = LANE; i < 2 * 576; i += 64) { IX(0)[i] = 0; (&L.signx[0][0])[i] = 0; }
#endif
    if (LANE < 44) {
        int c = LANE / 22, b = LANE % 22;
        L.NTadjust[c][b] = ss->NTadjust[c][b];
        L.ixmax[c][b] = 0; L.sf[c][b] = 0; L.active[c][b] = 0; L.gsf[c][b] = 0; L.gzero[c][b] = 0; L.gmin[c][b] = 0;
        L.x34max[c][b] = 0.0f; L.Noise[c][b] = 0; L.Noise0[c][b] = 0; L.NT[c][b] = 0; L.geval[c][b] = -1;
        L.up[c][b] = 0; L.lo[c][b] = 0;
    }
    if (LANE < 42) L.sf_save[LANE / 21][LANE % 21] = ss->sf_save[LANE / 21][LANE % 21];
    if (LANE == 0) { L.pow43 = gt->pow43; L.big_counter = COLD(done_counter) + HX_CNT_BIG_SWEEPS; L.nstrict = 0; }
#if !HX_SLIM
    if (LANE < 3) L.nlucky[LANE] = 0;
#endif
    if (LANE < 3) L.nrounds[LANE] = 0;
    if (LANE < 4) L.P.head[LANE] = gp->head[LANE];
    if (LANE < 16) L.P.vbr_main_framebytes[LANE] = gp->vbr_main_framebytes[LANE];
    if (LANE < 22) L.P.rnBand_l[LANE] = gp->rnBand_l[LANE];
    if (LANE < 2) {
        // a mono stream (mode 3) runs the same code with an empty second channel: no bands, no lines
        const bool on = LANE < gp->nchan;
        L.P.nsf[LANE] = on ? gp->nsf[LANE] : 0; L.P.nsf2[LANE] = on ? gp->nsf2[LANE] : 0; L.P.nsf3[LANE] = on ? gp->nsf3[LANE] : 0;
        L.P.nbmax[LANE] = on ? gp->nbmax[LANE] : 0; L.P.nbmax2[LANE] = on ? gp->nbmax2[LANE] : 0; L.P.nbmax3[LANE] = on ? gp->nbmax3[LANE] : 0;
    }
    if (LANE == 0) {
        L.P.remainder = gp->remainder; L.P.divisor = gp->divisor; L.P.main_framebytes = gp->main_framebytes;
        L.P.sf_bit_max = gp->sf_bit_max; L.P.AveTargetBits = gp->AveTargetBits;
        L.P.ms_flag = gp->ms_flag; L.P.hf_flag = gp->hf_flag; L.P.vbr_flag = gp->vbr_flag;
        L.P.ivbr_min = gp->ivbr_min; L.P.ivbr_max = gp->ivbr_max; L.P.vbr_pool_target = gp->vbr_pool_target;
        L.P.fbmin = gp->vbr_main_framebytes[gp->ivbr_min & 15]; L.P.fbmax = gp->vbr_main_framebytes[gp->ivbr_max & 15];
        L.P.initialMNR = gp->initialMNR; L.P.test1 = gp->test1;
        L.P.nsfs = gp->nsfs; L.P.nbmax_s = gp->nbmax_s; L.P.psyS.npart = gp->psyS.npart;
        L.P.nchan = gp->nchan; L.P.side_bytes = gp->side_bytes;
        L.P.is_flag = gp->is_flag; L.P.dual = gp->alloc1 && gp->h_mode == 2; L.P.npart_l = gp->psyL.npart;
        L.P.oflags = (a.packet ? 1 : 0) | (a.dbg ? 2 : 0) | (a.frame_stats ? 4 : 0) | (a.strict_sums ? 8 : 0);
        L.P.run_w = gp->run_w;
    }
#if HX_A1
    // the four noise-estimate tables of the first-generation allocator live in the (otherwise unused) term buffer
    for (int i = LANE; i < 256; i += 64) {
        (&L.term[0][0])[i] = gp->a1_f_ix[i]; (&L.term[0][0])[256 + i] = gp->a1_f_ixmax[i];
        (&L.term[0][0])[512 + i] = gp->a1_f_big_ix[i]; (&L.term[0][0])[768 + i] = gp->a1_f_big_ixmax[i];
    }
    if (LANE < 42) L.gsf[LANE / 21][LANE % 21] = ss->a1_gsf[LANE / 21][LANE % 21];
    if (LANE == 0) {
        L.a_calls = ss->a1_call_count; L.a_bitadjust[0] = ss->a1_bitadjust[0]; L.a_bitadjust[1] = ss->a1_bitadjust[1];
        L.a_running = ss->a1_running_a; L.a_ave = ss->a1_ave_alpha; L.a_alpha = ss->a1_alpha;
    }
#endif
    if (LANE == 0) {
        L.MNR = ss->MNR; L.PoolFraction = ss->PoolFraction; L.call_count = ss->call_count;
        L.hf_quant = 0; L.hf_quant_stereo[0] = L.hf_quant_stereo[1] = 0; L.gsf_hf = -1;
        L.gsf_hf_stereo[0] = L.gsf_hf_stereo[1] = -1;
        L.scfsi[0] = L.scfsi[1] = 0;
        for (int g = 0; g < 2; g++) for (int c = 0; c < 2; c++) {
            HxGr z = {};
            L.gr[g][c] = z;
            for (int k = 0; k < 3; k++) L.gr[g][c].subblock_gain[k] = ss->gr_subblock_gain[g][c][k];
        }
    }
#ifdef HX_PROFILE
    L.prof[LANE] = 0;
    if (LANE == 0) L.prof[HX_PROF_TOTAL] = (unsigned) clock64();        // (the total is a difference of the low 32 bits)
#endif
    HX_WAVE_SYNC();
}

// Frame assembly (reference mp3enc.cpp:2258-2325 keeps main data in a ring and copies frames out
// when complete).  Here every frame is written straight to its final place in `out`: its slot
// offset is the running sum of the frame sizes, main_data_begin is the reservoir level at the
// frame's start, and a frame's main data never extends past its own slot.  Pending = frames
// whose slot is not full yet: ring [side_p0, side_p1) of slot sizes (r_mf) and header offsets
// (r_off); only the first pending slot is partly filled (main_bytes bytes), the later ones are
// empty.  Between calls the pending frames' images travel in ss->main_buf (length main_p1).
// The reservoir registers, ring positions and the layout cursor (opos: offset of the next frame's header) live in L.fs
// (see FrameState): read where a frame is budgeted and where it is placed, not held over the allocator's code between.
// (the images of the frames pending from earlier calls are copied to the head of `out` by k_pack_pre: the packer
// kernels own the main data, and an allocator launch does not have to wait for the previous call's packing)
template <int LSF>
__device__ __forceinline__ void slots_init(const AllocArgs &a, AllocLds &L, int s, const HxStream *ss, const HxParams *gp)
{
    HX_LANE_DECL;
    const int F = a.NG / 2;
    if (LANE == 0) {
        FrameState &fs = L.fs;
        fs.padcount = ss->padcount;
        fs.main_tot = ss->main_tot; fs.main_sent = ss->main_sent; fs.mf_tot = ss->mf_tot;
        fs.main_bytes = ss->main_bytes;
        fs.side_p0 = ss->side_p0; fs.side_p1 = ss->side_p1;
        fs.tot_frames_out = ss->tot_frames_out; fs.tot_bytes_out = ss->tot_bytes_out;
        fs.ave_tot = ss->ave_tot_bytes_out;
        fs.opos = ss->main_p1;
        fs.slot_lo = 0; fs.slot_hi = (int) ((ss->side_p1 - ss->side_p0) & 31);      // list positions of side_p0 / side_p1
        COLD(pre_len)[s] = ss->main_p1;
    }
    if (LANE < 32) L.r_mf[LANE] = (unsigned short) ss->frame_mf_bytes[LANE];
    HX_WAVE_SYNC();
    // every slot of this call, in order, for k_pack: the pending ones first, then one per new frame
    if (LANE == 0) {
        HxSlot *slots = a.slots + (long long) s * (COLD(fpc) + HX_SLOTS_EXTRA);
        int o = 0, j = 0;
        for (unsigned k = L.fs.side_p0; k != L.fs.side_p1; k = (k + 1) & 31, j++) {
            L.r_off[k] = o;
            slots[j].off = o; slots[j].mf = L.r_mf[k];
            o += 4 + gp->side_bytes + L.r_mf[k];
        }
    }
    HX_WAVE_SYNC();
}

// A frame's budget (reference mp3enc.cpp:2241-2257 / 2117-2128; MPEG-2 :2500-2516 / :2355-2363): the reservoir's side goes to
// L.fs for the frame's placement, the allocator's bounds come back.  ba_min / ba_max: the bits the next granule (or channel) may
// take; inc_min / inc_max: what each later one gets on top.
struct FrameBudget { int ba_min, ba_max, inc_min, inc_max, dba_max, TargetBits, bit_pool; };
template <int LSF>
__device__ __forceinline__ FrameBudget frame_budget(AllocLds &L, int P_vbr, int nchan, int dual)
{
    HX_LANE_DECL;
    const AllocPrm *p = &L.P;
    const int pool_cap = LSF ? 255 : 511;       // what main_data_begin can address
    int ba_min, ba_max, inc_min, inc_max, dba_max, TargetBits, bit_pool;
    int pad = 0, byte_pool, byte_max, byte_min;
    int padcount = RFL(L.fs.padcount);
    const int P_rem = RFL(p->remainder), P_div = RFL(p->divisor), P_mfb = RFL(p->main_framebytes);
    const int P_fbmin = RFL(p->fbmin), P_fbmax = RFL(p->fbmax), P_sfmax = RFL(p->sf_bit_max), P_avg = RFL(p->AveTargetBits);
    byte_pool = (int) (RFL(L.fs.mf_tot) - RFL(L.fs.main_tot));
    if (!P_vbr) {
        padcount -= P_rem;
        if (padcount <= 0) { padcount += P_div; pad = 1; }
    }
    if (!P_vbr) { byte_max = P_mfb + pad + byte_pool; byte_min = byte_max - pool_cap; }
    else { byte_max = P_fbmax + byte_pool; byte_min = P_fbmin + byte_pool - pool_cap; }
    if (LANE == 0) { L.fs.padcount = padcount; L.fs.pad = pad; L.fs.byte_pool = byte_pool; L.fs.byte_max = byte_max; L.fs.byte_min = byte_min; }

    // ---- encode_jointB ----
    // stereo: encode_jointB (mp3enc.cpp:1500-1527); mono: encode_singleB (:1686-1699)
    // (first-generation allocator: encode_jointA :1236-1318, encode_singleA :1601-1672 and their MPEG-2 twins
    // :1753-1829, :1910-1973 - dual channel allocates each channel on its own from half the frame)
    const int nalloc = dual ? 1 : nchan;        // channels allocated together
    TargetBits = nalloc * P_avg;
    const int bsh = (LSF ? 3 : 2) - dual;       // a frame's budget covers one granule (MPEG-2) or two
    bit_pool = byte_pool << bsh;
    const int bit_max = byte_max << bsh;
    const int bit_min = (byte_min << bsh) + ((LSF && nchan == 2 && !dual && byte_pool > 245) ? 40 : 0);
    const int sf_bits = nalloc * P_sfmax;
    const int ba_bit_max = ((nchan == 2 && !LSF && !HX_A1) ? bit_max : min(bit_max, 4095)) - sf_bits, ba_bit_min = bit_min - sf_bits;
    dba_max = (nchan == 2 && !LSF && !HX_A1) ? bit_pool >> 2 : 0;
    ba_min = ba_bit_min; ba_max = ba_bit_max + dba_max;
    inc_min = ba_bit_min + sf_bits; inc_max = ba_bit_max + sf_bits;       // what the next granule (or channel) gets on top
    return FrameBudget{ba_min, ba_max, inc_min, inc_max, dba_max, TargetBits, bit_pool};
}

// One granule: its operands joined, its allocation, the next granule's fetch order, its segments sized and handed over (the
// outbox of g & 1).  pos: the frame's main-data bits so far; b: what is left of the frame's budget.
// NGs: the stream's granules of this call, the bound of the look-ahead fetch (a.NG is the stride of the granule arrays).
template <int LSF>
__device__ __forceinline__ void granule_alloc(const AllocArgs &a, AllocLds &L, const HxParams *gp, int s, int g, int NGs, int igr, int bt, int btp,
                                              int ms, int shortblock_frame, int nchan, int dual, int P_vbr, FrameBudget &b, int &pos PROF_CLOCK)
{
    HX_LANE_DECL;
    const AllocPrm *p = &L.P;
    const int NG = a.NG;
    BandIn bin;
    {   // the granule's operands were requested a hand-over phase ago (see below): wait for them; the band
        // start values move out of their landing area.  (The signs of a long granule's lines go from k_prep
        // straight to k_pack; the short-block and first-generation allocators take them from the raw spectrum.)
        HELPER_JOIN();
        bin = band_fetch(BAND_LANDING);
        HX_WAVE_SYNC();
    }
    PROF_ACC(HX_PROF_JOIN_FETCH);
    // long blocks: x^(3/4) and signs of the lines from k_prep (requested here, landed in LDS after the
    // band-parallel start below)
    bool fetch_posted = false;      // the helper wave's fetch order went out inside the allocator already
#if HX_A1
    (void) btp; (void) bin;
    {
        const float *th_g = COLD(thr) + ((long long) s * NG + g) * 128;
        const float *esv = (g == 0) ? COLD(thrprev) + (long long) s * 128 : th_g - 128;
        a1_sigmask(L, p, COLD(etab) + ((long long) s * NG + g) * 128, th_g, esv, g == 0);
    }
    if (LANE < 2) { L.gr[igr][LANE].block_type = 0; }
    HX_WAVE_SYNC();
    if (!dual) { A1Ctx cx = {0, 2, ms, RFL(p->is_flag)}; bitallo1(L, p, gp, cx, igr, b.ba_min, b.TargetBits, b.ba_max); }
#else
    if (bt == 2) {
        const float *th_g = COLD(thr) + ((long long) s * NG + g) * 128;
        const float *esv = (g == 0) ? COLD(thrprev) + (long long) s * 128 : th_g - 128;
        compute_mask_short(L, p, th_g, esv, g == 0, btp);
    }
    if (LANE < 2) { L.gr[igr][LANE].block_type = bt; }
    HX_WAVE_SYNC();
    PROF_ACC(HX_PROF_GR_PRE);
    if (bt != 2) fetch_posted = bitallo_long(L, p, igr, bt, b.ba_min, b.TargetBits, b.ba_max, b.bit_pool, ms, bin, g, (g + 1 < NGs) ? g + 1 : -1);
    else {      // CBitAllo3::BitAllo, block_type 2 branch (reference bitallo3.cpp:496-547)
        const int P_imnr = RFL(p->initialMNR);
        int MNR0;
        if (P_vbr == 0) {
            MNR0 = L.MNR - (max(L.MNR - P_imnr, 0) >> 1) - (max(L.MNR - P_imnr - 400, 0) >> 2);
            MNR0 = max(P_imnr + 400, MNR0);
        } else MNR0 = P_imnr + 400;
        if (LSF) MNR0 = min(MNR0, 850);         // bitallos.cpp:214-217
        HX_WAVE_SYNC();
        if (LANE == 0) { L.call_count++; L.block_type = 2; }
        HX_WAVE_SYNC();
        bitallo_short(L, p, igr, b.ba_min, b.TargetBits, b.ba_max, b.bit_pool, ms, MNR0, L.sfs);
    }
#endif
    PROF_ACC(HX_PROF_BITALLO);
    // xr is dead from here on (packing reads ix / signx): request the next granule's
    // spectrum and mask operands now, their latency hides behind the packing
    // the helper wave hands this granule's lines to k_pack and requests the next granule's operands; joined at
    // the start of the next granule (or behind the frame loop)
    if (!HX_A1 && !fetch_posted) {
        if (LANE == 0) { L.cmdw[2] = g; L.cmdw[3] = bt | ((L.gr[igr][0].aux_not_null != 0) << 8) | ((L.gr[igr][1].aux_not_null != 0) << 9); }
        HELPER_POST(HCMD_FETCH, (g + 1 < NGs) ? g + 1 : -1);
    }
    PROF_ACC(HX_PROF_FETCH_POST);
    {   // The bits are written by k_pack; here the granule's segments are sized and handed over: a channel's
        // first bit follows from the sizes before it, because the Huffman bits were counted (aux_bits).
        Outbox &ob = L.ob[g & 1];
        if (LANE == 0) ob.has_frame = 0;
        if (!LSF && !HX_A1 && bt != 2) {
            const int bits = handover_long2(L, ob, pos, igr, !shortblock_frame, nchan);
            pos += bits;
            b.ba_min -= bits;
            b.ba_max -= bits;
            HX_WAVE_SYNC();
        } else
#pragma unroll 1
        for (int ch = 0; ch < nchan; ch++) {
#if HX_A1
            if (dual) { A1Ctx cx = {ch, 1, 0, 0}; bitallo1(L, p, gp, cx, igr, b.ba_min, b.TargetBits, b.ba_max); }
#endif
            HxGr *gg = &L.gr[igr][ch];
            const int not_null = gg->aux_not_null;
            const int start = pos;
            int sc = 0, bits = 0;
            pos = pack_sf_any<LSF>(L, pos, igr, ch, bt, !shortblock_frame && !dual, not_null, &sc, ob.seg[ch].sf);
            if (not_null) { pos += gg->aux_bits; bits = pos - start; }
            else pos = start;
            PROF_ACC(HX_PROF_PACK_SF);
            seg_out(L, &ob.seg[ch], gg, start);
            HX_WAVE_SYNC();
            if (LANE == 0) { gg->scalefac_compress = sc; gg->part2_3_length = bits; }
            b.ba_min -= bits;
            b.ba_max -= bits;
            if (dual) { b.ba_min += b.inc_min; b.ba_max += b.inc_max; }
        }
        PROF_ACC(HX_PROF_HANDOVER);
    }
    if (HX_A1) {    // (its line arrays stay live until the last channel is allocated)
        if (LANE == 0) { L.cmdw[2] = g; L.cmdw[3] = bt | ((L.gr[igr][0].aux_not_null != 0) << 8) | ((L.gr[igr][1].aux_not_null != 0) << 9); }
        HELPER_POST(HCMD_FETCH, (g + 1 < NGs) ? g + 1 : -1);
    }
    if (!dual) {
        b.ba_min += b.inc_min;
        b.ba_max = b.ba_max - b.dba_max;
        b.ba_max += b.inc_max;
    }
    HX_WAVE_SYNC();
}

// A coded frame placed: header, side information, main data (into the outbox of its last granule, for the helper wave and
// k_pack); reservoir bookkeeping.
template <int LSF>
__device__ __forceinline__ void place_frame(const AllocArgs &a, AllocLds &L, int s, int f, int part, int ms, int pos, int P_vbr PROF_CLOCK)
{
    HX_LANE_DECL;
    const AllocPrm *p = &L.P;
    const int NG = a.NG, F = NG / 2;
    // the frame's budget and the stream's carried scalars, from where the budget section left them
    const int byte_pool = RFL(L.fs.byte_pool), byte_max = RFL(L.fs.byte_max), pad = RFL(L.fs.pad);
    int byte_min = RFL(L.fs.byte_min);
    unsigned side_p0 = (unsigned) RFL((int) L.fs.side_p0), side_p1 = (unsigned) RFL((int) L.fs.side_p1);
    int main_bytes = RFL(L.fs.main_bytes), opos = RFL(L.fs.opos), slot_lo = RFL(L.fs.slot_lo), slot_hi = RFL(L.fs.slot_hi);
    unsigned main_tot = (unsigned) RFL((int) L.fs.main_tot), main_sent = (unsigned) RFL((int) L.fs.main_sent), mf_tot = (unsigned) RFL((int) L.fs.mf_tot);
    unsigned tot_frames_out = (unsigned) RFL((int) L.fs.tot_frames_out);
    int bytesout = RFL(L.fs.bytesout);
    const int pk_first = RFL(L.fs.pk_first);
    const int P_oflags = RFL(p->oflags), P_mfb = RFL(p->main_framebytes), hdr = 4 + RFL(p->side_bytes);     // header + side info: 36 bytes, 21 for mono
    const int P_ivmin = RFL(p->ivbr_min), P_ivmax = RFL(p->ivbr_max), P_fbmin = RFL(p->fbmin), P_vpt = RFL(p->vbr_pool_target);
    // VBR: lane i holds the main-data capacity of bitrate index i (and of i + 1), so that the frame's index comes from
    // two ballots instead of two scans of the table in LDS (a dependent read per step: 2.2 k cycles per frame)
    const int fb_lane = p->vbr_main_framebytes[min(LANE, 15)], fbn_lane = p->vbr_main_framebytes[min(LANE + 1, 15)];
    int ring_mf = L.r_mf[LANE & 31];    // the ring's slot sizes, one per lane: the retire loop below reads them without an LDS round trip each
    int bytes = (pos + 7) >> 3;
    if (bytes > byte_max) atomicOr(COLD(status), 2);    // the reference asserts here
    int ibr = 0;
    if (P_vbr) {
        int bytes2 = bytes - byte_pool, bytes3 = bytes2 + P_vpt;
        {   // first index in [ivmin, ivmax] whose capacity holds bytes2 (ivmax + 1: none)
            const unsigned long long m = __ballot(LANE >= P_ivmin && LANE <= P_ivmax && bytes2 <= fb_lane);
            ibr = m ? (int) __builtin_ctzll(m) : P_ivmax + 1;
        }
        // MPEG-2 frames can be so small that the pool spans many of them: past 10 pending frames stop
        // filling it, past 15 drain it through byte_min padding (reference mp3enc.cpp:2387-2411)
        const int side_dp = (int) ((side_p1 - side_p0) & 31);
        if (!LSF || side_dp < 10) {
            const unsigned long long m = __ballot(LANE >= ibr && LANE <= P_ivmax && bytes3 < fbn_lane);
            ibr = m ? (int) __builtin_ctzll(m) : P_ivmax + 1;
        } else if (side_dp > 15) {
            byte_min = P_fbmin + ((side_dp > 24) ? byte_pool : (byte_pool >> 4));
        }
        if (ibr > P_ivmax) ibr = P_ivmax;
    }
    const int raw_bytes = bytes;
    if (bytes < byte_min) bytes = byte_min;
    const int mf = P_vbr ? __builtin_amdgcn_readlane(fb_lane, ibr) : P_mfb + pad;
    long long packet_off = -1;
    if (P_oflags & 1) packet_off = ((long long) s * F + f) * COLD(packet_stride) + ((LSF && part) ? pk_first : 0) + hdr;
    PROF_ACC(HX_PROF_PL_SIZES);
    // the frame's slot, and where its main data goes (k_pack moves the bits): into the outbox of its last granule
    Outbox &ob = L.ob[LSF ? part : 1];
    if ((LANE & 31) == (int) side_p1) ring_mf = (unsigned short) mf;
    if (LANE == 0) {
        L.r_mf[side_p1] = (unsigned short) mf; L.r_off[side_p1] = opos;
        ob.slot.off = opos; ob.slot.mf = mf; ob.slot_index = slot_hi;
        ob.frm.bytes = bytes; ob.frm.raw_bytes = raw_bytes; ob.frm.first_slot = slot_lo; ob.frm.main_bytes = main_bytes; ob.frm.packet_off = packet_off;
        ob.frm_index = LSF ? 2 * f + part : f;
        ob.ring_p0 = (int) side_p0;
        ob.opos = opos;
        ob.has_frame = 1;
    }
    slot_hi++;
    PROF_ACC(HX_PROF_PL_SLOT);
    {
        if (LANE < 4) {     // header (reference mp3enc.cpp:2077-2103): pad bit / bitrate index, mode extension
            unsigned char h = p->head[LANE];
            if (LANE == 2) {
                if (!P_vbr) { if (pad) h |= 2; }
                else h = (unsigned char) ((h & 0x0F) | (ibr << 4));
            }
            if (LANE == 3) h = (unsigned char) ((h & 0xCF) | ((ms + ms + (HX_A1 ? p->is_flag : 0)) << 4));     // mode extension: M/S, intensity
            ob.head[LANE] = h;
        }
        // the side information's fields as they stand now; main_data_begin = reservoir level at frame start
        (&ob.gr[0][0].part2_3_length)[LANE] = (&L.gr[0][0].part2_3_length)[LANE];
        if (LANE < 32) (&ob.gr[0][0].part2_3_length)[64 + LANE] = (&L.gr[0][0].part2_3_length)[64 + LANE];
        if (LANE == 0) { ob.scfsi[0] = L.scfsi[0]; ob.scfsi[1] = L.scfsi[1]; ob.mdb = byte_pool; ob.part = part; }
    }
    PROF_ACC(HX_PROF_PL_HEAD);
    if (P_oflags & 1) {     // nbytes_out[2] per call; the MPEG-2 call's two packets sit back to back (mp3enc.cpp:3352-3363)
        int *nb = COLD(packet_bytes) + ((long long) s * F + f) * 2;
        unsigned char *q = COLD(packet) + ((long long) s * F + f) * COLD(packet_stride);
        if (LSF && part) q += pk_first;
        emit_packet(L, p, q, nb + part, pad, ms, raw_bytes, hdr, LSF ? part : -1);
        if (LANE == 0) L.fs.pk_first = hdr + raw_bytes;
        if (!LSF && LANE == 0) nb[1] = 0;
    }
    if (LANE == 0 && (P_oflags & 2) && (!LSF || part)) {
        HxFrameDebug *d = COLD(dbg) + (long long) s * F + f;
        d->ms = ms; d->ms_metric[0] = LSF ? 0 : COLD(msdec)[(long long) s * NG + 2 * f]; d->ms_metric[1] = COLD(msdec)[(long long) s * NG + 2 * f + 1];
        d->byte_pool = byte_pool; d->MNR_after = L.MNR;
        for (int g2 = 0; g2 < 2; g2++) for (int c = 0; c < 2; c++) {
            d->gr[g2][c] = L.gr[g2][c];
            for (int b = 0; b < 22; b++) d->sf[g2][c][b] = L.sfout[g2][c][b];
        }
        d->scfsi[0] = L.scfsi[0]; d->scfsi[1] = L.scfsi[1];
        d->main_bytes = raw_bytes;
    }
    opos += hdr + mf;
    side_p1 = (side_p1 + 1) & 31;
    HX_WAVE_SYNC();
    PROF_ACC(HX_PROF_EMIT);
    main_tot += bytes;
    main_bytes += bytes;
    mf_tot += mf;
    // retire the slots that are now full (reference mp3enc.cpp:2293-2313)
    while (side_p0 != side_p1) {
        const int cap = __builtin_amdgcn_readlane(ring_mf, (int) side_p0);
        if (main_bytes < cap) break;
        tot_frames_out++;
        main_sent += cap;
        bytesout += hdr + cap;
        main_bytes -= cap;
        side_p0 = (side_p0 + 1) & 31;
        slot_lo++;
    }
    if (LANE == 0) {
        FrameState &fs = L.fs;
        fs.side_p0 = side_p0; fs.side_p1 = side_p1; fs.main_bytes = main_bytes; fs.opos = opos; fs.slot_lo = slot_lo; fs.slot_hi = slot_hi;
        fs.main_tot = main_tot; fs.main_sent = main_sent; fs.mf_tot = mf_tot; fs.tot_frames_out = tot_frames_out; fs.bytesout = bytesout;
    }
    if (!LSF || part) {     // the call's last frame: running totals (reference mp3enc.cpp:2316-2325)
        const unsigned tot_bytes_out = (unsigned) RFL((int) L.fs.tot_bytes_out) + (unsigned) bytesout;
        const int ave0 = RFL(L.fs.ave_tot), ave_tot = ave0 + ((((bytesout << 8) - ave0)) >> (LSF ? 6 : 7));
        if (LANE == 0) { L.fs.tot_bytes_out = tot_bytes_out; L.fs.ave_tot = ave_tot; }
        if ((P_oflags & 4) && LANE < 2) COLD(frame_stats)[((long long) s * F + f) * 2 + LANE] = (int) (LANE ? tot_bytes_out : tot_frames_out);
    }
    HX_WAVE_SYNC();
}

// The counters and packet sizes of the frames behind the stream's count (hx_batch_frame_counts), frames nf .. F - 1 of its
// row: the counters repeat the stream's as they stand at the end of its call, the packets there are empty.
__device__ __forceinline__ void tail_fill(int s, int nf, int F, unsigned tot_frames_out, unsigned tot_bytes_out)
{
    HX_LANE_DECL;
    if (nf >= F) return;
    int *fs = COLD(frame_stats), *pb = COLD(packet) ? COLD(packet_bytes) : nullptr;
    for (int i = 2 * nf + LANE; i < 2 * F; i += 64) {
        if (fs) fs[(long long) s * F * 2 + i] = (int) ((i & 1) ? tot_bytes_out : tot_frames_out);
        if (pb) pb[(long long) s * F * 2 + i] = 0;
    }
}

// A launch's bookkeeping at a stream's end: its duration for the next launch's order, the retired-counter, and its position's
// CU no longer reserved (see "parking" in alloc_stream) - for every stream of the launch, one that took no frame included.
__device__ __forceinline__ void stream_retire(int s, int idx, long long t_start)
{
    COLD(dur)[s] = (unsigned) (wall_clock64() - t_start);
    __threadfence();
    atomicAdd(COLD(done_counter) + HX_CNT_RETIRED, 1);
    if (idx < (COLD(park_k) & 0xFFFF)) __hip_atomic_store((unsigned *) COLD(done_counter) + HX_CNT_PARK + idx, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A stream that takes no frame of this call (count 0): its state, its pending frames' images and its row stay as they are;
// the call's byte counts are zero, its counters those it came with.  The master wave alone, no order to the helper.
__device__ __forceinline__ void stream_idle(int s, int idx, int F, const HxStream *ss, long long t_start)
{
    HX_LANE_DECL;
    tail_fill(s, 0, F, ss->tot_frames_out, ss->tot_bytes_out);
    if (LANE == 0) {
        COLD(pre_len)[s] = 0; COLD(carry_len)[s] = 0; COLD(out_bytes)[s] = 0;
        stream_retire(s, idx, t_start);
    }
}

// The end of the stream's call: the last granule's lines and outbox out, the frames that are not complete yet and the carried
// state into the stream record, the counters.  NGs: the stream's granules of this call.
__device__ __forceinline__ void stream_writeback(const AllocArgs &a, AllocLds &L, int s, int idx, int NGs, HxStream *ss, long long t_start)
{
    HX_LANE_DECL;
    HELPER_JOIN();          // the last granule's lines are out
    if (LANE == 0) { L.cmdw[2] = -1; L.cmdw[3] = NGs - 1; }
    HELPER_POST(HCMD_FETCH, -1);        // its outbox
    HELPER_JOIN();
    // ---- frames that are not complete yet travel to the next call in the stream state ----
    HX_WAVE_SYNC();
    const unsigned side_p0 = L.fs.side_p0, side_p1 = L.fs.side_p1;
    const int opos = L.fs.opos;
    const int done = (side_p0 != side_p1) ? L.r_off[side_p0] : opos;       // bytes of complete frames in `out`
    SYNC_G();
    // (their images - with the main data k_pack writes - are copied into ss->main_buf by k_pack_carry)
    if (LANE < 32) ss->frame_mf_bytes[LANE] = L.r_mf[LANE];
#ifdef HX_PROFILE
    if (LANE == 0) L.prof[HX_PROF_TOTAL] = (unsigned) clock64() - L.prof[HX_PROF_TOTAL];
    HX_WAVE_SYNC();
    if (COLD(prof)) COLD(prof)[(long long) s * HX_PROF_WORDS + LANE] = L.prof[LANE];
#endif
    // ---- write the stream state back ----
    if (LANE < 44) ss->NTadjust[LANE / 22][LANE % 22] = L.NTadjust[LANE / 22][LANE % 22];
    if (LANE < 42) ss->sf_save[LANE / 21][LANE % 21] = L.sf_save[LANE / 21][LANE % 21];
#if HX_A1
    if (LANE < 42) ss->a1_gsf[LANE / 21][LANE % 21] = L.gsf[LANE / 21][LANE % 21];
    if (LANE == 0) {
        ss->a1_call_count = L.a_calls; ss->a1_bitadjust[0] = L.a_bitadjust[0]; ss->a1_bitadjust[1] = L.a_bitadjust[1];
        ss->a1_running_a = L.a_running; ss->a1_ave_alpha = L.a_ave; ss->a1_alpha = L.a_alpha;
    }
#endif
    if (LANE == 0) {
        ss->MNR = L.MNR; ss->PoolFraction = L.PoolFraction; ss->call_count = L.call_count;
        const FrameState &fs = L.fs;
        ss->padcount = fs.padcount;
        ss->main_tot = fs.main_tot; ss->main_sent = fs.main_sent; ss->mf_tot = fs.mf_tot;
        ss->main_bytes = fs.main_bytes; ss->main_p0 = 0; ss->main_p1 = opos - done;
        ss->side_p0 = side_p0; ss->side_p1 = side_p1;
        ss->tot_frames_out = fs.tot_frames_out; ss->tot_bytes_out = fs.tot_bytes_out; ss->ave_tot_bytes_out = fs.ave_tot;
        // (a mono stream has no second channel: bitallo_short's side information of it is formed from LDS no one wrote, and the
        // stream state - the checkpoint blob - keeps the zeros it started with)
        for (int g = 0; g < 2; g++) for (int c = 0; c < 2; c++) for (int k = 0; k < 3; k++)
            ss->gr_subblock_gain[g][c][k] = c < L.P.nchan ? L.gr[g][c].subblock_gain[k] : 0;
        COLD(out_bytes)[s] = done;
        COLD(carry_len)[s] = opos - done;
        if (L.nstrict) atomicAdd(COLD(done_counter) + HX_CNT_STRICT_SUMS, L.nstrict);
#if !HX_SLIM
        if (L.nlucky[0]) for (int k = 0; k < 3; k++) atomicAdd(COLD(done_counter) + HX_CNT_LUCKY + k, L.nlucky[k]);
#endif
        if (L.nrounds[0]) {
            for (int k = 0; k < 2; k++) atomicAdd(COLD(done_counter) + HX_CNT_LUCKY_ROUNDS + k, L.nrounds[k]);
            atomicMax(COLD(done_counter) + HX_CNT_LUCKY_ROUNDS + 2, L.nrounds[2]);
        }
        stream_retire(s, idx, t_start);
    }
    tail_fill(s, NGs / 2, a.NG / 2, L.fs.tot_frames_out, L.fs.tot_bytes_out);
}

// Out of work: a workgroup that shares its CU with one of the launch's longest streams keeps the slot until that one retires
// (see "parking" in alloc_stream); the last workgroup out resets the claim counter; the helper wave stops.
__device__ __forceinline__ void walk_exit(AllocLds &L)
{
    HX_LANE_DECL;
    const int pk = COLD(park_k) & 0xFFFF;
    if (pk > 0 && LANE == 0) {
        unsigned *resv = (unsigned *) COLD(done_counter) + HX_CNT_PARK;
        const unsigned me = ((((unsigned) __builtin_amdgcn_s_getreg((31 << 11) | 20) << 16) | ((unsigned) __builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xFFFFu)) & ((COLD(park_k) >> 16) ? 0xFFFFFE00u : 0xFFFFFF00u)) | 1u;
        for (int k = 0; k < pk; k++) {
            if (__hip_atomic_load(resv + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != me) continue;
            // (bounded: 40 ms of wall clock - nothing depends on the wait, it only keeps the slot occupied)
            const long long t_park = wall_clock64();
            while (__hip_atomic_load(resv + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == me && wall_clock64() - t_park < 4000000LL)
                __builtin_amdgcn_s_sleep(127);
        }
    }
    // the last workgroup out leaves the claim counter at zero for the next launch (launches of a batch follow each other
    // on one HIP stream; a recorded graph replays the launch with the same arguments, so nothing here may depend on the host)
    if (HX_PERSIST && LANE == 0 && atomicAdd(COLD(done_counter) + HX_CNT_IDLE, 1) == (int) gridDim.x - 1) {
        __hip_atomic_store(COLD(done_counter) + HX_CNT_CLAIMED, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(COLD(done_counter) + HX_CNT_IDLE, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    HELPER_POST(HCMD_EXIT, 0);
}

// LSF = 1: MPEG-2 low-sampling-frequency streams.  Every granule is a frame of its own (reference
// mp3enc.cpp:2483-2593 CBR, :2337-2479 VBR; encode_jointB_MPEG2 :1832-1907, encode_singleB_MPEG2
// :1977-2027): budgets in bits = bytes << 3, reservoir capped at 255 bytes, no scfsi.
template <int LSF>
__device__ __forceinline__ void alloc_stream(const AllocArgs &a, AllocLds &L)
{
    HX_LANE_DECL;
    // Persistent workgroups: the launch has as many workgroups as the chip holds at once (or one per stream if that is
    // fewer); each claims the next stream of the launch order from a counter when it is done with one.  (Round 6: with one
    // workgroup per stream and more streams than slots, the hardware dispatcher deals workgroup i to XCD i mod 8 in strict
    // order, so a freed slot of another XCD waits for its turn, and every stream's end hands LDS and registers back and takes
    // them again: config 3 48.6 -> 48.0 ms per step, four full rounds 52.9 -> 51.5 ms.  Most of what a multi-round launch
    // idles - 14 % of its slot-time - is the last round's drain, which no claiming order removes: a stream's call is one job.)
    // The launch order is the streams that ran longest in the previous call first (longest-processing-time-first: the
    // launch's tail is made of short streams).
    // (HX_PERSIST: the low-footprint build only, see the top of hx_alloc.hip)
    // (the launch walks positions pos0 .. pos0 + npos - 1 of the batch-wide launch order: AllocArgs::pos0)
    if (!HX_PERSIST && (int) blockIdx.x >= a.npos) return;
    if (WAVE == 1) { helper_serve<LSF>(a, L); return; }
#if HX_PERSIST
  for (;;) {        // master wave: one stream of the launch order after the other
    HX_LANE_DECL;
    int idx = 0;
    if (LANE == 0) idx = atomicAdd(COLD(done_counter) + HX_CNT_CLAIMED, 1);
    idx = a.pos0 + __builtin_amdgcn_readfirstlane(idx);
    if (idx >= a.pos0 + a.npos) break;
#else
  {                 // master wave: the stream at this workgroup's position of the launch order
    const int idx = a.pos0 + (int) blockIdx.x;
#endif
    const int s = COLD(order) ? COLD(order)[idx] : idx;
    const long long t_start = wall_clock64();
    if (LANE == 0) {
        L.cur_s = s;
        atomicAdd(COLD(done_counter) + HX_CNT_STARTED, 1);        // this stream is being walked (the gates of the next call's front end count these)
        // where it runs (tests, placement experiments): XCC id << 16 | HW_ID[15:0], per position in the launch order
        const unsigned where = ((unsigned) __builtin_amdgcn_s_getreg((31 << 11) | 20) << 16) | ((unsigned) __builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xFFFFu);
        COLD(dur)[a.S + idx] = where;
        // Parking (resident-set batches): a launch lasts as long as its slowest stream, and the front end of the next call and
        // the packing of the previous one move into every CU slot a retiring stream frees - also next to that slowest stream,
        // whose LDS round trips they then lengthen (measured: K6 15.0 ms alone, 16.0 ms with them beside it).  The first
        // park_k positions of the launch order (the longest streams of the previous call) publish which CU they run on; a
        // workgroup that runs out of work on one of those CUs keeps its slot - asleep - until that stream has retired too, so
        // nothing else fits there (a CU holds four of these workgroups: 153 of 160 KB of LDS, all vector registers).
        // (park_k bit 16: the CU that shares the instruction and scalar caches with it - CU id with the low bit flipped - as well)
        if (idx < (COLD(park_k) & 0xFFFF))
            __hip_atomic_store((unsigned *) COLD(done_counter) + HX_CNT_PARK + idx, (where & ((COLD(park_k) >> 16) ? 0xFFFFFE00u : 0xFFFFFF00u)) | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    HxStream *ss = a.st + s;
    // The frames this stream takes of the call (hx_batch_frame_counts; null: all of them): the bound of the frame loop and of
    // the look-ahead fetch, while a.NG stays the stride of every [S][NG] array.  A stream that takes none still did all of the
    // launch's bookkeeping above and retires (stream_idle): the gates, the claim counter's reset, the next launch's order and
    // the workgroups parked on its CU count on every position of the launch.  It gives the helper wave no order: both waves
    // go on to the next claim, or to walk_exit, together.
    const int *nfr = COLD(nfr);
    const int F = nfr ? __builtin_amdgcn_readfirstlane(nfr[s]) : a.NG / 2;
    if (F == 0) {
        stream_idle(s, idx, a.NG / 2, ss, t_start);
#if HX_PERSIST
        continue;
#endif
    } else {
    const HxParams *gp = a.prm + ss->cls;
    const AllocPrm *p = &L.P;
    const int NG = a.NG, NGs = 2 * F;
    stage_stream(a, L, ss, gp, a.gt);
    slots_init<LSF>(a, L, s, ss, gp);

    int bt_last = a.btprev[s];
    if (LANE == 0) { L.cmdw[2] = -1; L.cmdw[3] = 0; }
    HELPER_POST(HCMD_FETCH, 0);         // the first granule's operands
    for (int f = 0; f < F; f++) {
        HX_LANE_DECL;           // (per frame: see hx_lane_opaque)
        PROF_T0();
        constexpr int GFN = (int) sizeof(L.gflag);       // granules staged at a time
        // The per-granule block types and stereo decisions are staged in LDS GFN / 2 frames at a time: fetched from global
        // memory one frame ahead, the compiler unpacked (= waited for) them at once and spilled them over the frame (2 k cycles).
        if ((f & (GFN / 2 - 1)) == 0) {
            const unsigned char *bt_s = COLD(bt) + (long long) s * NG;
            const unsigned char *ms_s = COLD(msflag) + (long long) s * NG;
            HX_WAVE_SYNC();
            for (int i = LANE; i < GFN; i += 64) { const int g = 2 * f + i; L.gflag[i] = (g < NG) ? (unsigned char) (bt_s[g] | (ms_s[g] << 2)) : 0; }
            HX_WAVE_SYNC();
        }
        const int gfl = RFL((int) *reinterpret_cast<const unsigned short *>(&L.gflag[(2 * f) & (GFN - 1)]));
        const int bt0 = gfl & 3, msb1 = (gfl >> 2) & 1, bt1 = (gfl >> 8) & 3, msb2 = (gfl >> 10) & 1;
        if (LANE == 0) { L.fs.bytesout = 0; L.fs.pk_first = 0; }
        // an MPEG-1 frame holds both granules of the 1152-sample block, an MPEG-2 frame one of them
      for (int part = 0; part < (LSF ? 2 : 1); part++) {
        const int P_vbr = RFL(p->vbr_flag), nchan = RFL(p->nchan);
        const int dual = HX_A1 && RFL(p->dual);
        FrameBudget b = frame_budget<LSF>(L, P_vbr, nchan, dual);
        const int shortblock_frame = (bt0 == 2) | (bt1 == 2);
        // the frame's stereo decision was made by k_msscan (hysteresis over the stream's granules)
        const int ms = (LSF && part) ? msb2 : msb1;
        HX_WAVE_SYNC();
        PROF_ACC(HX_PROF_BUDGET);
        int pos = 0;
        for (int igr = LSF ? part : 0; igr < (LSF ? part + 1 : 2); igr++) {
            const int bt = igr ? bt1 : bt0;
            granule_alloc<LSF>(a, L, gp, s, 2 * f + igr, NGs, igr, bt, bt_last, ms, shortblock_frame, nchan, dual, P_vbr, b, pos PROF_PASS);
            bt_last = bt;
        }
        PROF_ACC(HX_PROF_GR_TAIL);
        place_frame<LSF>(a, L, s, f, part, ms, pos, P_vbr PROF_PASS);
      }
        PROF_ACC(HX_PROF_RETIRE);
    }
    stream_writeback(a, L, s, idx, NGs, ss, t_start);
#if HX_PERSIST
    // the helper wave is through with this stream (its last stores read the outbox and the stream constants in LDS) before
    // the next stream's tables land there
    HELPER_POST(HCMD_SYNC, 0);
    HELPER_JOIN();
#endif
    }
  }
    walk_exit(L);
}

// ---- k_debug_count_* (tests only; hx_debug_count): the walk's quantiser and Huffman counter on records of the caller's ----
// One workgroup of two waves per record, as the walk has them: the master stages the class's tables (stage_stream), copies
// the record into LDS and calls the functions the rate loop calls; the helper wave serves its work orders (helper_serve), so
// channel 1 is quantised and counted where the walk does it.  What the functions left in LDS goes back out.  One kernel per
// stream-walk unit, built with that unit's macros and flags in the unit's twin (HX_TAP, below); the host (hx_batch.hip) has checked every record: nothing a
// record's value indexes can leave its bounds.  The kernel's first argument is an AllocArgs, which COLD() reads.
// The same kernel serves hx_debug_seek: from HX_DS_SEEK on, HxCountArgs::mode names a noise mode (debug_seek, below).
#if !HX_A1
// The noise modes (hx_debug_seek; HxDebugSeek in hx_types.h): the master has staged the tables; it copies record r into LDS
// where startup and the rate loop would have left the values, calls seek_actual or inverse_sf2 as allocate() does - channel 1
// goes to the helper wave through HCMD_SEEK / HCMD_ISF2 from inside them - and hands back what they left.  The double-table
// counter is the record's own result word, not the launch's.
__device__ __forceinline__ void debug_seek(const HxCountArgs &c, AllocLds &L, long long r)
{
    HX_LANE_DECL;
    const AllocPrm *p = &L.P;
    const int *h = c.hdr + r * HX_DSH_WORDS;
    int *out = c.out + r * HX_DSO_WORDS;
    const bool isf2 = c.mode == HX_DS_ISF2;
    const int nchan = h[HX_DSH_NCHAN];
    if (LANE < 2) {
        const bool on = LANE < nchan;
        L.P.nsf[LANE] = on ? h[HX_DSH_NSF0 + LANE] : 0;
        L.P.nbmax[LANE] = on ? h[HX_DSH_NBMAX0 + LANE] : 0;
        L.G[LANE] = h[HX_DSH_G0 + LANE]; L.scale[LANE] = h[HX_DSH_SCALE0 + LANE];
    }
    if (LANE == 0) { L.nchan = nchan; L.P.nchan = nchan; L.big_counter = out + HX_DSO_BIG; }
    for (int i = LANE; i < 2 * 576; i += 64) {
        (&L.xr[0][0])[i] = c.xr[r * 1152 + i];
        (&L.x34[0][0])[i] = isf2 ? 0.0f : c.x34[r * 1152 + i];
    }
    if (isf2) for (int i = LANE; i < 2 * 576; i += 64) IX(0)[i] = (ix_t) c.ix[r * 1152 + i];
    if (LANE < 2 * NB) {
        const int ch = LANE / NB, b = LANE % NB;
        const int *w = c.band + ((r * 2 + ch) * NB + b) * HX_DSB_WORDS;
        if (isf2) { L.up[ch][b] = w[HX_DSB_UP]; L.lo[ch][b] = w[HX_DSB_LO]; L.sf[ch][b] = w[HX_DSB_SF]; L.ixmax[ch][b] = w[HX_DSB_IXMAX]; }
        else {
            L.NT[ch][b] = w[HX_DSB_NT]; L.Noise0[ch][b] = w[HX_DSB_NOISE0]; L.gsf[ch][b] = w[HX_DSB_GSF]; L.gzero[ch][b] = w[HX_DSB_GZERO];
            L.NTadjust[ch][b] = w[HX_DSB_NTADJUST]; L.x34max[ch][b] = c.x34max[(r * 2 + ch) * NB + b];
        }
    }
    HX_WAVE_SYNC();
    if (isf2) inverse_sf2(L, p);
    else seek_actual(L, p);
    HX_WAVE_SYNC();
    if (LANE < 2 * NB) {
        const int ch = LANE / NB, b = LANE % NB;
        int *o = out + HX_DSO_BAND * LANE;
        if (isf2) { o[0] = L.sf[ch][b]; o[1] = L.geval[ch][b]; }
        else { o[0] = L.gsf[ch][b]; o[1] = L.Noise[ch][b]; o[2] = L.NTadjust[ch][b]; o[3] = L.geval[ch][b]; }
    }
    if (LANE == 0) out[HX_DSO_NSTRICT] = L.nstrict;
}
#endif

template <int LSF>
__device__ __forceinline__ void debug_count(const AllocArgs &a, const HxCountArgs &c, AllocLds &L)
{
    HX_LANE_DECL;
    if ((int) blockIdx.x >= c.n) return;
    if (WAVE == 1) { helper_serve<LSF>(a, L); return; }
    const long long r = blockIdx.x;
    const AllocPrm *p = &L.P;
    stage_stream(a, L, a.st, a.prm, a.gt);
#if !HX_A1
    if (c.mode >= HX_DS_SEEK) { debug_seek(c, L, r); HELPER_POST(HCMD_EXIT, 0); return; }
#endif
    const int *h = c.hdr + r * HX_DCH_WORDS;
    const int mode = c.mode, nchan = h[HX_DCH_NCHAN], opt = h[HX_DCH_OPT], zero21 = h[HX_DCH_ZERO21];
    const bool shortm = mode == HX_DC_SHORT || mode == HX_DC_SHORT_COUNT;
    const bool quant = mode == HX_DC_QUANT_COUNT || mode == HX_DC_QUANT_THEN_COUNT || mode == HX_DC_SHORT;
    if (LANE < 2) {
        const bool on = LANE < nchan;
        if (!shortm) {
            // (the band count a channel is counted to: the rate loop passes one of the class's arrays; here nsf2 holds the record's)
            L.P.nsf2[LANE] = on ? h[HX_DCH_NCB0 + LANE] : 0;
            L.P.nsf[LANE] = on ? h[(mode == HX_DC_COUNT ? HX_DCH_NCB0 : HX_DCH_NSF0) + LANE] : 0;
            L.P.nbmax[LANE] = on ? h[HX_DCH_NBMAX0 + LANE] : 0;
        }
        for (int k = 0; k < 4; k++) L.hs_table[LANE][k] = 0;
        for (int k = 0; k < 3; k++) L.hs_cbreg[LANE][k] = 0;
        L.hs_nbig[LANE] = 0; L.hs_nquads[LANE] = 0; L.hs_bits[LANE] = 0;
    }
    if (LANE == 0) { L.block_type = shortm ? 2 : h[HX_DCH_BT]; L.nchan = nchan; L.P.nchan = nchan; }
    for (int i = LANE; i < 2 * 576; i += 64) {
        IX(0)[i] = (ix_t) c.ix[r * 1152 + i];          // (channel 1's lines follow channel 0's in both layouts)
        (&L.x34[0][0])[i] = quant ? c.x34[r * 1152 + i] : 0.0f;
    }
    if (!shortm) {
        if (LANE < 2 * NB) {
            const int ch = LANE / NB, b = LANE % NB;
            L.ixmax[ch][b] = c.ixmax[(r * 2 + ch) * NB + b];
            if (quant) L.gsf[ch][b] = c.gsf[(r * 2 + ch) * NB + b];
        }
    } else {
        for (int i = LANE; i < 2 * 48; i += 64) {
            (&L.s_ixmax[0][0][0])[i] = c.ixmax[r * 96 + i];
            if (quant) (&L.s_gsf[0][0][0])[i] = (sgs_t) c.gsf[r * 96 + i];
        }
    }
    HX_WAVE_SYNC();
    int bits = 0;
    if (mode == HX_DC_COUNT) {
#if HX_A1
        const A1Ctx cx = {0, nchan, 0, 0};
        bits = a1_count_channels(L, p, cx);
#else
        bits = count_bits(L, p, p->nsf2);
#endif
    } else if (mode == HX_DC_QUANT_COUNT) bits = quant_count_bits(L, p, opt, zero21, p->nsf2);
    else if (mode == HX_DC_QUANT_THEN_COUNT) {      // as bitallo_long and requant_count do it while -HF lines are quantised in between
        do_quant(L, p, opt);
        if (zero21) { if (LANE == 0) L.ixmax[0][21] = 0; HX_WAVE_SYNC(); }
        bits = count_bits(L, p, p->nsf2);
    } else {
        if (mode == HX_DC_SHORT) s_do_quant(L, p, opt);
        bits = s_count_bits_ch(L, p, 0);
        if (nchan == 2) bits += s_count_bits_ch(L, p, 1);
    }
    HX_WAVE_SYNC();
    for (int i = LANE; i < 2 * 576; i += 64) c.ix[r * 1152 + i] = IX(0)[i];
    if (!shortm) { if (LANE < 2 * NB) c.ixmax[r * 2 * NB + LANE] = L.ixmax[LANE / NB][LANE % NB]; }
    else for (int i = LANE; i < 2 * 48; i += 64) c.ixmax[r * 96 + i] = (&L.s_ixmax[0][0][0])[i];
    if (LANE < 2) {
        int *o = c.out + r * HX_DCO_WORDS + HX_DCO_CH * LANE;
        for (int k = 0; k < 4; k++) o[HX_DCO_TABLE + k] = L.hs_table[LANE][k];
        for (int k = 0; k < 3; k++) o[HX_DCO_CBREG + k] = L.hs_cbreg[LANE][k];
        o[HX_DCO_NBIG] = L.hs_nbig[LANE]; o[HX_DCO_NQUADS] = L.hs_nquads[LANE]; o[HX_DCO_BITS] = L.hs_bits[LANE];
    }
    if (LANE == 0) c.out[r * HX_DCO_WORDS + HX_DCO_SUM] = bits;
    HELPER_POST(HCMD_EXIT, 0);
}

// The two instantiations live in separate translation units (hx_alloc.hip, hx_alloc_lsf.hip): with a
// single caller the allocator's device functions are inlined into the kernel; sharing them between
// two kernels of one module turns them into real calls (measured: +2 ms on the MPEG-1 kernel).
// The stream walk's waves issue ahead of the front-end and packing waves that share a SIMD with them in the launch's tail
// (measured: +0.6 % config 2, +0.8 % config 3).
#define HX_K6_PRIO __builtin_amdgcn_s_setprio(3)
// Each unit has a twin (hx_count*.hip, HX_TAP) that holds the test tap k_debug_count_* in the stream walk's place: the same
// sources, macros and flags in a code object of its own.  A second kernel beside the walk's would change what the inliner and
// the register allocation across calls make of the walk (tried: every function of the unit came out different).
#if HX_TAP
#define HX_K6(name, tap, lsf) \
    __global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(HX_WAVES, HX_WAVES))) void tap(AllocArgs a, HxCountArgs c) { __shared__ AllocLds L; debug_count<lsf>(a, c, L); }
#else
#define HX_K6(name, tap, lsf) \
    __global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(HX_WAVES, HX_WAVES))) void name(AllocArgs a) { HX_K6_PRIO; __shared__ AllocLds L; alloc_stream<lsf>(a, L); }
#endif
#if HX_A1 && !HX_LSF
// streams of the first-generation allocator (intensity stereo, dual channel), MPEG-1 rates
HX_K6(k_alloc1, k_debug_count_a1, 0)
#elif HX_A1
HX_K6(k_alloc1_lsf, k_debug_count_a1_lsf, 1)
#elif !HX_LSF && HX_SLIM
// low-footprint layout, three waves per SIMD: six streams per CU (hx_alloc_slim.hip)
#ifndef HX_PROFILE
static_assert(sizeof(AllocLds) <= 26880, "six workgroups of the low-footprint stream walk must fit a CU's 160 KB of LDS, which is handed out in pieces of 1280 bytes");
#endif
HX_K6(k_alloc_slim, k_debug_count_slim, 0)
#elif !HX_LSF
#ifndef HX_PROFILE
static_assert(sizeof(AllocLds) <= 40960, "four workgroups of the stream walk must fit a CU's 160 KB of LDS, which is handed out in pieces of 1280 bytes");
#endif
HX_K6(k_alloc, k_debug_count, 0)
#else
// the same stream walk for MPEG-2 LSF batches (16 / 22.05 / 24 kHz)
HX_K6(k_alloc_lsf, k_debug_count_lsf, 1)
#endif
