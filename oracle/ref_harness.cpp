/*
 * ref_harness.cpp - C-callable shim around the REAL reference encoder, compiled only by
 * `make -C oracle ref` against the sources where they lie under /root/reference (nothing of
 * the reference is copied into this repo).  Output: oracle/_ref/libhmp3ref.so (git-ignored).
 * TEST INFRASTRUCTURE: used to pin the oracle restatement and as bench.py's cpu_baseline
 * ("kind": "reference").  Never loaded by the product.
 *
 * The reference keeps process-global scratch (bit writer, sbt buffers ...), so callers must
 * drive one encoder at a time from one thread; interleaving frame-by-frame is fine.
 */
#include <vector>
#include <cstring>
#include <cstdio>
#include <malloc.h>
#define private public
#define protected public
#include "mp3enc.h"
#include "mp3low.h"
#include "srcc.h"
#undef private
#undef protected

extern "C" {

/* the reference's sample-format / sample-rate converter on its own (pins hmp3_amd/csrc/hx_src.cpp) */
void *ref_src_new(void) { return new Csrc; }
void ref_src_free(void *h) { delete (Csrc *) h; }
int ref_src_init(void *h, int source, int channels, int bits, int is_float, int target, int target_channels, int *cutoff)
{
    return ((Csrc *) h)->sr_convert_init(source, channels, bits, is_float, target, target_channels, cutoff);
}
int ref_src_convert(void *h, unsigned char *xin, float *yout, int *out_bytes)
{
    IN_OUT x = ((Csrc *) h)->sr_convert(xin, yout);
    *out_bytes = x.out_bytes;
    return x.in_bytes;
}
/* the reference's bit writer on a list of segments (pins hxo_pack_frame, oracle/hxo.h, which documents the arguments, and
 * through it k_pack): L3_outbits_init, per segment the scalefactor fields through L3_outbits - the value as the signed int
 * the reference would pass - then L3_pack_huff, then L3_outbits_flush.  L3_pack_huff reports the writer's position against
 * a file static that only the scalefactor packers set, so a segment's length is the difference of two positions, each asked
 * for with a granule record that codes nothing. */
int ref_pack_frame(int nseg, const int *hdr, const int *fld_val, const int *fld_len, int *ix, unsigned char *sign,
                   unsigned char *out, int *seg_bits)
{
    GR none;
    memset(&none, 0, sizeof(none));
    L3_outbits_init(out);
    for (int s = 0; s < nseg; s++) {
        const int *h = hdr + 9 * s;
        const int start = L3_pack_huff(&none, ix, sign);
        for (int j = 0; j < 40; j++)
            if (fld_len[40 * s + j] >= 0) L3_outbits((unsigned int) fld_val[40 * s + j], fld_len[40 * s + j]);
        if (h[0]) {
            GR g;
            memset(&g, 0, sizeof(g));
            g.aux_nreg[0] = h[1]; g.aux_nreg[1] = h[2]; g.aux_nreg[2] = h[3];
            g.big_values = h[1] + h[2] + h[3];
            g.aux_nquads = h[4];
            g.table_select[0] = h[5]; g.table_select[1] = h[6]; g.table_select[2] = h[7];
            g.count1table_select = h[8];
            L3_pack_huff(&g, ix + 576 * s, sign + 576 * s);
        }
        seg_bits[s] = L3_pack_huff(&none, ix, sign) - start;
    }
    return L3_outbits_flush();
}

/* CMp3Enc::MP3_audio_encode_init / MP3_audio_encode with every argument */
struct ZeroHeap;
int ref_init_mp3(void *h, E_CONTROL *ec, int bits, int is_float, int mpeg_select, int mono_convert)
{
    mallopt(M_PERTURB, 0xFF);
    struct Restore { ~Restore() { mallopt(M_PERTURB, 0); } } restore;
    return ((CMp3Enc *) h)->MP3_audio_encode_init(ec, bits, is_float, mpeg_select, mono_convert);
}
int ref_encode_mp3(void *h, unsigned char *pcm, unsigned char *out, int *in_bytes)
{
    IN_OUT x = ((CMp3Enc *) h)->MP3_audio_encode(pcm, out);
    *in_bytes = x.in_bytes;
    return x.out_bytes;
}

/* The reference reads members that its constructors and init functions never set (found by tools/fuzz_oracle_vs_ref.py
 * --a1: the first-generation allocator's output for impulses on silence depended on what earlier encoders of the
 * process had left on the heap).  A process that creates one encoder - the reference's own command line - gets them
 * from fresh, zero-filled pages; this harness pins that behaviour for every encoder it creates: while the encoder
 * object and the objects its init function allocates are created, glibc's allocator hands out zero-filled blocks
 * (M_PERTURB with 0xFF fills an allocated block with the complement, 0x00). */
struct ZeroHeap { ZeroHeap() { mallopt(M_PERTURB, 0xFF); } ~ZeroHeap() { mallopt(M_PERTURB, 0); } };
void *ref_new(void) { ZeroHeap z; return new CMp3Enc; }
void ref_free(void *h) { delete (CMp3Enc *) h; }
int ref_init(void *h, E_CONTROL *ec) { ZeroHeap z; return ((CMp3Enc *) h)->L3_audio_encode_init(ec); }
int ref_init_s16(void *h, E_CONTROL *ec) { ZeroHeap z; return ((CMp3Enc *) h)->MP3_audio_encode_init(ec, 16, 0, 0, 0); }
int ref_encode(void *h, float *pcm, unsigned char *out) { return ((CMp3Enc *) h)->L3_audio_encode(pcm, out).out_bytes; }
int ref_encode_packet(void *h, float *pcm, unsigned char *out, unsigned char *packet, int *nbytes)
{
    int nb[2] = {0, 0};
    int n = ((CMp3Enc *) h)->L3_audio_encode_Packet(pcm, out, packet, nb).out_bytes;
    nbytes[0] = nb[0]; nbytes[1] = nb[1];
    return n;
}
int ref_encode_s16(void *h, short *pcm, unsigned char *out) { return ((CMp3Enc *) h)->MP3_audio_encode((unsigned char *) pcm, out).out_bytes; }
unsigned ref_frames(void *h) { return ((CMp3Enc *) h)->L3_audio_encode_get_frames(); }
void ref_info_ec(void *h, E_CONTROL *ec) { ((CMp3Enc *) h)->L3_audio_encode_info_ec(ec); }
/* the reference's bitrate getters (pin tests/enc_cases.py's restatement of the running average, get_bitrate2_float) */
float ref_bitrate_float(void *h) { return ((CMp3Enc *) h)->L3_audio_encode_get_bitrate_float(); }
float ref_bitrate2_float(void *h) { return ((CMp3Enc *) h)->L3_audio_encode_get_bitrate2_float(); }
int ref_bitrate(void *h) { return ((CMp3Enc *) h)->L3_audio_encode_get_bitrate(); }

/* encode nframes of int16 stereo PCM in one call (timing loop for bench.py's cpu_baseline) */
long ref_encode_stream_s16(void *h, short *pcm, int nframes, unsigned char *out, long out_cap)
{
    CMp3Enc *e = (CMp3Enc *) h;
    long n = 0;
    for (int f = 0; f < nframes; f++) {
        if (out_cap - n < 8192) n = 0;     /* timing use: wrap instead of overflowing */
        n += e->MP3_audio_encode((unsigned char *) (pcm + 2304 * f), out + n).out_bytes;
    }
    return n;
}

/* snapshot of the members the oracle mirrors (pub/mp3enc.h:241-291, pub/bitallo3.h) */
typedef struct {
    float sample[2][4][576];
    float xr[2][2][576];
    float sig_mask[2][36][2];
    int ix[2][576];
    unsigned char signx[2][576];
    int sf_l[2][2][23];
    int gr[2][2][26];
    int scfsi[2];
    int attack_buf[2][32];
    float ecsave[2][64];
    int igrx, byte_pool, MNR, PoolFraction, call_count, ms_correlation_memory;
    int NTadjust[2][22];
    int nsb_limit, nsb_limitMS[2], band_limit, AveTargetBits, main_framebytes, initialMNR, nsf[2];
} ref_dump_t;

void ref_dump(void *h, ref_dump_t *d)
{
    CMp3Enc *e = (CMp3Enc *) h;
    CBitAllo3 *b = (CBitAllo3 *) e->BitAllo;
    memcpy(d->sample, e->sample, sizeof(d->sample));
    memcpy(d->xr, e->xr, sizeof(d->xr));
    memcpy(d->sig_mask, e->sig_mask, sizeof(d->sig_mask));
    memcpy(d->ix, e->ix, sizeof(d->ix));
    memcpy(d->signx, e->signx, sizeof(d->signx));
    for (int g = 0; g < 2; g++)
        for (int c = 0; c < 2; c++) {
            memcpy(d->sf_l[g][c], e->sf[g][c].l, sizeof(int) * 23);
            memcpy(d->gr[g][c], &e->side_info.gr[g][c], sizeof(int) * 26);
        }
    d->scfsi[0] = e->side_info.scfsi[0];
    d->scfsi[1] = e->side_info.scfsi[1];
    memcpy(d->attack_buf, e->attack_buf, sizeof(d->attack_buf));
    memcpy(d->ecsave[0], e->ecsave[0][0], sizeof(float) * 64);
    memcpy(d->ecsave[1], e->ecsave[1][0], sizeof(float) * 64);
    d->igrx = e->igrx;
    d->byte_pool = e->byte_pool;
    d->MNR = b->MNR;
    d->PoolFraction = b->PoolFraction;
    d->call_count = b->call_count;
    d->ms_correlation_memory = b->ms_correlation_memory;
    memcpy(d->NTadjust, b->NTadjust, sizeof(d->NTadjust));
    d->nsb_limit = e->nsb_limit;
    d->nsb_limitMS[0] = e->nsb_limitMS[0];
    d->nsb_limitMS[1] = e->nsb_limitMS[1];
    d->band_limit = e->band_limit;
    d->AveTargetBits = e->AveTargetBits;
    d->main_framebytes = e->main_framebytes;
    d->initialMNR = b->initialMNR;
    d->nsf[0] = b->nsf[0];
    d->nsf[1] = b->nsf[1];
}

/* psy tables as generated by amod_initLong/Short for the handle's configuration */
void ref_psy_tables(void *h, int *nsumL, int *cntoffL, float *wL, int *nsumS, int *cntoffS, float *wS)
{
    CMp3Enc *e = (CMp3Enc *) h;
    memcpy(nsumL, e->nsum, sizeof(int) * 68);
    memcpy(cntoffL, e->spd_cntl, sizeof(int) * 130);
    memcpy(wL, e->w_spd, sizeof(float) * 2200);
    memcpy(nsumS, e->nsumShort, sizeof(int) * 68);
    memcpy(cntoffS, e->spd_cntlShort, sizeof(int) * 130);
    memcpy(wS, e->w_spdShort, sizeof(float) * 1000);
}

/* The reference's quantisers and Huffman counters on the records of the quantise-and-count tests (tests/count_cases.py; the
 * layout is hx_debug_count's, include/hmp3_amd.h; pins hxo_count_record / hxo_count_record_short, oracle/hxo.h).  h: an
 * encoder initialised with a control of the second-generation allocator, whose band tables the allocator objects hold.
 * Long records: vect_quant / vect_quantB band by band as CBitAllo3::quant / quantB walk them (quant = 1), then
 * CBitAllo::subdivide2 (which goes on to subdivide2BT13 at block types 1 and 3) per channel on the record's own arrays - ix is
 * [2][576] like CMp3Enc::ix, so what a last quadruple reads behind channel 0 is channel 1 - and output_subdivide2, the one
 * way to what subdivide2 keeps in file statics.  out [2][12] per channel: {bits returned, table_select[3],
 * count1table_select, big_values, region0_count, region1_count, aux_nreg[3], aux_nquads}. */
int ref_count_record(void *h, int quant, const int *hdr, int *ix, int *ixmax, float *x34, const int *gsf, int *out)
{
    CBitAllo3 *b = (CBitAllo3 *) ((CMp3Enc *) h)->BitAllo;
    const int bt = hdr[0], nchan = hdr[1], opt = hdr[4], zero21 = hdr[5];
    const int saved_bt = b->block_type;
    int bits = 0;
    memset(out, 0, 2 * 12 * sizeof(int));
    if (quant) {
        for (int ch = 0; ch < nchan; ch++) {
            float *x = x34 + 576 * ch;
            int *qx = ix + 576 * ch;
            for (int i = 0; i < hdr[6 + ch]; i++) {
                const int n = b->nBand_l[i];
                ixmax[22 * ch + i] = (opt & 1) ? vect_quantB(x, qx, gsf[22 * ch + i], n) : vect_quant(x, qx, gsf[22 * ch + i], n);
                x += n; qx += n;
            }
        }
        if (zero21) ixmax[21] = 0;
    }
    b->block_type = bt;
    for (int ch = 0; ch < nchan; ch++) {
        int *o = out + 12 * ch;
        GR g;
        memset(&g, 0, sizeof(g));
        o[0] = b->subdivide2(ixmax + 22 * ch, ix + 576 * ch, hdr[2 + ch], 1, ch);
        b->output_subdivide2(&g, ch);
        o[1] = g.table_select[0]; o[2] = g.table_select[1]; o[3] = g.table_select[2]; o[4] = g.count1table_select;
        o[5] = g.big_values; o[6] = g.region0_count; o[7] = g.region1_count;
        o[8] = g.aux_nreg[0]; o[9] = g.aux_nreg[1]; o[10] = g.aux_nreg[2]; o[11] = g.aux_nquads;
        bits += o[0];
    }
    b->block_type = saved_bt;
    return bits;
}
/* Short records: vect_quant, or vect_quantB2 with the first offset at -0.30 (opt), band by band as CBitAlloShort::quant /
 * quantB walk them, then CBitAlloShort::subdivide2 per channel.  out [2][10] per channel: what subdivide2 saved -
 * {ntable_out[4], cbreg[3], nbig, nquads, bits}; returns the sum. */
int ref_count_record_short(void *h, int quant, const int *hdr, int *ix, int *ixmax, float *x34, const int *gsf, int *out)
{
    CBitAlloShort *s = &((CBitAllo3 *) ((CMp3Enc *) h)->BitAllo)->BitAlloShort;
    const int nchan = hdr[1], opt = hdr[4];
    int bits = 0;
    memset(out, 0, 2 * 10 * sizeof(int));
    for (int ch = 0; ch < nchan; ch++) {
        if (quant)
            for (int w = 0; w < 3; w++) {
                float *x = x34 + (3 * ch + w) * 192;
                int *qx = ix + (3 * ch + w) * 192;
                for (int i = 0; i < s->nsf[ch]; i++) {
                    const int n = s->nBand_s[i], g = gsf[(3 * ch + w) * 16 + i];
                    ixmax[(3 * ch + w) * 16 + i] = opt ? vect_quantB2(x, qx, g, n, -.30f) : vect_quant(x, qx, g, n);
                    x += n; qx += n;
                }
            }
        int *o = out + 10 * ch;
        bits += s->subdivide2((int (*)[16]) (ixmax + 48 * ch), (int (*)[192]) (ix + 576 * ch), s->nsf[ch], ch);
        for (int k = 0; k < 4; k++) o[k] = s->save[ch].ntable_out[k];
        for (int k = 0; k < 3; k++) o[4 + k] = s->save[ch].cbreg[k];
        o[7] = s->save[ch].nbig; o[8] = s->save[ch].nquads; o[9] = s->save[ch].bits;
    }
    return bits;
}
/* The reference's gain search and scalefactor refinement on the records of the noise-search tests (tests/noise_cases.py; the
 * layout is hx_debug_seek's, include/hmp3_amd.h; pins hxo_seek_record / hxo_isf2_record, oracle/hxo.h).  h: an encoder
 * initialised with a control of the second-generation allocator.  The record's values go into the allocator object's members,
 * CBitAllo3::noise_seek_actual (with ifnc_noise_actual, decrease_noise and increase_noise behind it) or CBitAllo3::inverse_sf2
 * runs on them, and the object is put back byte for byte.  out [2][22][4]: seek {gsf, Noise, NTadjust, 0}, isf2 {sf, 0, 0, 0}. */
void ref_seek_record(void *h, const int *hdr, float *xr, const float *x34, const int *band, int *out)
{
    CBitAllo3 *b = (CBitAllo3 *) ((CMp3Enc *) h)->BitAllo;
    std::vector<char> saved(sizeof(*b));
    memcpy(saved.data(), (void *) b, sizeof(*b));
    b->nchan = hdr[0]; b->nsf[0] = hdr[1]; b->nsf[1] = hdr[2];
    b->xr = (float (*)[576]) xr;
    memcpy(b->x34, x34, sizeof(b->x34));
    for (int ch = 0; ch < 2; ch++) for (int i = 0; i < 22; i++) {
        const int *w = band + (22 * ch + i) * 8;
        b->NT[ch][i] = w[0]; b->Noise0[ch][i] = w[1]; b->gsf[ch][i] = w[2]; b->gzero[ch][i] = w[3]; b->NTadjust[ch][i] = w[4];
        b->Noise[ch][i] = 0;
    }
    b->noise_seek_actual();
    for (int ch = 0; ch < 2; ch++) for (int i = 0; i < 22; i++) {
        int *o = out + 4 * (22 * ch + i);
        o[0] = b->gsf[ch][i]; o[1] = b->Noise[ch][i]; o[2] = b->NTadjust[ch][i]; o[3] = 0;
    }
    memcpy((void *) b, saved.data(), sizeof(*b));
}
void ref_isf2_record(void *h, const int *hdr, float *xr, int *ix, const int *band, int *out)
{
    CBitAllo3 *b = (CBitAllo3 *) ((CMp3Enc *) h)->BitAllo;
    std::vector<char> saved(sizeof(*b));
    int up[2][22], lo[2][22];
    memcpy(saved.data(), (void *) b, sizeof(*b));
    b->nchan = hdr[0]; b->nsf[0] = hdr[1]; b->nsf[1] = hdr[2];
    b->xr = (float (*)[576]) xr;
    b->ix = (int (*)[576]) ix;
    for (int ch = 0; ch < 2; ch++) {
        b->G[ch] = hdr[5 + ch]; b->scalefactor_scale[ch] = hdr[7 + ch];
        b->psf_upper_limit[ch] = up[ch]; b->psf_lower_limit[ch] = lo[ch];
        for (int i = 0; i < 22; i++) {
            const int *w = band + (22 * ch + i) * 8;
            up[ch][i] = w[0]; lo[ch][i] = w[1]; b->sf[ch][i] = w[2]; b->ixmax[ch][i] = w[3];
        }
    }
    b->inverse_sf2();
    for (int ch = 0; ch < 2; ch++) for (int i = 0; i < 22; i++) {
        int *o = out + 4 * (22 * ch + i);
        o[0] = b->sf[ch][i]; o[1] = o[2] = o[3] = 0;
    }
    memcpy((void *) b, saved.data(), sizeof(*b));
}
/* The reference's front end between the polyphase filter and the allocator on one granule of the caller's (tests/spec_cases.py;
 * pins hxo_spec_record, oracle/hxo.h, which documents the arguments): FreqInvert on copies of the two blocks per channel,
 * hybridLong + antialias or hybridShort with the encoder's nsb_limitMS[0], the allocator object's ms_correlation2 (CBitAllo3's,
 * with ms_correlation_memory zeroed around the call, or CBitAllo1's) when want_metric, then L3acousticQuick - emapLong +
 * spd_smrLongEcho or emapShort + spd_smrShort with the encoder's tables - per channel on a zeroed pre-echo memory.  The
 * reference hands out no partition table: esave [2][64] is the memory it leaves (twice the unclamped thresholds; short: twice
 * window 2's sums), sm [2][36][2] the {sig, mask} pairs.  The encoder's members are put back. */
void ref_spec_record(void *h, const float *prev, const float *cur, int bt, int nchan, int want_metric, float *xr, float *esave, float *sm, int *metric)
{
    CMp3Enc *e = (CMp3Enc *) h;
    const int nsb = e->nsb_limitMS[0];
    float a[576], b[576], xr_saved[2][576], ec_saved[2][2][64], eng_saved[3][64];
    SIG_MASK sm_saved[2][36];
    memset(xr, 0, 2 * 576 * sizeof(float));
    memset(esave, 0, 2 * 64 * sizeof(float));
    memset(sm, 0, 2 * 72 * sizeof(float));
    for (int ch = 0; ch < nchan; ch++) {
        memcpy(a, prev + 576 * ch, sizeof a);
        memcpy(b, cur + 576 * ch, sizeof b);
        FreqInvert(a, nsb);
        FreqInvert(b, nsb);
        if (bt != 2) { hybridLong(a, b, xr + 576 * ch, bt, nsb, 1); antialias(xr + 576 * ch, nsb); }
        else hybridShort(a, b, xr + 576 * ch, nsb);
    }
    *metric = 0;
    if (want_metric) {
        CBitAllo3 *b3 = dynamic_cast<CBitAllo3 *>(e->BitAllo);
        const int mem = b3 ? b3->ms_correlation_memory : 0;
        if (b3) b3->ms_correlation_memory = 0;
        *metric = e->BitAllo->ms_correlation2((float (*)[576]) xr, bt);
        if (b3) b3->ms_correlation_memory = mem;
    }
    memcpy(xr_saved, e->xr[0], sizeof xr_saved); memcpy(ec_saved, e->ecsave, sizeof ec_saved);
    memcpy(eng_saved, e->eng, sizeof eng_saved); memcpy(sm_saved, e->sig_mask, sizeof sm_saved);
    for (int ch = 0; ch < nchan; ch++) {
        memcpy(e->xr[0][ch], xr + 576 * ch, 576 * sizeof(float));
        memset(e->ecsave[ch][0], 0, 64 * sizeof(float));
        memset(e->sig_mask[ch], 0, sizeof(e->sig_mask[ch]));
        e->L3acousticQuick(ch, 0, bt, 0);
        memcpy(esave + 64 * ch, e->ecsave[ch][0], 64 * sizeof(float));
        for (int i = 0; i < 36; i++) { sm[72 * ch + 2 * i] = e->sig_mask[ch][i].sig; sm[72 * ch + 2 * i + 1] = e->sig_mask[ch][i].mask; }
    }
    memcpy(e->xr[0], xr_saved, sizeof xr_saved); memcpy(e->ecsave, ec_saved, sizeof ec_saved);
    memcpy(e->eng, eng_saved, sizeof eng_saved); memcpy(e->sig_mask, sm_saved, sizeof sm_saved);
}
/* the three quantisers on one run of lines (rule 0 = vect_quant, 1 = vect_quantB, 2 = vect_quantB2 at -0.30); returns the maximum */
int ref_quant_lines(int rule, float *x34, int *ix, int gsf, int n)
{
    return rule == 0 ? vect_quant(x34, ix, gsf, n) : (rule == 1 ? vect_quantB(x34, ix, gsf, n) : vect_quantB2(x34, ix, gsf, n, -.30f));
}
/* the band tables the handle's allocators hold: long {nBand_l[22], startBand_l[24]}, short {nBand_s[13], startBand_s[14], nsf} */
void ref_band_tables(void *h, int *tl, int *ts)
{
    CBitAllo3 *b = (CBitAllo3 *) ((CMp3Enc *) h)->BitAllo;
    memcpy(tl, b->nBand_l, 22 * sizeof(int)); memcpy(tl + 22, b->startBand_l, 24 * sizeof(int));
    memcpy(ts, b->BitAlloShort.nBand_s, 13 * sizeof(int)); memcpy(ts + 13, b->BitAlloShort.startBand_s, 14 * sizeof(int));
    ts[27] = b->BitAlloShort.nsf[0];
}

/* stage functions of the reference, callable on their own (mp3low.h, pub/balow.h) */
int ref_mbLogC(float x) { return mbLogC(x); }
float ref_mbExp(int x) { return mbExp(x); }
void ref_fpow34(float *x, float *y, int n) { vect_fpow34(x, y, n); }
void ref_sbt_L3(float *vbuf, float *samp) { sbt_init(); sbt_L3(vbuf, samp); }
void ref_tables_init(int sr_index, int band_limit) { L3table_init(sr_index, 1, band_limit); }
void ref_FreqInvert(float *y, int nsb) { FreqInvert(y, nsb); }
void ref_hybridLong(float *x1, float *x2, float *y, int bt, int n, int clear) { hybridLong(x1, x2, y, bt, n, clear); }
void ref_hybridShort(float *x1, float *x2, float *y, int n) { hybridShort(x1, x2, y, n); }
void ref_antialias(float *x, int n) { antialias(x, n); }
int ref_attack(float *samp, int *eng, int prev) { return attack_detectSBT_igr(samp, eng, prev); }

}   /* extern "C" */
