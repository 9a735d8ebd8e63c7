// hx_recon.hip - decoded PCM (hx_batch_recon_buffer): what an ISO 11172-3 decoder outputs for the frames a call coded,
// computed from the stream walk's hand-over instead of from the bytes.  Built as part of hx_pack.hip's unit.
//
// Three kernels behind a call's packing, on its stream:
//   k_recon_hybrid  (stream, granule): requantisation, M/S, alias reduction, IMDCT with the block-type windows, overlap-add
//                   and frequency inversion, for both channels -> hybrid output [S][NG][2][18 time slots][32 subbands]
//   k_recon_synth   (stream, frame): polyphase synthesis -> the caller's row, in the layout of the f32 PCM rows
//   k_recon_carry   (stream): the call's last IMDCT tails and last 15 time slots into the stream's carried state
// Inputs, all written by the stream walk: the quantised lines (bitstream order; defined up to 2 big_values + 4 quads), one
// sign bit per line, the segment record (short blocks' scalefactor fields) and the frame record (side information, long
// blocks' scalefactors with scfsi resolved, ms).  MPEG-1 streams of the second-generation allocator only (kind 0).
//
// Every granule is independent: workgroup (s, g) forms granule g's IMDCT and, for the overlap, the second half of granule
// g - 1's again (g = 0: the carried tails); the synthesis of a frame matrixes its own 36 slots and the 15 before them again
// (the call's first frame: the carried ones).  One operation order per output value, whichever workgroup forms it and however the frames are
// split over calls, and the state is carried as the floats themselves: the output is bit-identical under any split.
// The carried state is read by the workgroups of a stream's first granule and written by none of the first two kernels -
// the new tails go through a scratch row - so no workgroup's read races another's write; k_recon_carry runs behind both.
//
// LDS (k_recon_hybrid): a channel's 576 lines as [32 subbands][19], 18 used: lanes that differ in the subband read at a
// stride of 19 dwords, which no two lanes of a 32-lane half share a bank for; a wave works on one time slot, so the
// transform's row and the window tap are wave-uniform.  k_recon_synth: a thread holds its column of the matrixing table
// ([k][i]: lanes i = 0 .. 63 load consecutive dwords) and 26 slots' sums in registers, and the subband samples are an
// LDS broadcast of four at a time; the matrixed vectors are read at consecutive dwords by lanes that differ in the
// output sample, whose window taps sit in registers.
#include "hx_dev.h"

#define HX_RC_PITCH 19                  // dwords per subband of a channel's lines in LDS
#define HX_RC_LINES (32 * HX_RC_PITCH)

struct ReconLds {
    float x[2][2][HX_RC_LINES];         // [granule g - 1, granule g][channel]
    int lstart[24], sstart[16];         // first line of every long / short scalefactor band (ISO)
    int esf[2][2][40];                  // [granule][channel] quarter steps each band's scalefactor takes off the exponent
};

__device__ __forceinline__ int rc_pretab(int b) { return b < 11 ? 0 : b < 15 ? 1 : b < 17 ? 2 : b < 20 ? 3 : b < 21 ? 2 : 0; }
__device__ __forceinline__ int rc_at(int line) { return (line / 18) * HX_RC_PITCH + line % 18; }

// One granule's lines of both channels requantised into L.x[slot], M/S turned to L/R, alias reduction on long blocks.
// Returns the block type.  The whole workgroup, ahead of its barriers.
__device__ __forceinline__ int recon_lines(ReconLds &L, int slot, const HxGlobalTabs *gt, const HxReconTabs *rt, const short *ixq, const unsigned *sgn,
                           const HxSegOut *seg, const HxFrameDebug *rec, long long unit0, int igr, int nchan)
{
    const int tid = threadIdx.x;
    const int bt = rec->gr[igr][0].block_type & 3;
    // per band: (scalefac_scale ? 4 : 2) * (scalefactor + preflag * pretab), in quarter steps of the exponent
    for (int i = tid; i < 2 * 40; i += 256) {
        const int ch = i / 40, b = i - 40 * ch;
        int v = 0;
        if (ch < nchan) {
            const HxGr &q = rec->gr[igr][ch];
            const int mul = q.scalefac_scale ? 4 : 2;
            if (bt == 2) v = (b < 36) ? mul * (seg[unit0 + ch].sf[b] & 255) : 0;        // field 3 * band + window
            else v = (b < 21) ? mul * (rec->sf[igr][ch][b] + (q.preflag ? rc_pretab(b) : 0)) : 0;
        }
        L.esf[slot][ch][b] = v;
    }
    __syncthreads();
    for (int i = tid; i < 2 * 576; i += 256) {
        const int ch = i / 576, j = i - 576 * ch;       // line j of the bitstream's order
        if (ch >= nchan) break;
        const HxGr &q = rec->gr[igr][ch];
        const int ncoded = q.aux_not_null ? min(576, 2 * q.big_values + 4 * max(q.aux_nquads, 0)) : 0;
        int e4 = q.global_gain - 210, at;
        if (bt == 2) {
            int b = 0;
            while (b < 12 && j >= 3 * L.sstart[b + 1]) b++;
            const int wd = L.sstart[b + 1] - L.sstart[b], r = j - 3 * L.sstart[b], w = r / wd, l = L.sstart[b] + (r - w * wd);
            e4 -= 8 * q.subblock_gain[w] + L.esf[slot][ch][min(3 * b + w, 39)] * (b < 12);
            at = (l / 6) * HX_RC_PITCH + 6 * w + l % 6;     // subband, window, line of the window's six
        } else {
            int b = 0;
            while (b < 21 && j >= L.lstart[b + 1]) b++;
            e4 -= L.esf[slot][ch][b];
            at = rc_at(j);
        }
        float v = 0.0f;
        if (j < ncoded) {
            const int mag = (int) (unsigned short) ixq[(unit0 + ch) * 576 + j];
            const double d = ldexp(gt->pow43[min(mag, HX_POW43_N - 1)] * rt->pow2q[e4 & 3], e4 >> 2);
            v = (float) d;
            if ((sgn[(unit0 + ch) * HX_SGN_WORDS + (j >> 5)] >> (j & 31)) & 1u) v = -v;
        }
        L.x[slot][ch][at] = v;
    }
    __syncthreads();
    if (rec->ms && nchan == 2) {
        const float r2 = 0.70710678118654752440f;
        for (int i = tid; i < HX_RC_LINES; i += 256) {
            const float m = L.x[slot][0][i], s = L.x[slot][1][i];
            L.x[slot][0][i] = (m + s) * r2;
            L.x[slot][1][i] = (m - s) * r2;
        }
        __syncthreads();
    }
    if (bt != 2) {
        for (int i = tid; i < 2 * 31 * 8; i += 256) {
            const int ch = i / 248, r = i - 248 * ch, sb = 1 + (r >> 3), k = r & 7;
            if (ch >= nchan) break;
            float *x = L.x[slot][ch];
            const int lo = rc_at(18 * sb - 1 - k), hi = rc_at(18 * sb + k);
            const float a = x[lo], b = x[hi], cs = rt->cs[k], ca = rt->ca[k];
            x[lo] = a * cs - b * ca;
            x[hi] = b * cs + a * ca;
        }
        __syncthreads();
    }
    return bt;
}

// Output i (0 .. 35) of the windowed IMDCT of subband sb: 36 points, or three 12-point transforms laid at 6, 12 and 18
__device__ __forceinline__ float recon_imdct(const float *x, const HxReconTabs *rt, int bt, int sb, int i)
{
    const float *xs = x + sb * HX_RC_PITCH;
    if (bt != 2) {
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 18; k++) sum += xs[k] * rt->cos36[i][k];
        return sum * rt->win[bt][i];
    }
    float acc = 0.0f;
#pragma unroll
    for (int w = 0; w < 3; w++) {
        const int j = i - 6 - 6 * w;
        if (j < 0 || j >= 12) continue;
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; k++) sum += xs[6 * w + k] * rt->cos12[j][k];
        acc += sum * rt->win[2][j];
    }
    return acc;
}

// hyb [S][NG][2][18][32]; tails [S][2][32][18]: the IMDCT tails of each stream's last granule of the call; state [S][HX_RECON_STATE_FLOATS];
// rec [S][NG / 2] the call's frame records
__global__ __launch_bounds__(256) void k_recon_hybrid(const HxStream *__restrict__ st, const HxParams *__restrict__ prm, const HxGlobalTabs *__restrict__ gt,
                                                      const HxReconTabs *__restrict__ rt, const short *__restrict__ ixq, const unsigned *__restrict__ sgn,
                                                      const HxSegOut *__restrict__ seg, const HxFrameDebug *__restrict__ rec, float *__restrict__ hyb,
                                                      float *__restrict__ tails, const float *__restrict__ state, int NG, const int *__restrict__ nfr)
{
    __shared__ ReconLds L;
    const int tid = threadIdx.x;
    const int s = blockIdx.x / NG, g = blockIdx.x - s * NG;
    const int NGs = 2 * (nfr ? nfr[s] : NG / 2);
    if (g >= NGs) return;
    const HxParams *p = prm + st[s].cls;
    const int nchan = p->nchan;
    if (tid == 0) {
        int k = 0;
        for (int b = 0; b < 22; b++) { L.lstart[b] = k; k += p->nBand_l_iso[b]; }
        L.lstart[22] = L.lstart[23] = 576;
        k = 0;
        for (int b = 0; b < 13; b++) { L.sstart[b] = k; k += p->nBand_s[b]; }
        L.sstart[13] = L.sstart[14] = L.sstart[15] = 192;
    }
    __syncthreads();
    const HxFrameDebug *rs = rec + (long long) s * (NG / 2);
    int bt_prev = 0;
    if (g > 0) bt_prev = recon_lines(L, 0, gt, rt, ixq, sgn, seg, rs + ((g - 1) >> 1), ((long long) s * NG + g - 1) * 2, (g - 1) & 1, nchan);
    const int bt = recon_lines(L, 1, gt, rt, ixq, sgn, seg, rs + (g >> 1), ((long long) s * NG + g) * 2, g & 1, nchan);
    const float *carried = state + (long long) s * HX_RECON_STATE_FLOATS;
    // a wave takes one time slot i at a time - its transform rows and window taps are the same for all lanes, which differ in
    // the channel (the wave's halves) and the subband
    const int lane = tid & 63, ch = lane >> 5, sb = lane & 31;
    for (int i = __builtin_amdgcn_readfirstlane(tid >> 6); i < 18; i += 4) {
        if (ch >= nchan) continue;
        const int r = i * 32 + sb;
        const float cur = recon_imdct(L.x[1][ch], rt, bt, sb, i);
        const float tail = g > 0 ? recon_imdct(L.x[0][ch], rt, bt_prev, sb, 18 + i) : carried[ch * 576 + sb * 18 + i];
        float v = cur + tail;
        if ((sb & 1) && (i & 1)) v = -v;
        hyb[(((long long) s * NG + g) * 2 + ch) * 576 + r] = v;
        if (g == NGs - 1) tails[((long long) s * 2 + ch) * 576 + sb * 18 + i] = recon_imdct(L.x[1][ch], rt, bt, sb, 18 + i);
    }
}

struct __attribute__((packed, aligned(4))) ReconPair { float l, r; };      // (a recon row is 4-byte aligned and no more)

// out [S][row]: row floats per stream; a stereo stream's samples interleaved, a mono stream's at the start of its row.
// One workgroup per (stream, frame): its 36 time slots and the 15 before them.
__global__ __launch_bounds__(256) void k_recon_synth(const HxStream *__restrict__ st, const HxParams *__restrict__ prm, const HxReconTabs *__restrict__ rt,
                                                     const float *__restrict__ hyb, const float *__restrict__ state, float *__restrict__ out,
                                                     long long row, int NG, const int *__restrict__ nfr)
{
    constexpr int H = HX_RECON_HIST_SLOTS, NS = 36 + H, NJ = (NS + 1) / 2;
    __shared__ __align__(16) float sb_[2][NS][32];
    __shared__ float v_[2][NS][64];
    const int tid = threadIdx.x;
    const int F = NG / 2, s = blockIdx.x / F, f = blockIdx.x - s * F;
    if (f >= (nfr ? nfr[s] : F)) return;
    const int nchan = prm[st[s].cls].nchan;
    // time slots f * 36 - 15 .. f * 36 + 35 of the call: from the hybrid output, the ones before the call from the carried state
    const float *hist = state + (long long) s * HX_RECON_STATE_FLOATS + HX_RECON_TAIL_FLOATS;
    for (int i = tid; i < nchan * NS * 32; i += 256) {
        const int ch = i / (NS * 32), r = i - ch * NS * 32, j = r >> 5, k = r & 31, T = f * 36 + j - H;
        sb_[ch][j][k] = T >= 0 ? hyb[(((long long) s * NG + T / 18) * 2 + ch) * 576 + (T % 18) * 32 + k] : hist[(ch * H + H + T) * 32 + k];
    }
    __syncthreads();
    {   // matrixing: a thread takes one column (channel, n) of the table, held in registers, over half of the slots; a slot's
        // subband samples come four at a time, the same for every lane of the wave; each sum runs over k in ascending order
        const int col = tid & 127, ch = col >> 6, n = col & 63;
        const int half = __builtin_amdgcn_readfirstlane(tid >> 7), j0 = half ? NJ : 0, nj = half ? NS - NJ : NJ;
        if (ch < nchan) {
            float m[32], acc[NJ];
#pragma unroll
            for (int k = 0; k < 32; k++) m[k] = rt->synth[k][n];
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) acc[jj] = 0.0f;
#pragma unroll
            for (int k = 0; k < 32; k += 4) {
#pragma unroll
                for (int jj = 0; jj < NJ; jj++) {
                    if (jj >= nj) continue;
                    const float4 q = *reinterpret_cast<const float4 *>(&sb_[ch][j0 + jj][k]);
                    acc[jj] += m[k] * q.x;
                    acc[jj] += m[k + 1] * q.y;
                    acc[jj] += m[k + 2] * q.z;
                    acc[jj] += m[k + 3] * q.w;
                }
            }
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) if (jj < nj) v_[ch][j0 + jj][n] = acc[jj];
        }
    }
    __syncthreads();
    float *o = out + (long long) s * row;
    const int j = tid & 31;
    float dw0[8], dw1[8];       // the window taps of this thread's sample position j, the same in all its time slots
#pragma unroll
    for (int k = 0; k < 8; k++) { dw0[k] = rt->dwin[64 * k + j]; dw1[k] = rt->dwin[64 * k + 32 + j]; }
    for (int t = tid >> 5; t < 36; t += 8) {
        float acc[2] = {0.0f, 0.0f};
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            if (ch >= nchan) continue;
#pragma unroll
            for (int k = 0; k < 8; k++)
                acc[ch] += dw0[k] * v_[ch][H + t - 2 * k][j] + dw1[k] * v_[ch][H + t - 2 * k - 1][32 + j];
        }
        const long long n = (long long) f * 1152 + t * 32 + j;
        if (nchan == 2) { ReconPair pr = {acc[0], acc[1]}; *reinterpret_cast<ReconPair *>(o + 2 * n) = pr; }
        else o[n] = acc[0];
    }
}

__global__ __launch_bounds__(256) void k_recon_carry(const HxStream *__restrict__ st, const HxParams *__restrict__ prm, const float *__restrict__ hyb,
                                                     const float *__restrict__ tails, float *__restrict__ state, int NG, const int *__restrict__ nfr)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const int NGs = 2 * (nfr ? nfr[s] : NG / 2);
    if (NGs <= 0) return;
    const int nchan = prm[st[s].cls].nchan;
    float *dst = state + (long long) s * HX_RECON_STATE_FLOATS;
    for (int i = tid; i < nchan * 576; i += 256) dst[i] = tails[(long long) s * HX_RECON_TAIL_FLOATS + i];
    for (int i = tid; i < nchan * HX_RECON_HIST_SLOTS * 32; i += 256) {
        const int ch = i / (HX_RECON_HIST_SLOTS * 32), r = i - ch * HX_RECON_HIST_SLOTS * 32, T = NGs * 18 - HX_RECON_HIST_SLOTS + (r >> 5);
        dst[HX_RECON_TAIL_FLOATS + i] = hyb[(((long long) s * NG + T / 18) * 2 + ch) * 576 + (T % 18) * 32 + (r & 31)];
    }
}
