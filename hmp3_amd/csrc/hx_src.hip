// hx_src.hip - k_src (K0a): the sample-format / sample-rate converter of converting batches, source format / rate -> fp32 PCM at the encode rate.
// The GPU form of hx_src.cpp (reference srcc.cpp / srccf.cpp): every case (copy, exact 1:2, linear up-sampling, one
// polyphase bank, two stages), layout (mono, stereo, stereo summed to mono) and source format (u8, s16, s24 packed, s32,
// f32), bit-identical to hx_src_convert: each expression has hx_src.cpp's operand types (double where that code promotes),
// taps are summed in its order from 0.0f, and nothing is contracted (-ffp-contract=off).
//
// One workgroup per (stream, call): a call is one reference call of 1152 output samples per channel.  Its input window is
// format-converted into LDS, then every lane owns output samples and runs its own tap chain.  The converter's phase is a
// closed form of the stream's call count (hx_src.h), so the calls of a launch are independent, except:
//  - case 4 reads intermediate samples formed by the previous call.  Call 0 of a launch takes them from the carry the
//    previous launch left (formed samples, not input: the previous call's pointer may have read bytes the next call's
//    input does not hold); call f > 0 forms them again from call f - 1's input, as that call did.
//  - the down-mix of case 2 is a recurrence within a call (a = a + b does not give the midpoint back in float): one lane.
// A stream's last call of a launch (per stream: SrcArgs::nfr) writes the carry and the call count to the other copy of each
// (the first call of the launch reads the copy from before, so a one-call launch never reads what it writes).  The copies
// change roles with every launch, for the whole batch: a stream without a call in the launch copies both across.
#include "hx_dev.h"
#include "hx_src.h"

// (SrcArgs: hx_src.h, shared with the launch in hx_batch_src.hip)

// sample `idx` (interleaved channels) of a source in the given format, at int16 scale (hx_src_convert's staging)
__device__ __forceinline__ float src_sample(const unsigned char *x, long long idx, int bits, int is_float, bool aligned)
{
    if (bits == 8) return (((float) x[idx]) - 128.0f) * (256.0f);
    if (bits == 24) {
        const unsigned char *b = x + 3 * idx;
        const int v = (int) (((unsigned) b[2] << 24) | ((unsigned) b[1] << 16) | ((unsigned) b[0] << 8)) >> 8;
        return (float) ((float) v / 256.0f);
    }
    if (bits == 16) {
        short v;
        if (aligned) v = ((const short *) x)[idx];
        else v = (short) ((unsigned) x[2 * idx] | ((unsigned) x[2 * idx + 1] << 8));
        return (float) v;
    }
    unsigned u;
    if (aligned) u = ((const unsigned *) x)[idx];
    else { const unsigned char *b = x + 4 * idx; u = (unsigned) b[0] | ((unsigned) b[1] << 8) | ((unsigned) b[2] << 16) | ((unsigned) b[3] << 24); }
    if (is_float) return (float) __uint_as_float(u) * 32768.0f;
    return (float) ((int) u / 65536.0f);
}

// byte offset of call f's input in the row of stream s
__device__ __forceinline__ long long src_call_offset(const SrcArgs &a, const HxSrcPlan *p, int s, int f, long long c0)
{
    if (a.off) return a.off[(long long) s * a.nframes + f];
    const long long used = hx_src_consumed(p, c0, c0 + f);
    return used * p->channels * (p->bits / 8);
}

// intermediate sample q (case 4, channel ch; layout 2: the down-mix) of a call whose first intermediate sample is qs,
// from that call's input x[]: x[j] + coef1[q mod n1] (x[j + 1] - x[j]) with j = J(q) - J(qs)   (hx_src.cpp refill_*)
template <class Load>
__device__ __forceinline__ float src_form(const HxSrcPlan *p, int j, float c1, int ch, Load x)
{
    if (p->layout == 2) {
        const float a = (x(2 * j) + x(2 * j + 1)) * 0.5, b = (x(2 * j + 2) + x(2 * j + 3)) * 0.5;
        return a + c1 * (b - a);
    }
    const int C = p->channels;
    const float x0 = x(C * j + ch), x1 = x(C * (j + 1) + ch);
    return (float) x0 + c1 * ((float) x1 - (float) x0);
}

__global__ __launch_bounds__(256) void k_src(SrcArgs a)
{
    extern __shared__ float src_lds[];
    const int s = blockIdx.x / a.nframes, f = blockIdx.x - s * a.nframes, tid = threadIdx.x;
    // per-stream counts: the stream makes the first nn calls of the launch.  A workgroup beyond them leaves as a whole,
    // before it reads the plan, an offset or a byte of the row (s, f and nn are uniform: no barrier is split).  A stream
    // that sits the launch out has no last call, so its first workgroup hands the call count and the carried samples
    // from the copy this launch reads to the copy the next one reads.
    const int nn = a.nfr ? a.nfr[s] : a.nframes;
    if (f >= nn) {
        if (nn == 0 && f == 0) {
            const float *cin = a.carry_in + (long long) s * 2 * HX_SRC_CARRY;
            float *cout = a.carry_out + (long long) s * 2 * HX_SRC_CARRY;
            for (int t = tid; t < 2 * HX_SRC_CARRY; t += 256) cout[t] = cin[t];
            if (tid == 0) a.calls_out[s] = a.calls_in[s];
        }
        return;
    }
    const HxSrcPlan *p = a.plan + a.cls[s];
    const int ncase = p->ncase, layout = p->layout, C = p->channels, bits = p->bits, is_float = p->is_float;
    const long long c0 = a.calls_in[s], c = c0 + f, i0 = 1152 * c;
    const unsigned char *row = a.in + (long long) s * a.in_stride;
    const unsigned char *xin = row + src_call_offset(a, p, s, f, c0);
    const bool aligned = ((unsigned long long) xin & (bits == 32 ? 3 : 1)) == 0;
    long long used, rd;
    hx_src_call_extent(p, c, &used, &rd);
    float *xs = src_lds;                        // the call's input, interleaved like the source
    float *zs = src_lds + a.zoff;               // case 4: intermediate samples [u(i0), qstart(c + 1)) per channel
    float *cl = src_lds + a.coff;               // cases 2 - 4: the filter bank (fractions)
    // (cannot happen: xwin bounds every call's window, hx_src_plan; a broken bound is reported in the status word)
    if (rd > a.xwin) { if (tid == 0) atomicOr(a.status, HX_SRC_STATUS_WINDOW); return; }
    const int nx = (int) rd * C;
    const int n = p->n, m = p->m, k = p->k, ntaps = p->ntaps;
    for (int t = tid; t < nx; t += 256) xs[t] = src_sample(xin, t, bits, is_float, aligned);
    if (ncase >= 2) for (int t = tid; t < p->totcoef; t += 256) cl[t] = p->coef[t];
    __syncthreads();
    // (the row is pitched for a.nch channels, the stream's calls sit contiguous at its start: p->nch <= a.nch)
    float *y = a.out + ((long long) s * a.nframes * a.nch + (long long) f * p->nch) * 1152;
    // phase of the call's first output: r0 = i0 m mod n, i0 mod n; output t of the call sits w(i0 + t) - w(i0) =
    // (r0 + t m) / n bank steps after it (32-bit from here: t m < 1152 n)
    const int r0 = (int) ((i0 * m) % n), ph0 = (int) (i0 % n);
    switch (ncase) {
    case 0:
        for (int t = tid; t < 1152; t += 256) {
            if (layout == 0) y[t] = xs[t];
            else if (layout == 1) { y[2 * t] = xs[2 * t]; y[2 * t + 1] = xs[2 * t + 1]; }
            else y[t] = (float) ((xs[2 * t] + xs[2 * t + 1]) * 0.5);
        }
        break;
    case 1:
        for (int t = tid; t < 576; t += 256) {
            if (layout == 0) {      // the reference takes this path through integers
                const int ia = xs[t], ib = xs[t + 1];
                y[2 * t] = (float) (ia);
                y[2 * t + 1] = (float) ((ia + ib) >> 1);
            } else if (layout == 1) {
                for (int ch = 0; ch < 2; ch++) {
                    y[4 * t + ch] = xs[2 * t + ch];
                    y[4 * t + 2 + ch] = (float) ((xs[2 * t + ch] + xs[2 * t + 2 + ch]) * 0.5);
                }
            } else {
                const float sa = xs[2 * t] + xs[2 * t + 1], sb = xs[2 * t + 2] + xs[2 * t + 3];
                y[2 * t] = (float) (sa * 0.5);
                y[2 * t + 1] = (float) ((sa + sb) * 0.25);
            }
        }
        break;
    case 2:
        if (layout == 2) {          // a recurrence: one lane walks the call
            if (tid == 0) {
                float va = (xs[0] + xs[1]) * 0.5;
                float vb = ((xs[2] + xs[3]) * 0.5) - va;
                int u = 0, ic = ph0, r = r0;        // r = (i m) mod n: the bank steps as hx_src's step() does
                for (int t = 0; t < 1152; t++) {
                    y[t] = (float) (va + cl[ic] * vb);
                    if (++ic >= n) ic = 0;
                    r += m;
                    if (r >= n) { r -= n; u++; va = va + vb; vb = ((xs[2 * u + 2] + xs[2 * u + 3]) * 0.5) - va; }
                }
            }
            break;
        }
        for (int t = tid; t < 1152; t += 256) {
            const int u = (r0 + t * m) / n, ic = (ph0 + t) % n;
            const float cf = cl[ic];
            for (int ch = 0; ch < C; ch++) {
                const float x0 = xs[C * u + ch], x1 = xs[C * (u + 1) + ch];
                y[C * t + ch] = (float) ((float) x0 + cf * ((float) x1 - (float) x0));
            }
        }
        break;
    case 3:
        for (int t = tid; t < 1152; t += 256) {
            const int u = k * t + (r0 + t * m) / n;
            const float *cf = cl + ((ph0 + t) % n) * ntaps;
            if (layout == 0) {
                float acc = 0.0f;
                for (int j = 0; j < ntaps; j++) acc += cf[j] * xs[u + j];
                y[t] = acc;
            } else if (layout == 1) {
                float acc = 0.0f, acc2 = 0.0f;
                for (int j = 0; j < ntaps; j++) { acc += cf[j] * xs[2 * (u + j)]; acc2 += cf[j] * xs[2 * (u + j) + 1]; }
                y[2 * t] = acc; y[2 * t + 1] = acc2;
            } else {
                float acc = 0.0f;
                for (int j = 0; j < ntaps; j++) acc += cf[j] * ((xs[2 * (u + j)] + xs[2 * (u + j) + 1]) * 0.5);
                y[t] = acc;
            }
        }
        break;
    default: {
        // intermediate samples: z0 = u(i0) is the first one the call reads, qs = qstart(c) the first one it forms
        const long long z0 = hx_src_u(p, i0), qs = hx_src_qstart(p, c), qe = hx_src_qstart(p, c + 1);
        const int nz = (int) (qe - z0), nc = layout == 1 ? 2 : 1;
        if (nz > a.zwin || nz < HX_SRC_CARRY || qs - z0 > HX_SRC_CARRY) {           // (cannot happen either)
            if (tid == 0) atomicOr(a.status, HX_SRC_STATUS_WINDOW);
            break;
        }
        // (sample qs + t reads input (rq + t m1) / n1 of the call and fraction (pq + t) mod n1: 32-bit from here)
        const int n1 = p->n1, m1 = p->m1, rq = (int) ((qs * m1) % n1), pq = (int) (qs % n1);
        for (int t = tid; t < (int) (qe - qs); t += 256) {
            const int j = (rq + t * m1) / n1;
            const float c1 = p->coef1[(pq + t) % n1];
            for (int ch = 0; ch < nc; ch++) zs[ch * a.zwin + (int) (qs - z0) + t] = src_form(p, j, c1, ch, [&](int i) { return xs[i]; });
        }
        // the carried ones [z0, qs): formed by the previous call
        const int ncar = (int) (qs - z0);
        if (f == 0) {
            const float *cin = a.carry_in + (long long) s * 2 * HX_SRC_CARRY;
            for (int t = tid; t < ncar; t += 256)
                for (int ch = 0; ch < nc; ch++) zs[ch * a.zwin + t] = cin[ch * HX_SRC_CARRY + HX_SRC_CARRY - ncar + t];
        } else {
            const unsigned char *xprev = row + src_call_offset(a, p, s, f - 1, c0);
            const bool al = ((unsigned long long) xprev & (bits == 32 ? 3 : 1)) == 0;
            const long long qp = hx_src_qstart(p, c - 1);
            const int rp = (int) ((qp * m1) % n1), pp = (int) (qp % n1), d = (int) (z0 - qp);
            for (int t = tid; t < ncar; t += 256) {
                const int j = (rp + (d + t) * m1) / n1;
                const float c1 = p->coef1[(pp + d + t) % n1];
                for (int ch = 0; ch < nc; ch++)
                    zs[ch * a.zwin + t] = src_form(p, j, c1, ch, [&](int i) { return src_sample(xprev, i, bits, is_float, al); });
            }
        }
        __syncthreads();
        for (int t = tid; t < 1152; t += 256) {
            const int u = k * t + (r0 + t * m) / n;
            const float *cf = cl + ((ph0 + t) % n) * ntaps;
            for (int ch = 0; ch < nc; ch++) {
                const float *z = zs + ch * a.zwin + u;
                float acc = 0.0f;
                for (int j = 0; j < ntaps; j++) acc += cf[j] * z[j];
                y[nc * t + ch] = acc;
            }
        }
        if (f == nn - 1) {
            float *cout = a.carry_out + (long long) s * 2 * HX_SRC_CARRY;
            for (int t = tid; t < HX_SRC_CARRY; t += 256)
                for (int ch = 0; ch < nc; ch++) cout[ch * HX_SRC_CARRY + t] = zs[ch * a.zwin + nz - HX_SRC_CARRY + t];
        }
        break;
    }
    }
    if (f == nn - 1 && tid == 0) a.calls_out[s] = c0 + nn;
}
