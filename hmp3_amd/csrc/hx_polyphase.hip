// hx_polyphase.hip - the front end up to the subband samples and block types (batched MP3 encoder for MI355X, gfx950):
//   k_dcfilter   K0  optional input DC blocker, sequential per channel   (filter2.c:116-144)
//   k_polyphase  K1  int16 / fp32 PCM -> 32 x 18 subband samples per granule (the stage of sbt.c:57-310), and in its
//                    epilogue the subband energies in mB for the transient detector (detect.c:80-101)
//                    (its first tile of a stream also forms the energies of the carried granule: the call's first detector index)
//   k_detect     K2  attack metric for both "previous granule short" cases (detect.c:103-141) and the per-stream block-type
//                    state machine (mp3enc.cpp:1398-1440), one wavefront per stream
//   k_gate           the batch runtime's gate of a pipelined submit: no part of the front end, here for this unit's flags, under
//                    which its code is what it has been (hx_batch.hip launches it)
// Parallel over streams x channels x granules (x slots / subbands).  Each lane
// evaluates its unit with the reference's operation order, so results are bit-identical.
// Built without LLVM's iterative-ilp scheduling strategy, which hurts the polyphase loop (1.17 -> 1.38 ms): hx_units.tab.
#include "hx_dev.h"

// (K1_GPB granules per workgroup, K1_THREADS lanes: hx_types.h, shared with the launch in hx_batch.hip)

#define K1_NS (480 + 576 * K1_GPB)      // staged samples
#define K1_LDS (K1_NS + (K1_NS >> 5) + 1)

// N-point DCT of the analysis filterbank by odd / even decimation:
//   X[j], X[N-1-j] = E[j] +- tw_N[j] * O[j]   with   E = DCT_{N/2}(x[0], x[2], ...),  O = DCT_{N/2}(u),
//   u[i] = x[2i+1] - u[i+1],  u[N/2-1] = x[N-1]   (running difference of the odd samples from the top)
// tw_N[j] = 2 cos(pi (2j+1) / 2N) sits at tw[N/2 + j].  Everything stays in registers: the recursion is
// resolved at compile time into straight-line code, depth first.  Each sum is one rounding, in the order
// written here, which is also the reference's (sbt.c:134-259), so the subband samples agree bit for bit.
template <int N> struct AnalysisDct {
    template <class T>
    static __device__ __forceinline__ void run(const T *x, T *X, const float *tw)
    {
        constexpr int H = N / 2;
        T even[H], u[H], E[H], O[H];
        u[H - 1] = x[N - 1];
        even[H - 1] = x[N - 2];
#pragma unroll
        for (int i = H - 2; i >= 0; i--) { u[i] = x[2 * i + 1] - u[i + 1]; even[i] = x[2 * i]; }
        AnalysisDct<H>::run(even, E, tw);
        AnalysisDct<H>::run(u, O, tw);
#pragma unroll
        for (int j = 0; j < H; j++) {
            const T r = tw[H + j] * O[j];
            X[j] = E[j] + r;
            X[N - 1 - j] = E[j] - r;
        }
    }
};
template <> struct AnalysisDct<1> {
    template <class T>
    static __device__ __forceinline__ void run(const T *x, T *X, const float *) { X[0] = x[0]; }
};

// One lane = one time slot of BOTH channels: every value is a (left, right) pair and the arithmetic is packed fp32
// (v_pk_mul_f32 / v_pk_add_f32: two IEEE operations per lane and instruction, each rounded like the plain one), so the
// window taps, the LDS reads and the instruction stream are shared by the two channels.  A workgroup of four waves
// stages the interleaved stereo PCM of K1_GPB granules (plus 480 samples of history) as float pairs; a sample pair is
// one ds_read_b64 (2 LDS cycles per wave; stride 33 pairs between lanes = 66 words: conflict-free), the taps come
// through the scalar cache.  Round 3: 1.165 -> 0.865 ms per 1024 x 256 frames against one channel per lane with
// ds_read2_b32 samples and taps by LDS broadcast; the kernel now moves 3.6 GB in that time and is bound by HBM.
typedef float v2f __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(K1_THREADS) void k_polyphase(const int16_t *__restrict__ pcm, long long nsamp,
                                                   const HxStream *__restrict__ st,
                                                   const HxParams *__restrict__ prm,
                                                   const HxGlobalTabs *__restrict__ gt,
                                                   float *__restrict__ sb, int NG, int SG,
                                                   const float *__restrict__ pcmf, int pitch, int *__restrict__ eng,
                                                   const int *__restrict__ nfr)
{
    // pitch: the channels every PCM row is laid out for (hx_batch_pcm_channels); nchan below: the stream's own, which in a
    // mixed batch may be 1 under a pitch of 2 - its samples then sit contiguous at the start of its row
    __shared__ __attribute__((aligned(16))) v2f xs[K1_LDS];
    const int s = blockIdx.x, lt = threadIdx.x;
    const int g0 = blockIdx.y * K1_GPB;
    // the stream's granules of this call (hx_batch_frame_counts): the bound; NG stays the stride of eng.  A tile may be cut by
    // the count or lie beyond it: the workgroup is one stream's, so it leaves as one, ahead of its barrier
    const int NGs = nfr ? 2 * nfr[s] : NG;
    const int ng = min(K1_GPB, NGs - g0);
    if (ng <= 0) return;
    const int count = 480 + 576 * ng;
    const HxStream *ss = st + s;
    const HxParams *p = prm + __builtin_amdgcn_readfirstlane(ss->cls);
    const int nchan = p->nchan;                                 // (a scalar load: cls is wave-uniform)
    const int lsf = !p->h_id;                                   // the stream's own version (the same: the workgroup is one stream's)
    const int16_t *src = pcm + (long long) s * nsamp * pitch;   // interleaved L R (or one channel)
    if (blockIdx.y == 0 && lt < 18) {
        // The detector energies of eng index 0 (this kernel's epilogue writes the others): from the carried last granule of the
        // previous call, subband slot 2, which no workgroup of this launch writes.  (A kernel of its own until round 6: eighteen
        // lanes per stream, one launch less per call.)
        const int ch = lt / 9, k = lt - 9 * ch;
        const int sb0 = lsf ? 8 : 4, nsbb = lsf ? 20 : 14;
        const float *y = sb + ((long long) (s * 2 + ch) * SG + 2) * 576 + 18 * sb0 + 2 * k;
        float sum = 7.0e4f;
        for (int i = 0; i < nsbb; i++, y += 18) {
            float x = y[0] * y[0]; sum += x;
            x = y[1] * y[1]; sum += x;
        }
        eng[(long long) (s * 2 + ch) * NG * 9 + k] = hx_mblog(gt->mblog, sum);
    }
    const long long n0 = 576LL * g0 - 480;                      // sample index of staged slot 0
    const int hist = (g0 == 0) ? 480 : 0;                       // slots that come from the carry
    if (nchan == 1) {       // mono stream: the right half of every pair is silence
        const float *srcf = pcmf + (long long) s * nsamp * pitch;
        for (int idx = hist + lt; idx < count; idx += K1_THREADS)
            xs[idx + (idx >> 5)] = v2f{pcmf ? srcf[n0 + idx] : (float) src[n0 + idx], 0.0f};
    } else if (pcmf) {      // DC-blocked input from k_dcfilter: fp32, interleaved like the PCM
        const v2f *srcf = reinterpret_cast<const v2f *>(pcmf) + (long long) s * nsamp;       // (a stereo stream: pitch = 2)
        for (int idx = hist + lt; idx < count; idx += K1_THREADS) xs[idx + (idx >> 5)] = srcf[n0 + idx];
    } else if ((reinterpret_cast<unsigned long long>(pcm) & 15ull) == 0) {
        const int nv = count >> 2, vh = hist >> 2;              // 4 stereo samples per 16 bytes
        constexpr int NR = ((480 + 576 * K1_GPB) / 4 + K1_THREADS - 1) / K1_THREADS;
        int4 w[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int v = lt + K1_THREADS * r;
            const int vc = min(max(v, vh), nv - 1);
            w[r] = *reinterpret_cast<const int4 *>(src + 2 * (n0 + 4LL * vc));
        }
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int v = lt + K1_THREADS * r;
            if (v >= vh && v < nv) {
                const int q[4] = {w[r].x, w[r].y, w[r].z, w[r].w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int idx = 4 * v + e;
                    xs[idx + (idx >> 5)] = v2f{(float) (short) (q[e] & 0xFFFF), (float) (short) (q[e] >> 16)};
                }
            }
        }
    } else {
        for (int idx = hist + lt; idx < count; idx += K1_THREADS) {
            const long long n = n0 + idx;
            xs[idx + (idx >> 5)] = v2f{(float) src[2 * n], (float) src[2 * n + 1]};
        }
    }
    for (int i = lt; i < hist; i += K1_THREADS) xs[i + (i >> 5)] = v2f{ss->pcm_hist[0][i], nchan == 2 ? ss->pcm_hist[1][i] : 0.0f};
    __syncthreads();
    const int gl = lt / 18, t = lt - gl * 18;
    if (gl >= ng) return;
    const int base = 480 + 576 * gl + 32 * t + 31;          // newest sample of the slot
    // (volatile: single ds_read_b64, 2 LDS cycles each; merged into ds_read2_b64 a pair would take 8)
    typedef const volatile v2f __attribute__((address_space(3))) *LdsPairPtr;
    LdsPairPtr P = (LdsPairPtr) (xs + (base + (base >> 5) - 526));      // P[526 - pad(off)] = sample of age off
#define XS(off) P[526 - ((off) + ((off) >> 5))]
    // Two-stage pipeline over the 32 folded window lines, pinned with scheduling barriers: the 16 sample pairs of line
    // k + 1 are in flight while line k is summed.
    v2f b[32], X[32];
    v2f xa[2][8], xb[2][8];
    // The taps are the same for every lane: scalar loads into SGPRs, two lines ahead (a scalar load returns out of order,
    // so waiting for one means lgkmcnt(0): that wait stands at the top of a step, where the step's sample pairs are due
    // anyway, and the next line's reads are issued behind it).
    const float *wg = gt->anwin_r;
    float w[3][16];
#define K1_WLOAD(k) { _Pragma("unroll") for (int i = 0; i < 16; i++) w[(k) % 3][i] = wg[16 * (k) + i]; }
#define K1_TAP(k, i) w[(k) % 3][i]
#define K1_LOAD(k) { \
        const int A_ = ((k) == 0) ? 16 : ((k) <= 16) ? 16 + (k) : 80 - (k); \
        const int B_ = ((k) <= 16) ? 16 - (k) : 16 + (k); \
        _Pragma("unroll") for (int j = 0; j < 4; j++) { \
            xa[(k) & 1][2 * j] = XS(A_ + 128 * j); \
            xa[(k) & 1][2 * j + 1] = XS(A_ + 128 * j + 64); \
            if ((k) != 0) { xb[(k) & 1][2 * j] = XS(B_ + 128 * j); xb[(k) & 1][2 * j + 1] = XS(B_ + 128 * j + 64); } \
        } }
    K1_LOAD(0)
    K1_WLOAD(0)
    K1_WLOAD(1)
#pragma unroll
    for (int k = 0; k < 32; k++) {
        __builtin_amdgcn_s_waitcnt(0xC07F);         // lgkmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
        if (k + 2 < 32) K1_WLOAD(k + 2)
        if (k + 1 < 32) K1_LOAD(k + 1)
        __builtin_amdgcn_sched_barrier(0);
        v2f s1 = {0.0f, 0.0f}, s2 = {0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // (tap * pair: the packed multiply's operand selectors splat the SGPR over both channels)
            const float c0x = K1_TAP(k, 4 * j), c0y = K1_TAP(k, 4 * j + 1), c1x = K1_TAP(k, 4 * j + 2), c1y = K1_TAP(k, 4 * j + 3);
            s1 += c0x * xa[k & 1][2 * j];
            if (k) s2 += c0y * xb[k & 1][2 * j];
            s1 += c1x * xa[k & 1][2 * j + 1];
            if (k) s2 += c1y * xb[k & 1][2 * j + 1];
        }
        b[k] = k ? s1 + s2 : s1;
        __builtin_amdgcn_sched_barrier(0);
    }
#undef K1_LOAD
#undef K1_WLOAD
#undef K1_TAP
#undef XS
    AnalysisDct<32>::run(b, X, p->dct_tw);
    float *out = sb + ((long long) (s * 2) * SG + (g0 + gl + 3)) * 576 + t;
#pragma unroll
    for (int k = 0; k < 32; k++) out[18 * k] = X[k].x;
    if (nchan == 2) {
        float *out1 = out + (long long) SG * 576;
#pragma unroll
        for (int k = 0; k < 32; k++) out1[18 * k] = X[k].y;
    } else if (pitch == 2) {
        // A mono stream of a mixed batch: its slot may have run a stereo stream before (hx_batch_assign_streams), whose
        // channel-1 rows k_spec and k_msscan's carry would read again.  Zeros, as a mono batch's rows hold from create on.
        float *out1 = out + (long long) SG * 576;
#pragma unroll
        for (int k = 0; k < 32; k++) out1[18 * k] = 0.0f;
    }
    {   // transient detector input (reference detect.c:147-196): energy of subbands 4..17 (MPEG-2 LSF rates: 8..27) per pair
        // of time slots, as mB: slots 2 k (this lane) and 2 k + 1 (the next lane), subband after subband, in the reference's
        // order of additions.  eng index g <-> the granule one before coded granule g, so this granule's go to index + 1
        // (the last granule's are next call's index 0, formed from the carry at the top of this kernel).  A mono batch's silent
        // second channel sums to the floor by itself.
        v2f sum = {7.0e4f, 7.0e4f};
#define ENG_TERM(i) { const v2f y1 = {__shfl_down(X[i].x, 1, 64), __shfl_down(X[i].y, 1, 64)}; v2f x = X[i] * X[i]; sum += x; x = y1 * y1; sum += x; }
        if (!lsf) {
#pragma unroll
            for (int i = 4; i < 18; i++) ENG_TERM(i)
        } else {
#pragma unroll
            for (int i = 8; i < 28; i++) ENG_TERM(i)
        }
#undef ENG_TERM
        if (!(t & 1) && g0 + gl + 1 < NGs) {
            int *eo = eng + ((long long) (s * 2) * NG + g0 + gl + 1) * 9 + (t >> 1);
            eo[0] = hx_mblog(gt->mblog, sum.x);
            eo[(long long) NG * 9] = hx_mblog(gt->mblog, sum.y);
        }
    }
}

// attack metric of one channel at coded step g, for short_flag_prev = 0 and 1
// (the MPEG-2 detector looks back four values instead of six, detect.c:205-226)
__device__ __forceinline__ void attack_metric(const int *hist, const int *eng, int g, int *m0, int *m1, int lsf)
{
    // virtual buffer A: 32 history values followed by 9 new values per step
    int w[32];
#pragma unroll
    for (int j = 10; j < 29; j++) {
        int a = 9 * (g + 1) + j;
        w[j] = (a < 32) ? hist[a] : eng[a - 32];
    }
    int r0 = 0, r1 = 0;
#pragma unroll
    for (int j = 17; j < 29; j++) {
        int a0 = lsf ? -0x7fffffff : max(w[j - 6], w[j - 7]);
        int a1 = max(w[j - 4], w[j - 5]);
        int a2 = max(w[j - 2], w[j - 3]);
        a1 = max(a1, a0);
        int a = max(a1, a2);
        int d = w[j] - a;
        r0 = max(r0, d);
        if (j >= 18) r1 = max(r1, d);
    }
    *m0 = r0;
    *m1 = r1;
}

// Transient flags and block types of a stream, one wavefront per stream (round 6: two kernels before - a flag per (stream,
// granule) lane, then one lane per stream walking them): 64 granules at a time the lanes form their granule's two flags (for
// short_flag_prev = 0 and 1), lane 0 walks the state machine over them - block_type[g] = table[prev type][short now][short
// next] - and the lanes store the 64 types.
__global__ __launch_bounds__(256) void k_detect(HxStream *__restrict__ st, const HxParams *__restrict__ prm,
                                                const int *__restrict__ eng, unsigned char *__restrict__ flg,
                                                int *__restrict__ dbg_metric, unsigned char *__restrict__ bt,
                                                unsigned char *__restrict__ btprev, int NG, int S, const int *__restrict__ nfr)
{
    __shared__ unsigned char sflg[4][64], sbt[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wv;
    if (s >= S) return;         // (wave-uniform; nothing below is a workgroup barrier)
    // the stream's granules of this call: the bound of everything below (NG: the stride of eng, flg, bt).  A stream that takes
    // no frame keeps its detector history and block-type state as they are.
    const int NGs = nfr ? __builtin_amdgcn_readfirstlane(2 * nfr[s]) : NG;
    if (NGs == 0) return;
    HxStream *ss = st + s;
    // (the stream's class through a scalar register: the wave is one stream's, its neighbours in the workgroup may be of
    // another MPEG version, and nothing below is a workgroup barrier)
    const HxParams *p = prm + __builtin_amdgcn_readfirstlane(ss->cls);
    const int thr = p->short_block_threshold, lsf = !p->h_id;
    // sel[prev type * 4 + short now * 2 + short next] = {0, 1, 2, 2, 3, 2, 2, 2, 3, 2, 2, 2, 0, 1, 2, 2} as nibbles of a constant
    const unsigned long long sel = 0x2210222322232210ull;
    int prev_next = ss->short_flag_next_prev, prev_bt = ss->bt_prev;
    if (lane == 0) btprev[s] = (unsigned char) prev_bt;
    const int *e0 = eng + (long long) (s * 2 + 0) * NG * 9, *e1 = eng + (long long) (s * 2 + 1) * NG * 9;
    // (the hand-overs through sflg / sbt wait for the LDS writes themselves: a different primitive from HX_WAVE_SYNC)
#define DETECT_SYNC() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)
    for (int gb = 0; gb < NGs; gb += 64) {
        const int g = gb + lane;
        if (g < NGs) {
            int a0, a1, b0, b1;
            attack_metric(ss->attack_hist[0], e0, g, &a0, &a1, lsf);
            attack_metric(ss->attack_hist[1], e1, g, &b0, &b1, lsf);
            const int f0 = (a0 > thr) | (b0 > thr), f1 = (a1 > thr) | (b1 > thr);
            const unsigned char f = (unsigned char) (f0 | (f1 << 1));
            sflg[wv][lane] = f;
            flg[(long long) s * NG + g] = f;
            // (tests only: the metric of both channels for short_flag_prev = 0 and 1 - a0, b0, a1, b1)
            if (dbg_metric) *reinterpret_cast<int4 *>(dbg_metric + ((long long) s * NG + g) * 4) = make_int4(a0, b0, a1, b1);
        }
        DETECT_SYNC();
        if (lane == 0) {
            const int n = min(64, NGs - gb);
            for (int k = 0; k < n; k++) {
                const int f = sflg[wv][k];
                const int next = prev_next ? (f >> 1) & 1 : f & 1;
                const int b = (int) ((sel >> (4 * (prev_bt * 4 + prev_next * 2 + next))) & 15);
                prev_bt = b;
                prev_next = next;
                sbt[wv][k] = (unsigned char) b;
            }
        }
        DETECT_SYNC();
        if (g < NGs) bt[(long long) s * NG + g] = sbt[wv][lane];
        __builtin_amdgcn_wave_barrier();
    }
#undef DETECT_SYNC
    // roll the energy history: last 32 values of [hist | eng] (every lane has read the history above)
    int keep = 0;
    const int c = lane >> 5, j = lane & 31;
    {
        const int *e = c ? e1 : e0;
        const int a = 9 * NGs + j;
        keep = (a < 32) ? ss->attack_hist[c][a] : e[a - 32];
    }
    __builtin_amdgcn_wave_barrier();
    ss->attack_hist[c][j] = keep;
    if (lane == 0) { ss->short_flag_next_prev = prev_next; ss->bt_prev = prev_bt; }
}

// K0 (only when some stream asked for it, E_CONTROL filter_select = 1): the input DC blocker
// y = x - d, d += alpha * y (reference filter2.c:116-121,137-144).  A first-order recurrence
// evaluated in the reference's order, so it is sequential per channel: one lane per
// (stream, channel) walks its samples; streams without the filter are converted to float only.
__global__ void k_dcfilter(const int16_t *__restrict__ pcm, const float *__restrict__ pcm32, long long nsamp,
                           HxStream *__restrict__ st, const HxParams *__restrict__ prm, float *__restrict__ pcmf, int S, int pitch,
                           const int *__restrict__ nfr)
{
    // one lane per (stream, channel of the pitch): a lane whose channel its stream does not have leaves
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= pitch * S) return;
    const int s = u / pitch, ch = u - s * pitch;
    const long long nown = nfr ? 1152LL * nfr[s] : nsamp;      // the stream's samples of this call (nsamp: the row stride)
    HxStream *ss = st + s;
    const HxParams *p = prm + ss->cls;
    const int nchan = p->nchan;                                 // the stream's own: the stride inside its row
    if (ch >= nchan) return;
    const int16_t *src = pcm + (long long) s * nsamp * pitch + ch;
    const float *srcf = pcm32 + (long long) s * nsamp * pitch + ch;
    float *dst = pcmf + (long long) s * nsamp * pitch + ch;
    if (!p->filter_dc) {
        for (long long n = 0; n < nown; n++) dst[nchan * n] = pcm32 ? srcf[nchan * n] : (float) src[nchan * n];
        return;
    }
    const float alpha = p->filter_alpha;
    float d = ss->dc[ch];
    for (long long n0 = 0; n0 < nown; n0 += 8) {       // (a multiple of 1152)
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = pcm32 ? srcf[nchan * (n0 + k)] : (float) src[nchan * (n0 + k)];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float t = x[k] - d;
            d = d + alpha * t;
            dst[nchan * (n0 + k)] = t;
        }
    }
    ss->dc[ch] = d;
}

// Gate of a pipelined submit (hx_batch_submit_*): holds the stream it is launched on until `need` workgroups of
// the previous call's allocator kernel have started, i.e. until that kernel occupies its share of the chip.
// The front-end kernels behind the gate then queue for the slots that finishing streams free, and run in the
// allocator kernel's tail; released earlier they would take LDS away from allocator workgroups that have not
// started yet.  The counter runs over all launches of the batch and may wrap: `base` is its value when the
// previous launch began, and the distance is compared as unsigned.  Gives up after ~50 ms (late is harmless, a
// hang is not) and counts that in *timeouts, so the caller can see that the overlap degraded.
__global__ void k_gate(const unsigned *started_counter, unsigned base, unsigned need, int *timeouts)
{
    if (threadIdx.x != 0) return;
    const long long t0 = wall_clock64();        // 100 MHz
    while (__hip_atomic_load(started_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - base < need) {
        __builtin_amdgcn_s_sleep(32);
        if (wall_clock64() - t0 > 5000000LL) { atomicAdd(timeouts, 1); break; }
    }
}
