// hx_pcmin.hip - k_pcm_spread: a call's PCM segments (hx_batch_pcm_segments) spread into the rows the front end reads;
// k_pcm_planes (below, with its own comment): a call's channel planes (hx_batch_pcm_planes) interleaved into the same rows.
// Built as part of hx_pack.hip's unit, behind hx_ledger.hip.
//
// Under segments the caller's PCM is one image; stream s's input is the len_s bytes at img + off[s], in the order its row
// would hold them.  The front-end kernels read rows [S][row_bytes], so this kernel, at the head of the front end and on its
// stream, copies every segment to the start of its row in a batch-owned row buffer; nothing else of the pipeline knows.
// Workgroup (stream s, chunk c) moves bytes [c * HX_PCM_CHUNK, ...) of the segment, 16 per lane and step, all of a chunk's
// loads ahead of its stores; the grid covers the worst-case row, and a workgroup at or past len_s leaves at once.
//   len_s = n * 1152 * nchan * sample_bytes, n = nfr[s] (or nframes), nchan = prm[st[s].cls].nchan: the device's view in
//   stream order, as for every kernel behind an assign.  Every len_s is a multiple of 2304, so of 16: a segment is whole
//   vectors, no store carries padding.
// The row side is 16-byte aligned by construction (rows from hipMalloc, row_bytes a multiple of 16): every store is a
// dwordx4.  The image side carries no alignment promise (a file's data chunk 44 bytes into a buffer; int16 segments on any
// even address).  The segment's misalignment is workgroup-uniform: an aligned segment is read as dwordx4; any other from the
// two aligned 16-byte blocks a vector straddles, funnelled into place (v_alignbyte_b32, as k_dense_gather does).
// Two bounds:
//   - loads: with a misaligned segment every (whole) vector has bytes in both of its blocks, with an aligned one only the
//     first block is read - so only aligned blocks that hold a byte of the stream's own segment are touched;
//   - stores: vector v goes to row bytes [16 v, 16 v + 16) with v < len_s / 16 - nothing at or beyond len_s of the row, and
//     nothing of another stream's row (len_s <= row_bytes: the host's checks bound n by nframes, nchan by the pitch).
// A stream with n = 0 has no workgroup past the exit, so its offset is never read.  No LDS, no scratch, no atomics.
#include "hx_dev.h"

static_assert(HX_PCM_CHUNK % (16 * 256) == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
#define HX_PCM_STEPS (HX_PCM_CHUNK / 16 / 256)

__global__ __launch_bounds__(256) void k_pcm_spread(const unsigned char *__restrict__ img, const long long *__restrict__ off, unsigned char *__restrict__ rows,
                                                    long long row_bytes, int nframes, int sample_bytes, const HxStream *__restrict__ st,
                                                    const HxParams *__restrict__ prm, const int *__restrict__ nfr, int chunks)
{
    const int s = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int n = nfr ? nfr[s] : nframes;
    if (n <= 0) return;
    const int nchan = prm[__builtin_amdgcn_readfirstlane(st[s].cls)].nchan;
    const long long len = (long long) n * 1152 * nchan * sample_bytes;
    if ((long long) c * HX_PCM_CHUNK >= len) return;
    const unsigned char *src = img + off[s];
    uint4 *dst = reinterpret_cast<uint4 *>(rows + (long long) s * row_bytes);
    const unsigned mis = (unsigned) (reinterpret_cast<unsigned long long>(src) & 15u), ws = mis >> 2, sh = mis & 3;
    const uint4 *blk = reinterpret_cast<const uint4 *>(src - mis);
    const long long nv = len >> 4, v0 = (long long) c * (HX_PCM_CHUNK / 16) + (long long) threadIdx.x;
    uint4 lo[HX_PCM_STEPS], hi[HX_PCM_STEPS];
#pragma unroll
    for (int k = 0; k < HX_PCM_STEPS; k++) {
        const long long v = v0 + 256 * k;
        lo[k] = hi[k] = make_uint4(0, 0, 0, 0);
        if (v < nv) {
            lo[k] = blk[v];
            if (mis) hi[k] = blk[v + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < HX_PCM_STEPS; k++) {
        const long long v = v0 + 256 * k;
        if (v >= nv) break;
        uint4 val = lo[k];
        if (mis) {
            unsigned q[8] = {lo[k].x, lo[k].y, lo[k].z, lo[k].w, hi[k].x, hi[k].y, hi[k].z, hi[k].w};
            if (ws & 2) {
#pragma unroll
                for (int j = 0; j < 6; j++) q[j] = q[j + 2];
            }
            if (ws & 1) {
#pragma unroll
                for (int j = 0; j < 5; j++) q[j] = q[j + 1];
            }
            val.x = __builtin_amdgcn_alignbyte(q[1], q[0], sh);
            val.y = __builtin_amdgcn_alignbyte(q[2], q[1], sh);
            val.z = __builtin_amdgcn_alignbyte(q[3], q[2], sh);
            val.w = __builtin_amdgcn_alignbyte(q[4], q[3], sh);
        }
        dst[v] = val;
    }
}

// k_pcm_planes: a call's channel planes (hx_batch_pcm_planes) interleaved into the rows the front end reads, in k_pcm_spread's
// place at the head of the front end and on its stream, into the same row buffer.
//
// Under planes the caller's PCM is one image; channel c of stream s is the n * 1152 consecutive samples at
// img + pl[s] + c * pl[S + s] (pl: [2][S] offsets, then strides, relative to img; the host fills in the stride of a mono
// stream and of a stream that takes no frame).  The grid, len_s and the early exits are k_pcm_spread's: workgroup (stream s,
// chunk c) makes bytes [c * HX_PCM_CHUNK, ...) of the row, 16 per lane and step, all of a chunk's loads ahead of its stores.
//   Stereo: row vector v (16 bytes) is plane bytes [8 v, 8 v + 8) of either plane - four int16 samples of each, their
//   halfwords interleaved with v_perm_b32, or two floats of each.  A lane reads 8-byte blocks (form A of EXPERIMENTS.md: the
//   stores are the ideal pattern, the loads half the widest width; form B, 16-byte blocks and a register exchange between
//   two lanes, is named there and was not built).
//   Mono: k_pcm_spread's copy of plane 0, 16-byte blocks.
//   unit: every fp32 sample is x * 32768.0f, one IEEE multiplication (the unit keeps fp32 denormals and does not contract),
//   formed once, here.
// Loads.  Each plane has its own misalignment against its block size B (8 stereo, 16 mono), m = address % B, uniform over
// the workgroup; blk = the plane's start rounded down to B.  Vector v < nv needs plane bytes [B v, B v + B), which are bytes
// [B v + m, B v + m + B) from blk: block v and, when m > 0, block v + 1.  Block v holds plane byte B v (B v + m < B v + B);
// with m > 0 block v + 1 starts B - m > 0 bytes into the vector, at plane byte B v + B - m < B (v + 1) <= the plane's length
// (nv vectors are B nv plane bytes).  With m = 0 block v + 1 is not loaded.  So only aligned blocks that hold a byte of the
// stream's own plane are touched, and the funnel (v_alignbyte_b32) takes from them exactly the vector's bytes.
// Stores.  dwordx4 only, lane i of a step at row byte 16 * (step base + i); vector v < len_s / 16 of the stream's own row:
// nothing at or beyond len_s, nothing in another row (len_s <= row_bytes as for k_pcm_spread).
// A stream with n = 0 leaves before its offset or stride is read; a mono stream's stride is never read.
// No LDS, no scratch, no atomics.
static __device__ __forceinline__ unsigned pcm_scaled(unsigned x) { return __float_as_uint(__uint_as_float(x) * 32768.0f); }

__global__ __launch_bounds__(256) void k_pcm_planes(const unsigned char *__restrict__ img, const long long *__restrict__ pl, int S,
                                                    unsigned char *__restrict__ rows, long long row_bytes, int nframes, int sample_bytes, int unit,
                                                    const HxStream *__restrict__ st, const HxParams *__restrict__ prm, const int *__restrict__ nfr,
                                                    int chunks)
{
    const int s = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int n = nfr ? nfr[s] : nframes;
    if (n <= 0) return;
    const int nchan = prm[__builtin_amdgcn_readfirstlane(st[s].cls)].nchan;
    const long long len = (long long) n * 1152 * nchan * sample_bytes;
    if ((long long) c * HX_PCM_CHUNK >= len) return;
    const unsigned char *p0 = img + pl[s];
    uint4 *dst = reinterpret_cast<uint4 *>(rows + (long long) s * row_bytes);
    const long long nv = len >> 4, v0 = (long long) c * (HX_PCM_CHUNK / 16) + (long long) threadIdx.x;
    const bool f32 = sample_bytes == 4, scale = f32 && unit != 0;
    if (nchan == 1) {
        const unsigned mis = (unsigned) (reinterpret_cast<unsigned long long>(p0) & 15u), ws = mis >> 2, sh = mis & 3;
        const uint4 *blk = reinterpret_cast<const uint4 *>(p0 - mis);
        uint4 lo[HX_PCM_STEPS], hi[HX_PCM_STEPS];
#pragma unroll
        for (int k = 0; k < HX_PCM_STEPS; k++) {
            const long long v = v0 + 256 * k;
            lo[k] = hi[k] = make_uint4(0, 0, 0, 0);
            if (v < nv) {
                lo[k] = blk[v];
                if (mis) hi[k] = blk[v + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < HX_PCM_STEPS; k++) {
            const long long v = v0 + 256 * k;
            if (v >= nv) continue;
            uint4 val = lo[k];
            if (mis) {
                unsigned q[8] = {lo[k].x, lo[k].y, lo[k].z, lo[k].w, hi[k].x, hi[k].y, hi[k].z, hi[k].w};
                if (ws & 2) {
#pragma unroll
                    for (int j = 0; j < 6; j++) q[j] = q[j + 2];
                }
                if (ws & 1) {
#pragma unroll
                    for (int j = 0; j < 5; j++) q[j] = q[j + 1];
                }
                val.x = __builtin_amdgcn_alignbyte(q[1], q[0], sh);
                val.y = __builtin_amdgcn_alignbyte(q[2], q[1], sh);
                val.z = __builtin_amdgcn_alignbyte(q[3], q[2], sh);
                val.w = __builtin_amdgcn_alignbyte(q[4], q[3], sh);
            }
            if (scale) val = make_uint4(pcm_scaled(val.x), pcm_scaled(val.y), pcm_scaled(val.z), pcm_scaled(val.w));
            dst[v] = val;
        }
        return;
    }
    const unsigned char *p1 = p0 + pl[S + s];
    const unsigned m0 = (unsigned) (reinterpret_cast<unsigned long long>(p0) & 7u), m1 = (unsigned) (reinterpret_cast<unsigned long long>(p1) & 7u);
    const uint2 *b0 = reinterpret_cast<const uint2 *>(p0 - m0), *b1 = reinterpret_cast<const uint2 *>(p1 - m1);
    uint2 l0[HX_PCM_STEPS], h0[HX_PCM_STEPS], l1[HX_PCM_STEPS], h1[HX_PCM_STEPS];
#pragma unroll
    for (int k = 0; k < HX_PCM_STEPS; k++) {
        const long long v = v0 + 256 * k;
        l0[k] = h0[k] = l1[k] = h1[k] = make_uint2(0, 0);
        if (v < nv) {
            l0[k] = b0[v];
            if (m0) h0[k] = b0[v + 1];
            l1[k] = b1[v];
            if (m1) h1[k] = b1[v + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < HX_PCM_STEPS; k++) {
        const long long v = v0 + 256 * k;
        if (v >= nv) continue;
        uint2 a = l0[k], b = l1[k];
        if (m0) {
            unsigned q[4] = {l0[k].x, l0[k].y, h0[k].x, h0[k].y};
            if (m0 & 4) {
#pragma unroll
                for (int j = 0; j < 3; j++) q[j] = q[j + 1];
            }
            a.x = __builtin_amdgcn_alignbyte(q[1], q[0], m0 & 3);
            a.y = __builtin_amdgcn_alignbyte(q[2], q[1], m0 & 3);
        }
        if (m1) {
            unsigned q[4] = {l1[k].x, l1[k].y, h1[k].x, h1[k].y};
            if (m1 & 4) {
#pragma unroll
                for (int j = 0; j < 3; j++) q[j] = q[j + 1];
            }
            b.x = __builtin_amdgcn_alignbyte(q[1], q[0], m1 & 3);
            b.y = __builtin_amdgcn_alignbyte(q[2], q[1], m1 & 3);
        }
        uint4 val;
        if (f32) {
            val = make_uint4(a.x, b.x, a.y, b.y);
            if (scale) val = make_uint4(pcm_scaled(val.x), pcm_scaled(val.y), pcm_scaled(val.z), pcm_scaled(val.w));
        } else {
            // (v_perm_b32: selector bytes 0 .. 3 take the second operand's bytes, 4 .. 7 the first's)
            val.x = __builtin_amdgcn_perm(b.x, a.x, 0x05040100u);
            val.y = __builtin_amdgcn_perm(b.x, a.x, 0x07060302u);
            val.z = __builtin_amdgcn_perm(b.y, a.y, 0x05040100u);
            val.w = __builtin_amdgcn_perm(b.y, a.y, 0x07060302u);
        }
        dst[v] = val;
    }
}
