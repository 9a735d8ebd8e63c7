// hx_pcmin.hip - k_pcm_spread: a call's PCM segments (hx_batch_pcm_segments) spread into the rows the front end reads.
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
