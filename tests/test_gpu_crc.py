"""The MusicCRC output of the batched calls on a real MI355X (include/hmp3_amd.h, "MusicCRC"; k_crc in
hmp3_amd/csrc/hx_crc.hip): per stream and input frame the CRC-16 of the bytes the call had emitted by then, from seed 0.

Every comparison is equality.  The expected value is hx_xing_update_crc on the host over the row's first e[f] bytes, with
e[f] = out_bytes - (stats[last][1] - stats[f][1]) from the call's own frame counters (tests/test_xing_tag.py pins
hx_xing_update_crc to the reference).  Rows, byte counts and counters are compared with a twin batch that has no CRC
buffer.  CRC buffers are prefilled with 0xA5A5 and carry a guard region behind [S][F] that must stay untouched.
The CRC does not depend on the build of the rate-loop kernel, so the tests run once (one_k6_build); one test runs both
builds, each in a child process of its own."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from dense_cases import mixed_controls, mixed_pcm
from gpu_support import ROOT, CallBufs, batch_vs_single_vs_reference, cur_stream, cut, dev, host_crc, sync, write_wav
import gpu_support as G
from hmp3_amd import api, synth
from output_checks import expected_crc
from src_cases import Stream, make_batch

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
FILL16 = 0xA5A5
GUARD = 2048            # uint16 entries behind [S][F]
PASS_BYTES = 64 * 256   # what one pass of k_crc's workgroup covers (HX_CRC_CHUNK * HX_CRC_LANES)


def out_bufs(b, nf, shift=0, extra=0):
    """every output buffer of one call: rows (first row `shift` bytes past a 16-byte boundary, `extra` bytes added to the
    stride), byte counts, frame counters and the CRC buffer prefilled with FILL16, its guard region behind it"""
    return CallBufs(b, nf, shift=shift, extra=extra, counters=True, crc=True, crc_fill=FILL16, crc_guard=GUARD)


def device_call(b, blk, nf, crc=True, shift=0, extra=0, submit=False):
    return G.device_call(b, blk, nf, out_bufs(b, nf, shift, extra).set_on(b, crc=crc), submit=submit)


def check(out, tag):
    """the contract of one call's CRC buffer -> (rows, nb, stats, crc, e)"""
    rows, nb, stats, crc, guard = out.host()
    assert (nb >= 0).all(), tag
    want, e = expected_crc(rows, nb, stats)
    bad = np.argwhere(crc != want)
    assert bad.size == 0, "%s: stream %d frame %d (e = %d of %d): crc %04x, host %04x" % (
        (tag,) + tuple(bad[0]) + (e[tuple(bad[0])], nb[bad[0][0]], crc[tuple(bad[0])], want[tuple(bad[0])]))
    assert (crc[e == 0] == 0).all(), tag
    assert (guard == FILL16).all(), tag + ": entries written behind [S][F]"
    return rows, nb, stats, crc, e




def run_twins(make, pcm, calls, shift=0, extra=0, tag=""):
    """the same plain device calls on two batches from make(), one with a CRC buffer and one without: rows, byte counts
    and counters identical, every CRC buffer checked -> per call (rows, nb, stats, crc, e)"""
    bc, bt = make(), make()
    res, f0 = [], 0
    for c, nf in enumerate(calls):
        oc = device_call(bc, cut(pcm, f0, nf), nf, True, shift, extra)
        ot = device_call(bt, cut(pcm, f0, nf), nf, False, shift, extra)
        sync()
        r = check(oc, "%s call %d" % (tag, c))
        trows, tnb, tstats, tcrc, tguard = ot.host()
        assert r[1].tolist() == tnb.tolist() and (r[0] == trows).all() and (r[2] == tstats).all(), "%s call %d: rows / byte counts / counters differ from the twin batch's" % (tag, c)
        assert (tcrc == FILL16).all() and (tguard == FILL16).all(), "%s call %d: a batch without CRC buffer wrote one" % (tag, c)
        res.append(r)
        f0 += nf
    assert bc.status() == 0 and bt.status() == 0
    bc.close()
    bt.close()
    return res


def batch_of(controls, maxF, **kw):
    return lambda: api.Batch(controls, max_frames=maxF, **kw)


def test_mixed_rates_three_calls_and_their_fold():
    """5 streams at 32 / 44.1 / 48 kHz, VBR-50, calls of 1, 3 and 4 frames: the first call has streams that have emitted
    nothing (e = 0, CRC 0); the three calls' last entries folded by crc_combine equal the CRC of the concatenated stream"""
    S, calls = 5, [1, 3, 4]
    res = run_twins(batch_of(mixed_controls(S), max(calls)), mixed_pcm(S, sum(calls), 4000), calls, tag="mixed")
    assert (res[0][4] == 0).any() and res[2][1].min() > 0 and len(set(res[2][1].tolist())) > 1
    for s in range(S):
        run, whole = 0, b""
        for rows, nb, stats, crc, e in res:
            run = api.crc_combine(run, int(crc[s, -1]), int(nb[s]))
            whole += rows[s, :nb[s]].tobytes()
        assert run == host_crc(whole) and len(whole) > 0, "stream %d" % s


def test_rows_longer_than_one_pass_of_the_workgroup():
    """3 streams, CBR-320 stereo, 48 frames: rows of about 48 KB, which take three passes of 16 KB each"""
    S, F = 3, 48
    pcm = np.stack([synth.stream_pcm(4100 + i, F, rho=(0.7, 0.0, 0.3)[i], bursts=True) for i in range(S)]).astype(np.float32)
    (rows, nb, stats, crc, e), = run_twins(batch_of(api.default_control(bitrate=160), F, nstreams=S), pcm, [F], tag="cbr320")
    assert nb.min() > 2 * PASS_BYTES + 16
    assert len(set((e[0] // PASS_BYTES).tolist())) >= 3        # frames end in several passes


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_rows_without_alignment(shift):
    """the first row 1, 7 and 15 bytes past a 16-byte boundary and out_stride = hx_batch_out_stride + 13: every row has
    another misalignment"""
    S = 5
    res = run_twins(batch_of(mixed_controls(S), 4), mixed_pcm(S, 8, 4000), [4, 4], shift, 13, tag="shift %d" % shift)
    assert res[1][1].min() > 0


def test_pipelined_submits_write_the_buffers_set_at_the_submit():
    """two submits with a set of every buffer each; the CRC buffer is switched off between the second submit and
    hx_batch_wait, and both submits' CRCs arrive in their own buffers; rows and byte counts are a plain twin's"""
    import torch
    S, calls = 5, [3, 4]
    controls, pcm = mixed_controls(S), mixed_pcm(S, sum(calls), 4000)
    t = api.Batch(controls, max_frames=max(calls))
    want = []
    for c, nf in enumerate(calls):
        o = device_call(t, cut(pcm, sum(calls[:c]), nf), nf, crc=False)
        sync()
        want.append(o.host())
    t.close()
    b = api.Batch(controls, max_frames=max(calls))
    outs = [out_bufs(b, nf) for nf in calls]
    d_pcm = [torch.from_numpy(cut(pcm, sum(calls[:c]), nf)).to(dev()) for c, nf in enumerate(calls)]
    sync()
    for c, nf in enumerate(calls):
        outs[c].set_on(b)
        b.submit_device(d_pcm[c].data_ptr(), nf, outs[c].ptr, outs[c].stride, outs[c].nb.data_ptr(), cur_stream(), f32=True)
    b.crc_buffer(None)
    b.wait(cur_stream())
    sync()
    assert b.status() == 0
    b.close()
    for c in range(2):
        rows, nb, stats, crc, e = check(outs[c], "submit %d" % c)
        assert nb.tolist() == want[c][1].tolist() and (stats == want[c][2]).all(), "submit %d" % c
        for s in range(S):
            assert rows[s, :nb[s]].tobytes() == want[c][0][s, :nb[s]].tobytes(), "submit %d stream %d" % (c, s)
    assert outs[1].host()[1].min() > 0


def test_mpeg2_batch():
    """22.05 kHz: every input frame yields two frames; two frames per call"""
    S = 4
    pcm = np.stack([synth.stream_pcm(4200 + i, 6, sr=22050, rho=(0.7, 0.0, 1.0, 0.3)[i], bursts=True) for i in range(S)]).astype(np.float32)
    res = run_twins(batch_of([api.default_control(samprate=22050) for _ in range(S)], 2), pcm, [2, 2, 2], tag="mpeg2")
    assert res[2][1].min() > 0


def test_mono_batch():
    S = 4
    pcm = np.stack([synth.stream_pcm(4300 + i, 8, bursts=True)[:, 0] for i in range(S)]).astype(np.float32)[:, :, None]
    res = run_twins(batch_of(api.default_control(mode=3), 5, nstreams=S), pcm, [3, 5], tag="mono")
    assert res[1][1].min() > 0


def test_first_generation_allocator_batch():
    """dual channel at 16 kHz, 2 x 8 kbit/s (the configuration of the golden stream a1_dual_16k_antiphase): k_alloc1_lsf"""
    S = 3
    pcm = np.stack([synth.stream_pcm(4400 + i, 8, sr=16000, rho=(1.0, 0.25, 0.0)[i], bursts=True) for i in range(S)]).astype(np.float32)
    res = run_twins(batch_of(api.default_control(samprate=16000, mode=2, bitrate=8), 4, nstreams=S), pcm, [4, 4], tag="dual 16k")
    assert res[1][1].min() > 0


def child_check(build):
    """(runs in a child process with HMP3AMD_K6 = build in its environment, which a batch reads when it is created)"""
    S = 5
    b = api.Batch(mixed_controls(S), max_frames=4)
    assert b.k6_variant() == {"fat": 0, "slim": 1}[build]
    b.close()
    res = run_twins(batch_of(mixed_controls(S), 4), mixed_pcm(S, 8, 4000), [4, 4], tag=build)
    assert res[1][1].min() > 0


@pytest.mark.parametrize("build", ["fat", "slim"])
def test_both_builds_of_the_rate_loop_kernel(build):
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_crc as T; T.child_check(%r)" % (ROOT, os.path.join(ROOT, "tests"), build)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HMP3AMD_K6=build), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]


def test_converting_batch():
    """hx_batch_encode_src_device, 48 kHz 24-bit sources encoded at 44.1 kHz, two calls"""
    import torch
    streams = [Stream(48000, 24, 0, mpeg_select=44100, seed=91 + i, seconds=1.0) for i in range(4)]
    S, nf = len(streams), 4
    pos = {True: [0] * S, False: [0] * S}
    batches = {True: make_batch(streams, nf), False: make_batch(streams, nf)}
    for c in range(2):
        got = {}
        for with_crc, b in batches.items():
            in_stride = b.in_stride(nf)
            rows_in = np.zeros((S, in_stride), np.uint8)
            for i, s in enumerate(streams):
                chunk = np.frombuffer(s.data[pos[with_crc][i]:pos[with_crc][i] + in_stride], np.uint8)
                rows_in[i, :len(chunk)] = chunk
            d_in = torch.from_numpy(rows_in).to(dev())
            o = out_bufs(b, nf)
            used = np.zeros(S, np.int64)
            sync()
            o.set_on(b, crc=with_crc)
            assert api.lib().hx_batch_encode_src_device(b.h, d_in.data_ptr(), in_stride, None, nf, o.ptr, o.stride, o.nb.data_ptr(),
                                                          used.ctypes.data, cur_stream()) == 0, api.last_error()
            sync()
            assert b.status() == 0
            got[with_crc] = o
            for i in range(S):
                pos[with_crc][i] += int(used[i])
        rows, nb, stats, crc, e = check(got[True], "converting call %d" % c)
        trows, tnb, tstats, tcrc, _ = got[False].host()
        assert nb.tolist() == tnb.tolist() and (rows == trows).all() and (stats == tstats).all() and (tcrc == FILL16).all()
    assert nb.min() > 0
    for b in batches.values():
        b.close()


def test_host_calls_return_the_crcs_of_the_device_path():
    """hx_batch_encode_f32_host_crc and hx_multi_encode_f32_host_crc (three blocks on device 0 over 7 streams: uneven
    blocks) against plain device calls with a CRC buffer, two calls"""
    S, calls = 7, [1, 3]
    controls, pcm = mixed_controls(S), mixed_pcm(S, sum(calls), 4000)
    want = run_twins(batch_of(controls, max(calls)), pcm, calls, tag="device path")
    b = api.Batch(controls, max_frames=max(calls))
    m = api.Multi(controls, max_frames=max(calls), devices=[0, 0, 0])
    assert [m.shard(k)[2] for k in range(3)] == [3, 2, 2]
    for c, nf in enumerate(calls):
        rows, nb, stats, crc, e = want[c]
        blk = cut(pcm, sum(calls[:c]), nf)
        for name, h in (("batch", b), ("multi", m)):
            res, st, cr = h.encode_host(blk, stats=True, crc=True)
            assert res == [rows[s, :nb[s]].tobytes() for s in range(S)], "%s call %d" % (name, c)
            assert (st == stats).all() and cr.dtype == np.uint16 and (cr == crc).all(), "%s call %d" % (name, c)
    assert b.status() == 0 and m.status() == 0 and want[1][1].min() > 0
    n = S * calls[1]
    null = [(b.h, api.lib().hx_batch_encode_f32_host_crc), (m.h, api.lib().hx_multi_encode_f32_host_crc)]
    out, nb, st, cr = np.zeros((S, b.out_stride(3)), np.uint8), np.zeros(S, np.int32), np.zeros(2 * n, np.int32), np.zeros(n, np.uint16)
    for h, fn in null:      # both arrays are required
        assert fn(h, blk.ctypes.data, 3, out.ctypes.data, out.shape[1], nb.ctypes.data, st.ctypes.data, None) == -1
        assert fn(h, blk.ctypes.data, 3, out.ctypes.data, out.shape[1], nb.ctypes.data, None, cr.ctypes.data) == -1
    b.close()
    m.close()


def test_crc_buffer_without_frame_counters_is_refused():
    """-1 with a message before anything runs (call and submit), hx_batch_status stays 0, nothing is written, and the
    next well-formed call on the batch is correct; an odd d_crc is refused by the setter"""
    import torch
    S, nf = 5, 4
    controls, pcm = mixed_controls(S), mixed_pcm(S, 8, 4000)
    want = run_twins(batch_of(controls, nf), pcm, [nf, nf], tag="twin")
    b = api.Batch(controls, max_frames=nf)
    o = out_bufs(b, nf)
    d_pcm = torch.from_numpy(cut(pcm, 0, nf)).to(dev())
    sync()
    L = api.lib()
    with pytest.raises(RuntimeError, match="2-byte aligned"):
        b.crc_buffer(o.crc.data_ptr() + 1)
    b.crc_buffer(o.crc.data_ptr())
    for fn in (L.hx_batch_encode_f32_device, L.hx_batch_submit_f32_device):
        assert fn(b.h, d_pcm.data_ptr(), nf, o.ptr, o.stride, o.nb.data_ptr(), cur_stream()) == -1
        assert "frame-counter" in api.last_error()
    assert b.status() == 0
    sync()
    rows, nb, stats, crc, guard = o.host()
    assert (nb == -1).all() and (stats == -1).all() and (crc == FILL16).all() and not rows.any()
    for c in range(2):
        o = device_call(b, cut(pcm, c * nf, nf), nf)
        sync()
        rows, nb, stats, crc, e = check(o, "after the refusal, call %d" % c)
        assert nb.tolist() == want[c][1].tolist() and (rows == want[c][0]).all() and (crc == want[c][3]).all()
    assert b.status() == 0
    b.close()


def test_cli_batch_mode_writes_the_crc_of_the_audio_bytes(tmp_path):
    """`hmp3amd -batch` on three WAVs of 40, 100 and 200 frames (calls of 96 frames: the files end in the first, second
    and third call, each inside it): the outputs equal the single-file mode's byte for byte, and the MusicCRC field of
    the tag is the host's CRC of the audio bytes behind the tag frame"""
    kbps = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
    files = []
    for i, frames in enumerate((40, 100, 200)):
        wav = str(tmp_path / ("in%d.wav" % i))
        write_wav(wav, synth.stream_pcm(4500 + i, frames, bursts=True)[:frames * 1152 - 333 * i], 44100, False)
        files.append((wav, wav, str(tmp_path / ("batch%d.mp3" % i))))
    _, outputs = batch_vs_single_vs_reference(files, reference=False)
    for (wav, _, _), data in zip(files, outputs):
        assert data[0] == 0xFF and (data[1] >> 3) & 1 == 1 and (data[2] >> 2) & 3 == 0       # MPEG-1, 44.1 kHz
        head_bytes = 144000 * kbps[data[2] >> 4] // 44100
        at = data.index(b"LAMEH5.24", 0, head_bytes) + 32     # version 9, revision 1, lowpass 1, ReplayGain 8, flags 2, delays 3, misc 4, length 4
        assert struct.unpack(">I", data[at - 4:at])[0] == len(data)
        assert struct.unpack(">H", data[at:at + 2])[0] == host_crc(data[head_bytes:]), wav
        assert len(data) > head_bytes + 10000
