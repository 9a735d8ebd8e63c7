"""The inputs of the finished-file tests (include/hmp3_amd.h, "finished files"): tests/test_gpu_file_tags.py runs them on the
GPU, tests/test_file_tags_abi.py holds hx_file_tag_build to the three hx_xing_* calls on them and checks on the CPU, with the
oracle alone, that the GPU shape reaches the edges it exists for.

The GPU shape: one hx_batch_create_any batch of seven slots under per-stream counts, calls of 8 frames.  Every slot has its
own configuration and, through it, its own tag frame; slot LONG takes at least 520 input calls, so that its table of 512 seek
points halves once (every == 2), and the other slots sit its later calls out."""
import ctypes as C

import numpy as np

CALL = 8                # frames per call
DRAIN = 32              # frames of silence a file may take behind its input
# kw: the control; ch: the source's channels; xing: the command line's -X flag (0: no tag, 1: counts, 3: counts, TOC and the
# LAME fields); ncalls: the file's input calls
SLOTS = [
    dict(kw=dict(), ch=2, xing=3, ncalls=5),                                    # 44.1 kHz stereo VBR
    dict(kw=dict(samprate=48000, bitrate=64), ch=2, xing=3, ncalls=12),         # 48 kHz stereo CBR-128
    dict(kw=dict(mode=3, samprate=32000, bitrate=48), ch=1, xing=3, ncalls=3),  # 32 kHz mono CBR-48: the TOC is dropped from the frame
    dict(kw=dict(samprate=22050), ch=2, xing=3, ncalls=20),                     # 22.05 kHz stereo (two frames per call)
    dict(kw=dict(mode=3, samprate=16000), ch=1, xing=1, ncalls=7),              # 16 kHz mono: no TOC, no LAME fields
    dict(kw=dict(), ch=2, xing=0, ncalls=1),                                    # untagged: head_bytes 0
    dict(kw=dict(mode=3), ch=1, xing=3, ncalls=524),                            # 44.1 kHz mono: the table halves
]
NO_TOC_CBR, MPEG2, COUNTS_ONLY, UNTAGGED, LONG = 2, 3, 4, 5, 6
TAIL = 2 * 1152 + 77    # samples of silence between the audio's end and the end of the file's last input call
MID_CALL = 0            # the tags are also built behind this call (0-based): the files of more than 5 calls are live then


def control_of(api, s):
    return api.default_control(**SLOTS[s]["kw"])


def resolved(api, ec):
    """(the control the encoder runs, its frame header) as hx_control_info reports them"""
    used, head = api.EControl(), api.MpegHead()
    assert api.lib().hx_control_info(C.byref(ec), C.byref(used), C.byref(head)) != 0
    return used, head


def tag_of(api, ec, ch, xing, samples_audio, in_samplerate=None):
    """the FileTag the command-line tool's Tagger would describe: begin()'s flags and hx_xing_header arguments, finish()'s
    hx_xing_update_info arguments"""
    used, head = resolved(api, ec)
    flags = (1 | 2 | 8 if xing else 0) | (4 | 0x40 if xing & 2 else 0)
    return api.FileTag(samprate=used.samprate, h_mode=head.mode, cr_bit=used.cr_bit, original_bit=used.original, flags=flags,
                       kbps=used.bitrate * ch, vbr_scale=used.vbr_mnr if used.vbr_flag else -1, lowpass=used.freq_limit,
                       in_samplerate=used.samprate if in_samplerate is None else in_samplerate, reserved=0, samples_audio=samples_audio)


def slot_tag(api, s, samples_audio=None, in_samplerate=None):
    """slot s's tag; samples_audio None: the file's true length.  An untagged slot's is all zero: it names no sample rate and
    so describes no frame (size 0) - the tool's Tagger never calls hx_xing_header for such a file"""
    c = SLOTS[s]
    if not c["xing"]:
        return api.FileTag()
    n = true_samples(s) if samples_audio is None else samples_audio
    return tag_of(api, control_of(api, s), c["ch"], c["xing"], n, in_samplerate)


def true_samples(s):
    """the file's true length in samples: its input calls are those of the single-file loop, which feeds the audio and then
    silence, so the audio ends TAIL samples in front of the last call's end.  The drain ends when the frame counter reaches
    the input calls, so frames x 1152 (MPEG-2: 2 frames x 576) = ncalls x 1152 and the trimming rule's difference
    frames x spf - audio - 1680 is TAIL - 1680 = 701: below 4096, the rule does not fire"""
    return max(SLOTS[s]["ncalls"] * 1152 - TAIL, 1)


def slot_head(api, s):
    return api.file_tag_bytes(slot_tag(api, s)) if SLOTS[s]["xing"] else 0


def slot_flags(s):
    """the record's flags: seek points are kept for a file whose tag may hold a TOC"""
    return 1 if SLOTS[s]["xing"] & 2 else 0


def grid(api, s):
    """the parameter grid of the ended records: samples_audio x in_samplerate.  With the file's true length the frames exceed
    the audio by the encoder's delay and the padding of the last frame - about 2 x 1152 - and the trimming rule's difference
    mp3 - audio - 1680 is 701 (true_samples): it does not fire.  With samples_audio = 0 the rule is not looked at and the LAME
    fields are skipped; with 1 the difference is far beyond 4096: it fires; with the true length + 10 x 1152 the audio is longer
    than the frames, the unsigned difference wraps to 2^64 - (10 x 1152 - 701) and the rule fires from the other side."""
    true = true_samples(s)
    sr = resolved(api, control_of(api, s))[0].samprate
    return [slot_tag(api, s, n, r) for n in (0, 1, true, true + 10 * 1152) for r in (0, 44100, 48000, 96000, sr // 2)]


def trim_fires(frames, spf, samples_audio, in_sr, out_sr):
    """hx_xing_update_info's rule, worked out in exact integer / double arithmetic: -> (fires, the unsigned 64-bit difference)"""
    if in_sr == 0 or out_sr == 0:
        in_sr = out_sr = 1
    audio = int(float(samples_audio) * (float(out_sr) / float(in_sr)) + 0.5)
    d = (frames * spf - audio - 1680) % (1 << 64)
    return d >= 4096, d


def slot_pcm(synth, s):
    """the file's PCM [ncalls * 1152, ch] float32"""
    c = SLOTS[s]
    sr = c["kw"].get("samprate", 44100)
    pcm = synth.stream_pcm(9100 + s, c["ncalls"], sr=sr, bursts=True)[:, :c["ch"]].astype(np.float32)
    pcm[true_samples(s):] = 0
    return pcm


def counts_at(given):
    """the call's per-stream counts: every file takes up to CALL frames until it has had its input and DRAIN frames of silence"""
    return [max(0, min(CALL, c["ncalls"] + DRAIN - g)) for c, g in zip(SLOTS, given)]


def three_calls(api, rec, tag):
    """the reference of hx_file_tag_build: the three hx_xing_* calls the header names, on an hx_xing of the caller's -> the
    first head_bytes bytes, b"" where hx_xing_header returns 0 or the record's points are refused"""
    L = api.lib()
    x = L.hx_xing_create()
    try:
        buf = (C.c_ubyte * 2048)()
        size = L.hx_xing_header(x, tag.samprate, tag.h_mode, tag.cr_bit, tag.original_bit, tag.flags, 0, 0, tag.vbr_scale, None, buf, None, None, tag.kbps)
        if size == 0 or size != rec.head_bytes or L.hx_xing_load_points(x, C.byref(rec)) != 1:
            return b"", size
        n = rec.head_bytes + rec.bytes
        assert L.hx_xing_update_info(x, rec.frames, n, tag.vbr_scale, None, buf, None, None, tag.samples_audio, n, tag.lowpass, tag.in_samplerate,
                                     tag.samprate, rec.crc) == 1
        return bytes(buf[:size]), size
    finally:
        L.hx_xing_destroy(x)


def drive(api, ncalls, fpc=1, head=0, flags=1, call=CALL, delay=2, stall=0, seed=5):
    """a record through hx_ledger_update on synthetic counters, in calls of `call` input frames until the file ends: the
    encoder runs `delay` frames behind its input and emits nothing for the `stall` input frames after that (repeated seek
    points), fpc frames per input frame afterwards -> the record"""
    rec = api.ledger_open(ncalls, fpc, head, flags)
    rng = np.random.default_rng(seed)
    fed, fr, by = 0, 0, 0
    while not rec.ended:
        st = np.zeros((call, 2), np.int32)
        nb = 0
        for f in range(call):
            out = fpc if fed >= delay + stall else 0
            add = sum(int(rng.integers(96, 700)) for _ in range(out))
            fr, by, nb, fed = fr + out, by + add, nb + add, fed + 1
            st[f] = fr, by
        api.ledger_update(rec, st, rng.integers(0, 65536, call).astype(np.uint16), nb)
        assert fed < ncalls + 64 * call
    return rec


def oracle_records(api, O, synth, stop=None):
    """the GPU shape through the CPU oracle and hx_ledger_update -> the records behind call `stop` (None: at the end)"""
    S = len(SLOTS)
    enc = [O.OracleEncoder(O.default_control(**c["kw"])) for c in SLOTS]
    full = [slot_pcm(synth, s) for s in range(S)]
    rec = [api.ledger_open(c["ncalls"], 1 if resolved(api, control_of(api, s))[1].id else 2, slot_head(api, s), slot_flags(s)) for s, c in enumerate(SLOTS)]
    given, call = [0] * S, 0
    while True:
        counts = counts_at(given)
        if not any(counts) or (stop is not None and call > stop):
            return rec
        for s, n in enumerate(counts):
            st, nb = np.zeros((n, 2), np.int32), 0
            for f in range(n):
                blk = np.zeros((1152, SLOTS[s]["ch"]), np.float32)
                part = full[s][(given[s] + f) * 1152:(given[s] + f + 1) * 1152]
                blk[:len(part)] = part
                nb += len(enc[s].encode_f32(blk))
                st[f] = enc[s].frames_out(), enc[s].bytes_out()
            if n:
                api.ledger_update(rec[s], st, np.zeros(n, np.uint16), nb)
            given[s] += n
        call += 1
