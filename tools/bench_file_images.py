"""The file route with and without file images, at the command-line tool's call shape: a mixed batch (stereo and mono
entries alternating), calls of 96 frames under per-stream counts that cycle, the PCM as one packed image (PCM segments) in
page-locked memory, files of a few calls that end on the way and whose slots take the next file.  Three twin batches take the
same calls, alternated call by call in one process:
  rows:    hx_batch_encode_f32_host_crc + hx_batch_ledger_read of the fed slots + the host's append of rows[s, :call_bytes]
  images:  hx_batch_encode_f32_host_files + hx_batch_ledger_poll, and for the files that ended in the call one
           hx_batch_ledger_read of their slots and one hx_batch_file_fetch each
  many:    hx_batch_encode_f32_host_files + hx_batch_ledger_poll, and for the files that ended in the call one
           hx_batch_file_tags (their tag frames built on the GPU) and one hx_batch_file_fetch_many (all of them as one image)
Per loop: ms per call (median; the call alone, the records, the append / the fetches) and the bytes that cross the link in
each direction per call - counted from what each entry point copies by its contract (include/hmp3_amd.h), not measured on
the bus - and the launches and copies a call makes for its finished files.  The files of the three loops are compared at
the end (the audio bytes; the third loop's files carry their tag frames in front).  One JSON line.
  python tools/bench_file_images.py [--streams 512] [--steps 24] [--file-frames 600] [--out profiles/file_images.json]
--file-frames takes a list (600,150: the two shapes of DESIGN.md section 7, profiles/file_images_many.json): one run and one
JSON line per shape, and --out then holds one object with a member per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CH, DRAIN, HEAD = 96, 32, 417


PINNED = []             # what a shape's run allocated page-locked: released behind it


def pinned(L, nbytes, dtype):
    p = L.hx_pinned_alloc(int(nbytes))
    if not p:
        raise MemoryError("hx_pinned_alloc(%d)" % nbytes)
    PINNED.append(p)
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(int(nbytes),)).view(dtype)


def slot_tag(api, ec, channels, nframes):
    """the FileTag of a file of nframes input frames under control ec, as the command-line tool describes it for -X2"""
    used, head = api.EControl(), api.MpegHead()
    assert api.lib().hx_control_info(C.byref(ec), C.byref(used), C.byref(head)) != 0
    return api.FileTag(samprate=used.samprate, h_mode=head.mode, cr_bit=used.cr_bit, original_bit=used.original, flags=1 | 2 | 4 | 8 | 0x40,
                       kbps=used.bitrate * channels, vbr_scale=used.vbr_mnr if used.vbr_flag else -1, lowpass=used.freq_limit,
                       in_samplerate=used.samprate, reserved=0, samples_audio=max(1, nframes * 1152 - 2381))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--file-frames", default="600", help="the shortest file's frames (a slot's files have this + 41 * (slot mod 7)); a comma-separated list: one run per value")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    shapes = [int(v) for v in args.file_frames.split(",")]
    results = {}
    for ff in shapes:
        args.file_frames = ff
        res, same = run(args)
        print(json.dumps(res))
        results["files_%d_to_%d_frames" % (ff, ff + 41 * 6)] = res
        if not same:
            sys.exit("the loops' files differ")
    if args.out:
        with open(args.out, "w") as f:
            f.write((json.dumps(results[next(iter(results))]) if len(shapes) == 1 else json.dumps(results, indent=1)) + "\n")


def run(args):
    """one shape -> (the result, whether the loops' files are identical)"""
    from hmp3_amd import api, synth
    S, L = args.streams, api.lib()
    menu = [api.default_control(), api.default_control(mode=3)]
    cfg = [s & 1 for s in range(S)]
    nch = [2 - c for c in cfg]
    batch = {v: api.Batch.mixed(menu, S, cfg=cfg, max_frames=CH) for v in ("rows", "images", "many")}
    stride = batch["rows"].out_stride(CH)
    nfile = [args.file_frames + 41 * (s % 7) for s in range(S)]     # calls (frames) of every file of slot s
    cap = HEAD + (max(nfile) + DRAIN) * batch["rows"].out_stride(1)
    batch["images"].file_images(cap)
    batch["many"].file_images(cap)
    tags = [slot_tag(api, menu[cfg[s]], nch[s], nfile[s]) for s in range(S)]
    head = {v: [api.file_tag_bytes(tags[s]) if v == "many" else HEAD for s in range(S)] for v in batch}
    assert all(0 < h <= HEAD for h in head["many"])
    many_buf = pinned(L, 16, np.uint8)
    many_off = np.zeros(S + 1, np.int64)
    src = synth.batch_pcm(S, CH, unique=16).astype(np.float32)      # every call feeds these frames again: the cost does not depend on them
    pcm = pinned(L, S * CH * 1152 * 2 * 4, np.float32)
    out = pinned(L, S * stride, np.uint8).reshape(S, stride)
    stats = pinned(L, S * CH * 2 * 4, np.int32)
    crc = pinned(L, S * CH * 2, np.uint16)
    nb = np.zeros(S, np.int32)
    led = (api.Ledger * S)()
    brief = (api.LedgerBrief * S)()
    files = {v: [bytearray() for _ in range(S)] for v in batch}     # rows: appended call by call; images: fetched at the end
    done = {v: [] for v in batch}
    fetch_buf = pinned(L, cap, np.uint8)
    fed = {v: [0] * S for v in batch}
    ended = {v: [False] * S for v in batch}

    def begin(v, slots):
        b = batch[v]
        b.ledger_begin(slots, [nfile[s] for s in slots], [head[v][s] for s in slots], 1)
        b.reset_streams(slots)
        for s in slots:
            fed[v][s], ended[v][s] = 0, False

    for v in batch:
        begin(v, list(range(S)))
    t = {v: {"call": [], "records": [], "files": []} for v in batch}
    link = {v: {"up": [], "down": []} for v in batch}
    pattern = (CH, CH, 48, 0, CH, 17, CH, 64)
    nfetched = nmany = 0
    for step in range(args.steps + 1):              # (step 0: warm-up, not counted)
        for v in batch:
            b = batch[v]
            cnt = [0 if ended[v][s] else min(pattern[(s + step) % len(pattern)], nfile[s] + DRAIN - fed[v][s]) for s in range(S)]
            off, total = api.packed_layout(CH, nch, cnt, f32=True)
            for s in range(S):
                n = cnt[s] * 1152 * nch[s]
                pcm[off[s] // 4:off[s] // 4 + n] = (src[s, :cnt[s] * 1152] if nch[s] == 2 else src[s, :cnt[s] * 1152, 0]).reshape(-1)
            b.frame_counts(cnt)
            b.pcm_segments(off, total)
            fed_slots = [s for s in range(S) if cnt[s]]
            arr = (C.c_int * len(fed_slots))(*fed_slots)
            down = 0
            t0 = time.perf_counter()
            if v == "rows":
                if L.hx_batch_encode_f32_host_crc(b.h, pcm.ctypes.data, CH, out.ctypes.data, stride, nb.ctypes.data, stats.ctypes.data, crc.ctypes.data) != 0:
                    raise RuntimeError(api.last_error())
                t1 = time.perf_counter()
                if L.hx_batch_ledger_read(b.h, arr, len(fed_slots), led) != 0:
                    raise RuntimeError(api.last_error())
                t2 = time.perf_counter()
                for e, s in enumerate(fed_slots):
                    files[v][s] += out[s, :led[e].call_bytes].tobytes()
                    fed[v][s], ended[v][s] = led[e].fed, bool(led[e].ended)
                t3 = time.perf_counter()
                down = len(fed_slots) * stride + 4 * S + stats.nbytes + crc.nbytes + len(fed_slots) * C.sizeof(api.Ledger)
            elif v == "many":
                if L.hx_batch_encode_f32_host_files(b.h, pcm.ctypes.data, CH) != 0:
                    raise RuntimeError(api.last_error())
                t1 = time.perf_counter()
                if L.hx_batch_ledger_poll(b.h, brief) != 0:
                    raise RuntimeError(api.last_error())
                t2 = time.perf_counter()
                down = 4 + 32 * S
                for s in fed_slots:
                    fed[v][s], ended[v][s] = brief[s].fed, bool(brief[s].ended)
                over = [s for s in fed_slots if ended[v][s]]
                held = 0.0
                if over:
                    n = len(over)
                    need = sum((head[v][s] + brief[s].image_bytes + 15) & ~15 for s in over)
                    if need > many_buf.nbytes:          # (the page-locked buffer grows outside the clock)
                        h0 = time.perf_counter()
                        many_buf = pinned(L, need + need // 2, np.uint8)
                        held = time.perf_counter() - h0
                    arr_over = (C.c_int * n)(*over)
                    if L.hx_batch_file_tags(b.h, arr_over, (api.FileTag * n)(*[tags[s] for s in over]), n, None) != 0:
                        raise RuntimeError(api.last_error())
                    if L.hx_batch_file_fetch_many(b.h, arr_over, n, many_buf.ctypes.data, many_buf.nbytes, many_off.ctypes.data) != need:
                        raise RuntimeError(api.last_error())
                    for e, s in enumerate(over):
                        seg = many_buf[many_off[e]:many_off[e] + head[v][s] + brief[s].image_bytes]
                        assert seg[0] == 0xFF and bytes(seg[4 + (32 if nch[s] == 2 else 17):][:4]) == b"Xing"
                        files[v][s] = bytearray(seg[head[v][s]:].tobytes())
                    down += 8 * (n + 1) + need
                t3 = time.perf_counter() - held
                nmany += len(over) if step else 0
            else:
                if L.hx_batch_encode_f32_host_files(b.h, pcm.ctypes.data, CH) != 0:
                    raise RuntimeError(api.last_error())
                t1 = time.perf_counter()
                if L.hx_batch_ledger_poll(b.h, brief) != 0:
                    raise RuntimeError(api.last_error())
                t2 = time.perf_counter()
                down = 4 + 32 * S
                for s in fed_slots:
                    fed[v][s], ended[v][s] = brief[s].fed, bool(brief[s].ended)
                over = [s for s in fed_slots if ended[v][s]]
                if over and L.hx_batch_ledger_read(b.h, (C.c_int * len(over))(*over), len(over), led) != 0:      # (the seek points: one read for all)
                    raise RuntimeError(api.last_error())
                for s in over:
                    n = int(L.hx_batch_file_fetch(b.h, s, fetch_buf.ctypes.data, cap))
                    if n < 0:
                        raise RuntimeError(api.last_error())
                    files[v][s] = bytearray(fetch_buf[HEAD:n].tobytes())
                    down += C.sizeof(api.Ledger) + 8 + n - HEAD
                t3 = time.perf_counter()
                nfetched += len(over) if step else 0
            over = [s for s in fed_slots if ended[v][s]]
            for s in over:
                done[v].append((s, bytes(files[v][s])))
                files[v][s] = bytearray()
            if over:
                begin(v, over)
            if step:
                t[v]["call"].append(t1 - t0)
                t[v]["records"].append(t2 - t1)
                t[v]["files"].append(t3 - t2)
                link[v]["up"].append(int(total))
                link[v]["down"].append(int(down))
    same = done["rows"] == done["images"] == done["many"]
    for b in batch.values():
        assert b.status() == 0
    ms = lambda x: round(1e3 * float(np.median(x)), 3)
    res = {"streams": S, "frames_per_call": CH, "calls": args.steps, "build_id": api.build_id(), "image_cap": int(cap),
           "files_finished": len(done["rows"]), "files_identical": bool(same)}
    for v in batch:
        tot = [a + b_ + c for a, b_, c in zip(t[v]["call"], t[v]["records"], t[v]["files"])]
        res[v] = {"ms_per_call": ms(tot), "ms_call_alone": ms(t[v]["call"]), "ms_records": ms(t[v]["records"]),
                  "ms_append_or_fetch": ms(t[v]["files"]), "ms_each": [round(1e3 * x, 2) for x in tot],
                  "bytes_up_per_call": int(np.mean(link[v]["up"])), "bytes_down_per_call": int(np.mean(link[v]["down"]))}
    res["images"]["files_fetched"] = nfetched
    res["many"]["files_fetched"] = nmany
    res["many"]["us_per_file_fetched"] = round(1e6 * float(np.sum(t["many"]["files"])) / max(1, nmany), 1)
    # what a call does for its n finished files, by the entry points' contracts (include/hmp3_amd.h)
    res["images"]["per_finished_file"] = {"launches": "1 record gather per call", "copies": "2 per file (length word, bytes) + 1 record copy per call"}
    res["many"]["per_finished_file"] = {"launches": "3 per call (k_file_tag, k_file_off, k_file_gather)", "copies": "2 per call (offsets, image) + 2 list uploads"}
    res["images"]["us_per_file_fetched"] = round(1e6 * float(np.sum(t["images"]["files"])) / max(1, nfetched), 1)
    res["file_frames"] = args.file_frames
    res["file_bytes_per_call"] = int(sum(len(d) for _, d in done["rows"]) / max(1, args.steps))
    for b in batch.values():
        b.close()
    while PINNED:
        L.hx_pinned_free(PINNED.pop())
    return res, same


if __name__ == "__main__":
    main()
