// hmp3amd - file front end over libhmp3amd.
//   hmp3amd <input.wav|-> <output.mp3|-> [flags]                 one file: a bounded regular file as a batch of one, a pipe or
//                                                                 a very large file frame by frame (hx_enc_* API)
//   hmp3amd -batch in1.wav out1.mp3 in2.wav out2.mp3 ... [flags]  many files at once (hx_multi_* API): mono and stereo, MPEG-1
//                                                                 and MPEG-2 rates, any stereo mode together (hx_multi_create_any);
//                                                                 files at any rate and -A go through a converting batch
//   ... -slots<n>                                                 the files of -batch through n slots of one batch: a file is
//                                                                 read when a slot is free and written when its drain ends
// Same flags, encode loop and output files as the reference CLI (reference
// test/tomp3.cpp:336-602 main, :645-1088 ff_encode): Xing/Info tag frame first, audio frames, four
// frames of silence behind the input, drain until every submitted frame is out, then the tag is
// completed in place.  Accepted: RIFF/WAVE, mono or stereo, 8/16/24/32-bit PCM or 32-bit float,
// 8 - 48 kHz (rates other than 16 / 22.05 / 24 / 32 / 44.1 / 48 kHz, or -A, go through the sample-rate
// converter first, as in the reference); everything else fails like an unsupported file.
// Batch mode encodes all files as one batch of streams (either channel count, either MPEG version, same flags) and
// reproduces per file exactly what the single-file loop writes.  Containers: RIFF, RIFX, RF64 / BW64, Wave64.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hmp3_amd.h"

namespace {

struct WavInfo { int channels = 0, rate = 0, bits = 0, type = 0, bigendian = 0; uint64_t data_bytes = 0; };
struct Options { HX_E_CONTROL ec; int xing_flag = 3 | 0x40, ignore_length = 0, mpeg_select = 0, ec_display = 0, ngpus = 0, nslots = 0; };

// a header field of n bytes in the file's byte order
uint64_t field(const unsigned char *p, int n, int be)
{
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint64_t) p[be ? n - 1 - i : i] << (8 * i);
    return v;
}

bool read_exact(FILE *f, void *dst, size_t n) { return fread(dst, 1, n, f) == n; }
bool skip_bytes(FILE *f, uint64_t n)
{
    unsigned char tmp[4096];
    while (n) { size_t k = n < sizeof(tmp) ? (size_t) n : sizeof(tmp); if (fread(tmp, 1, k, f) != k) return false; n -= k; }
    return true;
}

// Walk to the start of the audio data (works on pipes: no seeking).  Containers and rules as the
// reference's pcmhead_file (pcmhpm.c:203-429): RIFF, RIFX (big-endian fields and samples), RF64 / BW64
// (64-bit data size in the ds64 chunk) and Sony Wave64 (GUID chunks, sizes include the 24-byte chunk
// header, bodies padded to 8).  bits = 8 * block align / channels, or the valid-bits field of a
// WAVE_FORMAT_EXTENSIBLE header; an odd data size is rounded up to even (the pad byte is read as audio).
bool wav_header(FILE *f, WavInfo *w)
{
    static const unsigned char w64_riff[16] = {0x72, 0x69, 0x66, 0x66, 0x2E, 0x91, 0xCF, 0x11, 0xA5, 0xD6, 0x28, 0xDB, 0x04, 0xC1, 0x00, 0x00};
    static const unsigned char w64_tail[12] = {0xF3, 0xAC, 0xD3, 0x11, 0x8C, 0xD1, 0x00, 0xC0, 0x4F, 0x8E, 0xDB, 0x8A};   // wave / fmt / data GUIDs after their four letters
    static const unsigned char ext_tail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};
    unsigned char h[24];
    bool w64 = false, rf64 = false;
    uint64_t ds64_data = 0;
    if (!read_exact(f, h, 8)) return false;
    if (!memcmp(h, "RIFF", 4)) { }
    else if (!memcmp(h, "RF64", 4) || !memcmp(h, "BW64", 4)) rf64 = true;
    else if (!memcmp(h, "RIFX", 4)) w->bigendian = 1;
    else {
        if (!read_exact(f, h + 8, 16) || memcmp(h, w64_riff, 16)) return false;
        w64 = true;
    }
    const int be = w->bigendian;
    if (w64) { if (!read_exact(f, h, 16) || memcmp(h, "wave", 4) || memcmp(h + 4, w64_tail, 12)) return false; }
    else if (!read_exact(f, h, 4) || memcmp(h, "WAVE", 4)) return false;
    if (rf64) {
        unsigned char d[36];
        if (!read_exact(f, d, 36) || memcmp(d, "ds64", 4)) return false;
        uint64_t size = field(d + 4, 4, be) + 8;
        if (size < 36) return false;
        if (size & 1) size++;
        ds64_data = field(d + 16, 8, be);
        if (!skip_bytes(f, size - 36)) return false;
    }
    bool have_fmt = false;
    for (;;) {
        uint64_t n;     // body bytes to consume, padding included
        bool is_fmt, is_data;
        if (w64) {
            if (!read_exact(f, h, 24)) return false;
            n = field(h + 16, 8, 0);
            if (n < 24) return false;
            n -= 24;
            if (n % 8) n += 8 - n % 8;
            const bool ours = !memcmp(h + 4, w64_tail, 12);
            is_fmt = ours && !memcmp(h, "fmt ", 4);
            is_data = ours && !memcmp(h, "data", 4);
        } else {
            if (!read_exact(f, h, 8)) return false;
            n = field(h + 4, 4, be);
            is_fmt = !memcmp(h, "fmt ", 4);
            is_data = !memcmp(h, "data", 4);
            if ((n & 1) && n != 0xFFFFFFFFu) n++;
            if (is_data && rf64 && n == 0xFFFFFFFFu) { n = ds64_data; if (n & 1) n++; }
        }
        if (is_fmt && !have_fmt) {
            if (n < 16 || n >= (1u << 31)) return false;
            std::vector<unsigned char> b((size_t) n);
            if (!read_exact(f, b.data(), b.size())) return false;
            w->type = (int) field(&b[0], 2, be);
            w->channels = (int) field(&b[2], 2, be);
            w->rate = (int) field(&b[4], 4, be);
            w->bits = (int) field(&b[14], 2, be);
            if (w->channels > 0) w->bits = 8 * ((int) field(&b[12], 2, be) / w->channels);
            if (w->type == 65534 && n >= 18 + 22 && field(&b[16], 2, be) >= 22) {      // WAVE_FORMAT_EXTENSIBLE
                if (!memcmp(&b[24 + 2], ext_tail, 14)) w->type = (int) field(&b[24], 2, be);
                w->bits = (int) field(&b[18], 2, be);
            }
            have_fmt = true;
        } else if (is_data && have_fmt) {
            w->data_bytes = n;
            return true;
        } else {
            if (n >= (1u << 31)) return false;
            if (!skip_bytes(f, n)) return false;
        }
    }
}

void usage()
{
    fprintf(stderr,
            "\n hmp3amd <input.wav|-> <output.mp3|-> [flags]"
            "\n hmp3amd -batch in1.wav out1.mp3 in2.wav out2.mp3 ... [flags]"
            "\n   -Bn  kbps per channel (CBR)      -Vn  VBR quality 0..150 (default 50)"
            "\n   -Mn  0 stereo, 1 joint stereo, 3 mono      -Fn  low-pass Hz      -HFn high-frequency mode"
            "\n   -SBTn short-block threshold      -S1  DC blocker       -Xn  0 no tag, 1 Xing, 2/3 + TOC, default + info"
            "\n   -Cn -On copyright / original bits   -Ln VBR bitrate cap   -Tn -TXn tuning   -IL ignore the WAV length field"
            "\n   -An  encode rate: 0 track the input (default), 1 an MPEG-1 rate, 2 an MPEG-2 rate, else that rate in Hz"
            "\n   -EC  print the encoder settings in use    -D  no progress display    -Gn  GPUs used by -batch (default all)"
            "\n   -slotsn  -batch through n slots: at most n files in memory, a slot takes the next file when its file is done\n");
}

// one input file, read and checked
struct Input {
    WavInfo wi;
    std::vector<unsigned char> data;    // the audio bytes; pad() appends the silence the encode loop runs into
    uint64_t audio_bytes = 0;
    int frame_in = 0, mono_convert = 0, is_float = 0;
    HX_E_CONTROL ec;                    // as given to the encoder
    HX_E_CONTROL ec_used;               // as reported back (settings in use)
    HX_MPEG_HEAD head;
    size_t size = 0;                    // bytes the encode loop may consume: audio + 4 x init_bytes of zero bytes
    // The reference refills a large buffer and, when it meets the end of the data, appends 4 x bytes_in_init
    // zero bytes (tomp3.cpp:925-934); a call is made while at least bytes_in_init bytes are left (:904-941).
    // A linear buffer of (data ++ zeros) gives the same sequence of calls.  The converter may stage more
    // than it consumes, so some slack follows.
    void pad(int init_bytes) { size = audio_bytes + 4 * (size_t) init_bytes; data.resize(size + (1 << 17), 0); }
};

// open the input, parse and check its header; on success *fp is positioned at the first audio byte and
// *indatasize is the number of audio bytes to read (UINT64_MAX: until the end of the file)
// (announce: print the header line - a file of -slots is opened twice, for its header and for its audio)
bool open_input(const char *path, const Options &opt, Input *in, FILE **fp, uint64_t *indatasize_out, bool announce = true)
{
    FILE *f = strcmp(path, "-") ? fopen(path, "rb") : stdin;
    if (!f) { fprintf(stderr, "\n CANNOT_OPEN_INPUT_FILE %s\n", path); return false; }
    *fp = f;
    const int ignore_length = opt.ignore_length || f == stdin;
    if (!wav_header(f, &in->wi)) { fprintf(stderr, "\n UNRECOGNIZED PCM FILE TYPE\n"); return false; }
    const WavInfo &wi = in->wi;
    // a data size of 0xFFFFFFFF means "until the end of the file" (tomp3.cpp:751-768)
    const uint64_t indatasize = (ignore_length || wi.data_bytes == 0xFFFFFFFFu) ? UINT64_MAX : wi.data_bytes;
    if (indatasize == 0) { fprintf(stderr, "\n INPUT FILE CONTAINS NO AUDIO\n"); return false; }
    *indatasize_out = indatasize;
    if (announce) fprintf(stderr, "\n pcm file:  channels = %d  bits = %d,  rate = %d  type = %d", wi.channels, wi.bits, wi.rate, wi.type);
    in->is_float = wi.type == 3;
    if ((wi.channels != 1 && wi.channels != 2) ||
        !((wi.type == 1 && (wi.bits == 8 || wi.bits == 16 || wi.bits == 24 || wi.bits == 32)) || (in->is_float && wi.bits == 32)) ||
        wi.rate < 8000 || wi.rate > 48000) {
        fprintf(stderr, "\n UNSUPPORTED PCM FILE TYPE\n Mono or stereo, 8/16/24/32-bit PCM or 32-bit float, 8000 Hz - 48000 Hz.\n");
        return false;
    }
    in->ec = opt.ec;
    if (in->ec.mode < 0) in->ec.mode = 0;
    in->mono_convert = in->ec.mode == 3;        // -M3: encode one channel (tomp3.cpp:562-563)
    if (wi.channels == 1) in->ec.mode = 3;
    else if (in->ec.mode == 3) in->ec.mode = 1;
    in->ec.samprate = wi.rate;
    in->frame_in = 1152 * wi.channels * (wi.bits / 8);
    return true;
}

// cvt_to_pcm (pcmhpm.c:454-484): big-endian samples to host byte order
void to_host_order(const WavInfo &wi, unsigned char *p, size_t nbytes)
{
    if (!wi.bigendian || wi.bits <= 8) return;
    const size_t bs = (size_t) wi.bits / 8, ns = nbytes / bs;
    for (size_t i = 0; i < ns; i++) std::reverse(p + i * bs, p + (i + 1) * bs);
}

// a whole input in memory (regular files of the batched routes)
bool load_input(const char *path, const Options &opt, Input *in, bool announce = true)
{
    FILE *f = nullptr;
    uint64_t indatasize = 0;
    *in = Input();
    if (!open_input(path, opt, in, &f, &indatasize, announce)) { if (f && f != stdin) fclose(f); return false; }
    const WavInfo &wi = in->wi;
    std::vector<unsigned char> chunk(1 << 20);
    while (in->data.size() < indatasize) {
        size_t want = chunk.size();
        if (in->data.size() + want > indatasize) want = (size_t) (indatasize - in->data.size());
        const size_t got = fread(chunk.data(), 1, want, f);
        in->data.insert(in->data.end(), chunk.begin(), chunk.begin() + got);
        if (got < want) break;
    }
    to_host_order(wi, in->data.data(), in->data.size());
    in->audio_bytes = in->data.size();
    if (f != stdin) fclose(f);
    return true;
}

// the tag frame, its running seek table and the MusicCRC of one output file (tomp3.cpp:871-896, :976-984, :1055-1072)
struct Tagger {
    hx_xing *xg = hx_xing_create();
    std::vector<unsigned char> tag = std::vector<unsigned char>(2048, 0);
    int head_flags = 0, head_bytes = 0, vbr_scale = -1, toc_counter = 0;
    unsigned crc = 0;
    ~Tagger() { hx_xing_destroy(xg); }
    void begin(const Input &in, int xing_flag)
    {
        if (xing_flag) head_flags = 1 | 2 | 8;
        if (xing_flag & 2) head_flags |= 4 | 0x40;
        if (!xing_flag) return;
        if (in.ec_used.vbr_flag) vbr_scale = in.ec_used.vbr_mnr;
        head_bytes = hx_xing_header(xg, in.ec_used.samprate, in.head.mode, in.ec_used.cr_bit, in.ec_used.original, head_flags, 0, 0,
                                    vbr_scale, nullptr, tag.data(), nullptr, nullptr, in.ec_used.bitrate * in.wi.channels);
    }
    void after_call(unsigned frames_out, unsigned bytes_out)    // once per input frame of the main loop
    {
        if ((head_flags & 4) && --toc_counter <= 0) toc_counter = hx_xing_toc(xg, (int) frames_out + 1, (int) bytes_out + head_bytes);
    }
    void bytes(const unsigned char *p, int n) { crc = hx_xing_update_crc((unsigned short) crc, p, n); }
    // what begin() and finish() pass, for the tag frame that the GPU builds from the file's record (hx_multi_file_tags); a
    // file without a tag: all zero, which describes no frame
    HX_FILE_TAG describe(const Input &in) const
    {
        HX_FILE_TAG t = {};
        if (!head_bytes) return t;
        t.samprate = in.ec_used.samprate; t.h_mode = in.head.mode; t.cr_bit = in.ec_used.cr_bit; t.original_bit = in.ec_used.original;
        t.flags = head_flags; t.kbps = in.ec_used.bitrate * in.wi.channels; t.vbr_scale = vbr_scale;
        t.lowpass = (unsigned) in.ec_used.freq_limit; t.in_samplerate = (unsigned) in.wi.rate;
        t.samples_audio = in.audio_bytes / (uint64_t) (in.wi.channels * (in.wi.bits / 8));
        return t;
    }
    void finish(const Input &in, unsigned frames, uint64_t out_bytes)
    {
        const uint64_t samples_audio = in.audio_bytes / (uint64_t) (in.wi.channels * (in.wi.bits / 8));
        hx_xing_update_info(xg, frames, (int) out_bytes, vbr_scale, nullptr, tag.data(), nullptr, nullptr, samples_audio,
                            (unsigned) out_bytes, (unsigned) in.ec_used.freq_limit, (unsigned) in.wi.rate, (unsigned) in.ec_used.samprate,
                            (unsigned short) crc);
    }
};

// One file on its way through a batch: its input, what the batch takes for it, the calls of the single-file loop on it and
// what its stream has produced so far.
struct Job {
    Input in;
    HX_E_CONTROL ctl;                   // the control the batch is created with for the file (converting route: the source's)
    HX_SOURCE src = {0, 0, 0, 0};
    int nch = 0;                        // channels the file encodes to (mono, or stereo summed to mono: 1)
    size_t nc = 0;                      // calls of the single-file loop on the file's input (the drain follows them)
    std::vector<long long> start;       // converting route: where each of them starts in the file's bytes
    std::vector<unsigned char> stream;  // the file's audio bytes; whole: the output file as fetched from its file image, the tag frame
    bool whole = false;                 // (built on the GPU, k_file_tag) in front
    size_t est_calls = 0;               // -slots: an upper bound of nc from the header alone (0: the header does not say)
    HX_LEDGER led = {};                 // the file's record as last read from the batch's ledger: calls fed, frames / bytes out so far,
                                        // the MusicCRC of those bytes, the seek points; ended: the drain has ended, it takes no more frames
};
int encode_jobs(std::vector<Job> &jobs, const std::vector<const char *> &files, const Options &opt, bool loaded);

bool mpeg_rate(int r) { return r == 32000 || r == 44100 || r == 48000 || r == 16000 || r == 22050 || r == 24000; }
// The reference appends the four calls' worth of silence only if it fits a limit derived from its input buffer
// (128 frames of stereo floats) and a per-format factor (tomp3.cpp:268,802,925; pcmhpm.c:450): with 32-bit
// samples and a down-conversion by more than 1.14 (24-bit: 2.03) it never does, and the tail of the input that
// is shorter than one call's need is dropped.  Found by tools/fuzz_cli.py.
bool pad_fits(const WavInfo &wi, int init_bytes)
{
    const uint64_t ref_bufbytes = 128ull * sizeof(float) * 2304, fmt_factor = (uint64_t) wi.channels * (uint64_t) ((wi.bits * 7) / 8);
    return fmt_factor != 0 && (((ref_bufbytes << 1) / fmt_factor) & ~1ull) > 4ull * (uint64_t) init_bytes;
}

// the file goes through the sample-rate converter: its rate is no MPEG rate, or -A asks for another one
bool needs_conversion(const Input &in, const Options &opt) { return opt.mpeg_select || !mpeg_rate(in.wi.rate); }

// The calls the frame-by-frame loop (encode_streaming) makes on a file that goes through the converter, computed on the host:
// over the window audio ++ 4 x init_bytes zero bytes (where pad_fits allows them) one call while at least init_bytes are left,
// each consuming what the converter's schedule says.  Sets in->size to the window's size and appends the zero bytes and the
// slack to in->data; start: the byte position of every call's input; ec_enc: the control the encoder behind the converter
// runs.  Returns the number of calls, -1 if the converter rejects the source (hx_last_error).
long long converter_calls(Input &in, const Options &opt, std::vector<long long> *start, HX_E_CONTROL *ec_enc)
{
    const HX_SOURCE src = {in.wi.bits, in.is_float, opt.mpeg_select, in.mono_convert};
    HX_E_CONTROL ec2;
    const int init_bytes = hx_src_encode_control(&in.ec, &src, &ec2);
    if (!init_bytes) return -1;
    if (ec_enc) *ec_enc = ec2;
    hx_src *conv = hx_src_create();
    int cutoff = 0;
    if (!hx_src_init(conv, in.wi.rate, in.wi.channels, in.wi.bits, in.is_float, ec2.samprate, ec2.mode == 3 ? 1 : 2, &cutoff)) { hx_src_destroy(conv); return -1; }
    in.size = (size_t) in.audio_bytes + (pad_fits(in.wi, init_bytes) ? 4 * (size_t) init_bytes : 0);
    in.data.resize(in.size + (1 << 17), 0);
    long long calls = 0, pos = 0, nbytes = 0;
    while ((long long) in.size - pos >= init_bytes) {
        if (start) start->push_back(pos);
        hx_src_schedule(conv, calls++, 1, &nbytes);
        pos += nbytes;
    }
    hx_src_destroy(conv);
    return calls;
}

// tomp3.cpp:1169-1196 (-EC)
void print_ec(const HX_E_CONTROL *ec)
{
    fprintf(stderr, "\n-------------------------------------------------------------------------------");
    fprintf(stderr, "\nec->layer =         %d\t\t\tec->mode =          %d", ec->layer, ec->mode);
    fprintf(stderr, "\nec->bitrate =       %d\t\t\tec->samprate =      %d", ec->bitrate, ec->samprate);
    fprintf(stderr, "\nec->nsbstereo =     %d\t\t\tec->freq_limit =    %d", ec->nsbstereo, ec->freq_limit);
    fprintf(stderr, "\nec->filter_select = %d\t\t\tec->nsb_limit =     %d", ec->filter_select, ec->nsb_limit);
    fprintf(stderr, "\nec->cr_bit =        %d\t\t\tec->original =      %d", ec->cr_bit, ec->original);
    fprintf(stderr, "\nec->hf_flag =       %d\t\t\tec->vbr_flag =      %d", ec->hf_flag, ec->vbr_flag);
    fprintf(stderr, "\nec->vbr_mnr =       %d\t\t\tec->vbr_br_limit =  %d", ec->vbr_mnr, ec->vbr_br_limit);
    fprintf(stderr, "\nec->sparse_scale =  %d\t\t\tec->chan_add_f0 =   %d", ec->sparse_scale, ec->chan_add_f0);
    fprintf(stderr, "\nec->vbr_delta_mnr = %d\t\t\tec->chan_add_f1 =   %d", ec->vbr_delta_mnr, ec->chan_add_f1);
    fprintf(stderr, "\nec->quick =         %d\t\t\tec->cpu_select =    %d", ec->quick, ec->cpu_select);
    fprintf(stderr, "\nec->test1 =         %d\t\t\tec->short_block_threshold = %d", ec->test1, ec->short_block_threshold);
    fprintf(stderr, "\n-------------------------------------------------------------------------------");
}

// regular files up to this size take the batched route (whole file in memory); larger ones and pipes stream
const uint64_t kBatchRouteMaxBytes = 1ull << 30;

bool regular_file_size(const char *path, uint64_t *size)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fseek(f, 0, SEEK_END) == 0;
    const long n = ok ? ftell(f) : -1;
    fclose(f);
    if (n < 0) return false;
    *size = (uint64_t) n;
    return true;
}

// The reference's loop (tomp3.cpp:897-1050) with its bounded buffers: the input is read in pieces into a
// sliding window, every call's bytes are written as they arrive, the tag is completed by seeking back at the
// end.  Memory does not grow with the length of the input, so an unbounded pipe works.
int encode_streaming(const char *fin, const char *fout, const Options &opt)
{
    Input in;
    FILE *fi = nullptr;
    uint64_t indatasize = 0;
    if (!open_input(fin, opt, &in, &fi, &indatasize)) { if (fi && fi != stdin) fclose(fi); return 1; }
    int rc = 1;
    hx_enc *enc = hx_enc_create(0);
    FILE *out = nullptr;
    do {
        // bytes a call needs in the buffer (more than it consumes); with a sample-rate conversion a call consumes a varying amount
        const int init_bytes = enc ? hx_enc_MP3_audio_encode_init(enc, &in.ec, in.wi.bits, in.is_float, opt.mpeg_select, in.mono_convert) : 0;
        if (!init_bytes) { fprintf(stderr, "\n ENCODER INIT FAIL: %s\n", hx_last_error()); break; }
        out = strcmp(fout, "-") ? fopen(fout, "w+b") : stdout;
        if (!out) { fprintf(stderr, "\n CANNOT CREATE OUTPUT FILE\n"); break; }
        char info[128];
        hx_enc_info_string(enc, info);
        fprintf(stderr, "\n %s\n", info);
        hx_enc_info_ec(enc, &in.ec_used);       // the settings actually in use
        hx_enc_info_head(enc, &in.head);
        if (opt.ec_display) print_ec(&in.ec_used);
        Tagger tg;
        tg.begin(in, opt.xing_flag);
        uint64_t out_bytes = tg.head_bytes;
        if (tg.head_bytes && fwrite(tg.tag.data(), 1, tg.head_bytes, out) != (size_t) tg.head_bytes) { fprintf(stderr, "\n FILE WRITE ERROR\n"); break; }

        // window over (audio ++ 4 x init_bytes zero bytes): a call is made while at least init_bytes are
        // left (tomp3.cpp:904-941); the converter may stage more than it consumes, hence the slack
        const size_t slack = 1 << 17, piece = 1 << 20;
        std::vector<unsigned char> win(piece + (size_t) init_bytes + slack, 0), bs(128 * 1024), zero((size_t) 4 * init_bytes + slack, 0);
        size_t lo = 0, hi = 0;                  // valid bytes of the window: [lo, hi)
        uint64_t audio = 0, zeros_left = pad_fits(in.wi, init_bytes) ? 4ull * (uint64_t) init_bytes : 0;      // (the silence behind the input)
        bool eof = false, werr = false;
        unsigned frames_expected = 0;
        auto emit = [&](const HX_IN_OUT &x) {
            if (x.out_bytes && fwrite(bs.data(), 1, x.out_bytes, out) != (size_t) x.out_bytes) werr = true;
            tg.bytes(bs.data(), x.out_bytes);
            out_bytes += x.out_bytes;
        };
        for (;;) {
            if (hi - lo < (size_t) init_bytes && !(eof && zeros_left == 0)) {      // refill
                memmove(win.data(), win.data() + lo, hi - lo);
                hi -= lo; lo = 0;
                while (hi + 8 <= piece && !(eof && zeros_left == 0)) {     // (less than a sample's room left counts as full)
                    if (!eof) {
                        size_t want = piece - hi;
                        if ((uint64_t) want > indatasize - audio) want = (size_t) (indatasize - audio);
                        else {      // every piece ends on a sample boundary of the data (24-bit samples do not divide 1 MiB), so
                                    // that the byte swap of big-endian input never tears a sample; the data's torn tail is padding
                            const size_t bsz = (size_t) std::max(in.wi.bits / 8, 1), over = (size_t) ((audio + want) % bsz);
                            if (want > over) want -= over;
                        }
                        const size_t got = want ? fread(win.data() + hi, 1, want, fi) : 0;
                        to_host_order(in.wi, win.data() + hi, got);
                        hi += got; audio += got;
                        if (got < want || audio >= indatasize) eof = true;
                    } else {
                        const size_t z = (size_t) std::min<uint64_t>(zeros_left, piece - hi);
                        memset(win.data() + hi, 0, z);
                        hi += z; zeros_left -= z;
                    }
                }
                memset(win.data() + hi, 0, win.size() - hi);
            }
            if (hi - lo < (size_t) init_bytes) break;
            const HX_IN_OUT x = hx_enc_MP3_audio_encode(enc, win.data() + lo, bs.data());
            emit(x);
            lo += (size_t) x.in_bytes;
            frames_expected++;
            const HX_INT_PAIR fb = hx_enc_get_frames_bytes(enc);
            tg.after_call((unsigned) fb.a, (unsigned) fb.b);
            if (werr) break;
        }
        in.audio_bytes = audio;
        if (in.ec_used.samprate < 32000) frames_expected *= 2;                          // MPEG-2: two frames per call (tomp3.cpp:1022)
        // drain, tomp3.cpp:1020-1036 (bounded: an encoder that stopped emitting - a failed device call - must not hang the tool)
        for (unsigned spare = frames_expected + 64; !werr && hx_enc_get_frames(enc) < frames_expected && spare; spare--)
            emit(hx_enc_MP3_audio_encode(enc, zero.data(), bs.data()));
        if (hx_enc_get_frames(enc) < frames_expected) { fprintf(stderr, "\n ENCODER FAIL: %s\n", hx_last_error()); break; }
        if (werr) { fprintf(stderr, "\n FILE WRITE ERROR\n"); break; }
        const unsigned frames = hx_enc_get_frames(enc);
        if (opt.xing_flag) {
            tg.finish(in, frames, out_bytes);
            if (out == stdout || fseek(out, 0, SEEK_SET) != 0) fprintf(stderr, "\n OUTPUT IS NOT SEEKABLE: TAG FRAME LEFT WITHOUT TOTALS");
            else fwrite(tg.tag.data(), 1, tg.head_bytes, out);
        }
        fprintf(stderr, "\n %u frames, %llu bytes, %.2f kbps\n", frames, (unsigned long long) out_bytes, hx_enc_get_bitrate_float(enc));
        rc = frames == 0 ? 1 : 0;
    } while (0);
    if (out && out != stdout) fclose(out);
    if (fi && fi != stdin) fclose(fi);
    hx_enc_destroy(enc);
    return rc;
}

int encode_one_file(const char *fin, const char *fout, const Options &opt)
{
    // A regular file of bounded size with a seekable output goes through the batched API as a batch of one (96
    // frames per call instead of one), which writes exactly what the frame-by-frame loop writes - a file that needs a
    // rate conversion (its rate, or -A) through a converting batch.  Pipes and very large files stream frame by frame,
    // and so does an input too short for one converter call, which that loop answers with a file of the tag alone.
    uint64_t fsize = 0;
    if (strcmp(fin, "-") && strcmp(fout, "-") && regular_file_size(fin, &fsize) && fsize <= kBatchRouteMaxBytes) {
        std::vector<Job> one(1);
        if (!load_input(fin, opt, &one[0].in)) return 1;
        if (!needs_conversion(one[0].in, opt) || converter_calls(one[0].in, opt, nullptr, nullptr) > 0) return encode_jobs(one, {fin, fout}, opt, true);
    }
    return encode_streaming(fin, fout, opt);
}

// samples of one input frame as fp32 at int16 scale, the way Csrc::sr_convert / src_filter_to_mono_case0
// produce them (srcc.cpp:804-836, srccf.cpp:458-468)
// what hx_enc_MP3_audio_encode_init returns when source and encode rate are equal: 1153 sample frames
int init_bytes_same_rate(const Input &in) { return 1153 * in.wi.channels * (in.wi.bits / 8); }
// calls of the single-file loop: one per frame_in bytes while at least init_bytes are left
size_t ncalls(const Input &in)
{
    const size_t init = (size_t) init_bytes_same_rate(in);
    return in.size >= init ? (in.size - init) / (size_t) in.frame_in + 1 : 0;
}

void frame_to_float(const Input &in, const unsigned char *src, float *dst)
{
    const int ns = 1152 * in.wi.channels;
    if (in.wi.bits == 32 && in.is_float) { const float *f = (const float *) src; for (int i = 0; i < ns; i++) dst[i] = f[i] * 32768.0f; }
    else if (in.wi.bits == 32) { const int *s = (const int *) src; for (int i = 0; i < ns; i++) dst[i] = (float) (s[i] / 65536.0f); }
    else if (in.wi.bits == 24)
        for (int i = 0; i < ns; i++) {
            const unsigned char *b = src + 3 * i;
            const int s = (int) (((unsigned) b[2] << 24) | ((unsigned) b[1] << 16) | ((unsigned) b[0] << 8)) >> 8;
            dst[i] = (float) ((float) s / 256.0f);
        }
    else if (in.wi.bits == 16) { const int16_t *s = (const int16_t *) src; for (int i = 0; i < ns; i++) dst[i] = (float) s[i]; }
    else for (int i = 0; i < ns; i++) dst[i] = (((float) src[i]) - 128.0f) * (256.0f);
    if (in.wi.channels == 2 && in.mono_convert)
        for (int i = 0; i < 1152; i++) dst[i] = (float) ((dst[2 * i] + dst[2 * i + 1]) * 0.5);
}

// Without -slots every file is read whole before the first call and has a slot of its own.  With -slots<n> only the headers
// are read here: the files go through min(n, files) slots, and a file's audio is read when it gets one.
int encode_batch(const std::vector<const char *> &files, const Options &opt)
{
    const int S = (int) files.size() / 2;
    std::vector<Job> jobs(S);
    for (int i = 0; i < S; i++) {
        if (opt.nslots <= 0) { if (!load_input(files[2 * i], opt, &jobs[i].in)) return 1; continue; }
        FILE *f = nullptr;
        uint64_t indatasize = 0;
        const bool ok = open_input(files[2 * i], opt, &jobs[i].in, &f, &indatasize);
        if (f && f != stdin) fclose(f);
        if (!ok) return 1;
        // what the file's image must hold at most: its sample frames at the highest rate an encoder runs at, in blocks of 1152,
        // and the calls on the zero bytes behind them
        const WavInfo &wi = jobs[i].in.wi;
        if (indatasize != UINT64_MAX)
            jobs[i].est_calls = (size_t) (indatasize / (uint64_t) (wi.channels * (wi.bits / 8)) * 48000 / (uint64_t) wi.rate / 1152) + 16;
    }
    return encode_jobs(jobs, files, opt, opt.nslots <= 0);
}

// the calls of the single-file loop on a file whose audio is in memory (conv: through the converter); false: no such call
bool job_calls(Job &j, const char *name, const Options &opt, bool conv)
{
    if (!conv) { j.in.pad(init_bytes_same_rate(j.in)); j.nc = ncalls(j.in); return true; }
    const long long n = converter_calls(j.in, opt, &j.start, nullptr);
    if (n < 0) { fprintf(stderr, "\n ENCODER INIT FAIL (%s): %s\n", name, hx_last_error()); return false; }
    if (n == 0) { fprintf(stderr, "\n %s is shorter than one call of its converter\n", name); return false; }
    j.nc = (size_t) n;
    return true;
}

// what the batch takes for a file and the settings its encoder will report, from the header alone
bool job_control(Job &j, const char *name, const Options &opt, bool conv)
{
    Input &in = j.in;
    HX_E_CONTROL ec = in.ec;
    if (conv) {
        j.src = {in.wi.bits, in.is_float, opt.mpeg_select, in.mono_convert};
        if (!hx_src_encode_control(&in.ec, &j.src, &ec)) { fprintf(stderr, "\n ENCODER INIT FAIL (%s): %s\n", name, hx_last_error()); return false; }
    } else if (in.mono_convert) ec.mode = 3;
    j.nch = ec.mode == 3 ? 1 : 2;
    if (!hx_control_info(&ec, &in.ec_used, &in.head)) { fprintf(stderr, "\n ENCODER INIT FAIL (%s)\n", name); return false; }
    j.ctl = conv ? in.ec : ec;          // (a converting batch derives the encoder's control from the source's, as converter_calls did)
    return true;
}

// a finished file: what the single-file loop would have written
bool job_write(Job &j, const char *name, const Options &opt)
{
    const Input &in = j.in;
    bool ok = true;
    if (!j.led.ended) { fprintf(stderr, "\n %s: drain did not complete\n", name); ok = false; }
    const unsigned frames = j.led.frames, nbytes = j.led.bytes;
    const uint64_t out_bytes = (uint64_t) j.led.head_bytes + nbytes;
    FILE *o = fopen(name, "wb");
    if (!o) { fprintf(stderr, "\n CANNOT CREATE OUTPUT FILE %s\n", name); return false; }
    if (j.whole) {
        // (the file came down once, from its image on the GPU, the tag frame in front of it: built there from the file's
        // record, k_file_tag - it is written as it came)
        if (j.stream.size() != (size_t) out_bytes) { fprintf(stderr, "\n %s: the file image holds %zu bytes of %llu\n", name, j.stream.size(), (unsigned long long) out_bytes); ok = false; }
        fwrite(j.stream.data(), 1, std::min<size_t>(j.stream.size(), (size_t) out_bytes), o);
    } else {
        // the ledger has made the tagger's calls on the device (k_ledger): one seek point per input call, the end of the drain
        // (while (get_frames() < frames_expected) encode silence) and the CRC up to there
        Tagger tg;
        tg.begin(in, opt.xing_flag);
        tg.crc = j.led.crc;
        hx_xing_load_points(tg.xg, &j.led);
        if (opt.xing_flag) tg.finish(in, frames, out_bytes);
        fwrite(tg.tag.data(), 1, tg.head_bytes, o);
        fwrite(j.stream.data(), 1, nbytes, o);
    }
    fclose(o);
    fprintf(stderr, "\n %s: %u frames, %llu bytes", name, frames, (unsigned long long) out_bytes);
    return ok;
}

// the description of a file's tag frame (Tagger::begin, Tagger::finish), for the GPU to build it from the file's record
HX_FILE_TAG job_tag(const Job &j, const Options &opt)
{
    Tagger tg;
    tg.begin(j.in, opt.xing_flag);
    return tg.describe(j.in);
}

// what the batch's ledger takes for a file when the file gets its slot (the tag frame's size and whether it has seek
// points: Tagger::begin)
HX_LEDGER_OPEN job_ledger(const Job &j, const Options &opt)
{
    Tagger tg;
    tg.begin(j.in, opt.xing_flag);
    return {(int) j.nc, tg.head_bytes, (tg.head_flags & 4) ? 1 : 0, 0};
}

// loaded: every file's audio is in memory and every file has its own slot; else (-slots) jobs hold the headers only
int encode_jobs(std::vector<Job> &jobs, const std::vector<const char *> &files, const Options &opt, bool loaded)
{
    const int S = (int) jobs.size(), NS = loaded ? S : std::min(S, opt.nslots);
    // One file that needs the converter sends all of them through a converting batch (a file at its own MPEG rate is the
    // converter's copy case); without one the plain batch runs, fed fp32 frames made here.
    bool conv = false;
    for (int i = 0; i < S; i++) conv = conv || needs_conversion(jobs[i].in, opt);
    for (int i = 0; i < S; i++)
        if ((loaded && conv && !job_calls(jobs[i], files[2 * i], opt, conv)) || !job_control(jobs[i], files[2 * i], opt, conv) ||
            (loaded && !conv && !job_calls(jobs[i], files[2 * i], opt, conv))) return 1;
    const int CH = 96;                                  // frames per batched call at most
    const size_t DRAIN = 32;                            // room for a file's drain frames (a reservoir never spans that many)
    // the files (the slots) spread over the node's GPUs in contiguous blocks (-Gn limits the count), one host thread per device
    hx_multi *b = nullptr;
    std::vector<int> file_cfg(S, 0);                    // the menu entry of each file
    {
        // the menu: the distinct (control, source) pairs of all files, of whatever channel count, rate and stereo mode; the
        // slots start with the first files' entries - without -slots every file has its own
        std::vector<HX_E_CONTROL> ctl;
        std::vector<HX_SOURCE> srcs;
        for (int i = 0; i < S; i++) {
            size_t k = 0;
            while (k < ctl.size() && (memcmp(&ctl[k], &jobs[i].ctl, sizeof(HX_E_CONTROL)) || memcmp(&srcs[k], &jobs[i].src, sizeof(HX_SOURCE)))) k++;
            if (k == ctl.size()) { ctl.push_back(jobs[i].ctl); srcs.push_back(jobs[i].src); }
            file_cfg[i] = (int) k;
        }
        b = hx_multi_create_any(opt.ngpus, nullptr, NS, ctl.data(), (int) ctl.size(), conv ? srcs.data() : nullptr, file_cfg.data(), CH);
    }
    if (!b) {
        fprintf(stderr, "\n ENCODER INIT FAIL: %s\n", hx_last_error());
        return 1;
    }
    if (!loaded) fprintf(stderr, "\n %d files through %d slots on %d GPU(s)", S, NS, hx_multi_ndevices(b));
    else if (S > 1) fprintf(stderr, "\n %d files on %d GPU(s)", S, hx_multi_ndevices(b));
    if (opt.ec_display) print_ec(&jobs[0].in.ec_used);
    // slot -> the file it holds (-1: none any more), and the next file that waits for a slot
    std::vector<int> held(NS);
    int next = NS, rc = 0;
    for (int s = 0; s < NS; s++) {
        held[s] = s;
        if (!loaded && (!load_input(files[2 * s], opt, &jobs[s].in, false) || !job_control(jobs[s], files[2 * s], opt, conv) || !job_calls(jobs[s], files[2 * s], opt, conv))) { hx_multi_destroy(b); return 1; }
    }
    const long long stride = hx_multi_out_stride(b, CH);
    // the plain route feeds one tight image per call (PCM segments): every file's frames of the call back to back, a mono
    // file's at half a stereo file's size, nothing for a slot that sits the call out - only that crosses the link.  (Its
    // capacity is the rows': pitched for the widest file's channels.)
    const int pitch = hx_batch_pcm_channels(hx_multi_batch(b, 0));
    std::vector<float> pcm(conv ? 0 : (size_t) NS * CH * 1152 * pitch), tmp(2304);
    std::vector<long long> seg(NS + 1, 0);
    std::vector<int> seg_ch(NS, 1);
    long long image = 0;
    const std::vector<unsigned char> zero_frame(2304 * 4, 0);
    // converting route: a row holds the file's bytes from its next call on, enough for CH calls of any file, then a region of
    // zero bytes that every drain call reads, as the single-file loop hands one zero buffer to all of them
    const long long row_data = conv ? hx_multi_src_in_stride(b, CH) : 0, in_stride = row_data + (conv ? hx_multi_src_in_stride(b, 1) : 0);
    std::vector<unsigned char> rows((size_t) NS * in_stride);
    std::vector<long long> off(conv ? (size_t) NS * CH : 0);
    std::vector<unsigned char> out((size_t) NS * stride);
    std::vector<int> nb(NS), stats((size_t) NS * CH * 2);
    // the MusicCRC per file: every call returns the CRC of its own bytes up to each input frame (k_crc, on the GPU), and the
    // file's is those joined by hx_xing_crc_combine - whole calls, then the call in which the file's drain ends up to there
    std::vector<unsigned short> crc((size_t) NS * CH);
    // Every call gives each file the frames it still needs (per-stream frame counts): its input frames, then silence up to the
    // frame at which its drain ends; a finished file takes 0 and costs nothing, and the loop ends with the last file, not
    // DRAIN frames behind the longest one for all.  The call is as long as its largest count.
    std::vector<int> cnt(NS), take_slot, take_cfg, fed_slot;
    // The ledger (k_ledger, on the GPU) decides where each file ends and keeps its byte count, MusicCRC and seek points: a
    // file's record begins when the file gets its slot, and after each call the records of the slots that took frames come down
    std::vector<HX_LEDGER_OPEN> take_open(NS);
    std::vector<HX_LEDGER> led(NS);
    // File images: the bytes the ledger gives to a file are put behind the file's bytes so far in the slot's image on the GPU
    // (k_file_append), so a call brings down its status and one short record per slot, and a file comes down once, when it
    // has ended: the files that end in a call get their tag frames built into their images' head room (k_file_tag, from the
    // records on the device) and come down together as one dense image (hx_multi_file_tags, hx_multi_file_fetch_many).  An
    // image holds the largest file of the run at the bound of hx_multi_out_stride: every block it is fed, the
    // drain's included, at the size of the largest frames a block can yield, behind the tag frame.  Where the device cannot
    // hold that for every slot, the rows come back with every call as before.
    bool use_img = true;
    {
        size_t most = 0;
        for (const Job &j : jobs) {
            const size_t calls = loaded ? j.nc : j.est_calls;
            use_img = use_img && calls > 0;
            most = std::max(most, calls);
        }
        const long long cap = 2048 + (long long) (most + DRAIN) * hx_multi_out_stride(b, 1);
        if (!use_img) fprintf(stderr, "\n an input's length is not known in advance: no file images, every call's rows come back");
        else if (hx_multi_file_images(b, cap) != 0) {
            fprintf(stderr, "\n no file images of %lld bytes per slot (%s): every call's rows come back", cap, hx_last_error());
            use_img = false;
        }
    }
    std::vector<HX_LEDGER_BRIEF> brief(NS);
    std::vector<int> done;                              // the slots whose files have finished in this call, their tags' descriptions,
    std::vector<HX_FILE_TAG> done_tag;                  // and their files as one image: segment e at many_off[e]
    std::vector<unsigned char> many;
    std::vector<long long> many_off;
    for (int s = 0; s < NS; s++) { fed_slot.push_back(s); take_open[s] = job_ledger(jobs[s], opt); }
    if (hx_multi_ledger_begin(b, fed_slot.data(), take_open.data(), NS) != 0) {
        fprintf(stderr, "\n ENCODE FAIL: %s\n", hx_last_error());
        hx_multi_destroy(b);
        return 1;
    }
    for (int s = 0; s < NS; s++) hx_ledger_open(&jobs[s].led, take_open[s].ncalls, 1, take_open[s].head_bytes, take_open[s].flags);
    for (;;) {
        int nf = 0;
        for (int s = 0; s < NS; s++) {
            cnt[s] = 0;
            if (held[s] < 0) continue;
            const Job &j = jobs[held[s]];
            const size_t fed = (size_t) j.led.fed, room = j.nc + DRAIN;
            cnt[s] = (j.led.ended || fed >= room) ? 0 : (int) std::min<size_t>(CH, room - fed);
            nf = std::max(nf, cnt[s]);
        }
        if (nf == 0) break;
        if (!conv) {
            for (int s = 0; s < NS; s++) seg_ch[s] = held[s] >= 0 ? jobs[held[s]].nch : 1;
            image = hx_pcm_packed_layout(NS, nf, cnt.data(), seg_ch.data(), (int) sizeof(float), seg.data());
        }
        for (int s = 0; s < NS && !conv; s++) {
            if (cnt[s] == 0) continue;
            const Job &j = jobs[held[s]];
            const size_t p0 = (size_t) j.led.fed;
            for (int k = 0; k < cnt[s]; k++) {
                // past the end the single-file loop feeds frames of zero BYTES: silence, except for
                // 8-bit unsigned input where a zero byte is full-scale negative
                if (p0 + k < j.nc) frame_to_float(j.in, j.in.data.data() + (p0 + k) * j.in.frame_in, tmp.data());
                else frame_to_float(j.in, zero_frame.data(), tmp.data());
                memcpy(&pcm[(size_t) seg[s] / sizeof(float) + (size_t) k * j.nch * 1152], tmp.data(), sizeof(float) * 1152 * j.nch);
            }
        }
        for (int s = 0; s < NS && conv; s++) {
            // the calls on the file's input start where the schedule puts them, counted from the row's first byte; the
            // drain calls all read the zero region (zero bytes: 8-bit input stays full-scale negative there too)
            if (cnt[s] == 0) continue;
            const Job &j = jobs[held[s]];
            const size_t p0 = (size_t) j.led.fed;
            unsigned char *row = rows.data() + (size_t) s * in_stride;
            memset(row, 0, (size_t) in_stride);
            const long long base = p0 < j.nc ? j.start[p0] : 0;
            if (p0 < j.nc) memcpy(row, j.in.data.data() + base, (size_t) std::min<long long>(row_data, (long long) j.in.data.size() - base));
            for (int k = 0; k < nf; k++) off[(size_t) s * nf + k] = (k < cnt[s] && p0 + k < j.nc) ? j.start[p0 + k] - base : row_data;
        }
        int rc_call;
        if (!use_img)
            rc_call = conv ? hx_multi_encode_src_counts_host(b, rows.data(), in_stride, off.data(), nf, cnt.data(), out.data(), stride, nb.data(), nullptr, stats.data(), crc.data())
                           : (hx_multi_frame_counts(b, cnt.data()) != 0 || hx_multi_pcm_segments(b, seg.data(), image) != 0 || hx_multi_encode_f32_host_crc(b, pcm.data(), nf, out.data(), stride, nb.data(), stats.data(), crc.data()) != 0);
        else {
            // (the call's return value is the status word: a file that outgrew its image ends the run, anything else is
            // reported at the end as before)
            rc_call = conv ? hx_multi_encode_src_files_host(b, rows.data(), in_stride, off.data(), nf, cnt.data(), nullptr)
                           : (hx_multi_frame_counts(b, cnt.data()) != 0 || hx_multi_pcm_segments(b, seg.data(), image) != 0) ? -1 : hx_multi_encode_f32_host_files(b, pcm.data(), nf);
            if (rc_call > 0 && (rc_call & 64)) {
                fprintf(stderr, "\n ENCODE FAIL: a file outgrew its image on the GPU\n");
                hx_multi_destroy(b);
                return 1;
            }
            if (rc_call > 0) rc_call = 0;
        }
        if (rc_call != 0) {
            fprintf(stderr, "\n ENCODE FAIL: %s\n", hx_last_error());
            hx_multi_destroy(b);
            return 1;
        }
        take_slot.clear(); take_cfg.clear(); take_open.clear(); fed_slot.clear();
        for (int s = 0; s < NS; s++) if (cnt[s] > 0) fed_slot.push_back(s);
        if ((use_img ? hx_multi_ledger_poll(b, brief.data()) : hx_multi_ledger_read(b, fed_slot.data(), (int) fed_slot.size(), led.data())) != 0) {
            fprintf(stderr, "\n ENCODE FAIL: %s\n", hx_last_error());
            hx_multi_destroy(b);
            return 1;
        }
        done.clear(); done_tag.clear();
        for (size_t e = 0; e < fed_slot.size() && use_img; e++) {
            // the short record says how far the file is; when it has ended (or reached its drain bound) it is one of this call's
            // finished files
            const int s = fed_slot[e];
            Job &j = jobs[held[s]];
            const HX_LEDGER_BRIEF &r = brief[s];
            j.led.open = r.open; j.led.ended = r.ended; j.led.fed = r.fed; j.led.frames = r.frames; j.led.bytes = r.bytes; j.led.crc = r.crc;
            j.led.call_bytes = r.call_bytes;
            if (!(j.led.ended || (size_t) j.led.fed >= j.nc + DRAIN)) continue;
            done.push_back(s);
            done_tag.push_back(job_tag(j, opt));
        }
        if (!done.empty()) {
            // one launch builds their tag frames, two launches and two copies bring them down, however many they are
            const int n = (int) done.size();
            long long need = 0;
            for (int s : done) need += ((long long) jobs[held[s]].led.head_bytes + brief[s].image_bytes + 15) & ~15LL;
            many.resize((size_t) std::max(need, 16LL));
            many_off.assign((size_t) n + 1, 0);
            if (hx_multi_file_tags(b, done.data(), done_tag.data(), n) != 0 ||
                hx_multi_file_fetch_many(b, done.data(), n, many.data(), (long long) many.size(), many_off.data()) != need) {
                fprintf(stderr, "\n ENCODE FAIL: %s\n", hx_last_error());
                hx_multi_destroy(b);
                return 1;
            }
            for (int e = 0; e < n; e++) {
                Job &j = jobs[held[done[e]]];
                const size_t len = (size_t) j.led.head_bytes + brief[done[e]].image_bytes;
                j.stream.assign(many.begin() + many_off[e], many.begin() + many_off[e] + (long long) len);
                j.whole = true;
            }
        }
        for (size_t e = 0; e < fed_slot.size(); e++) {
            const int s = fed_slot[e];
            Job &j = jobs[held[s]];
            if (!use_img) {
                // the bytes of this call's row that belong to the file: all of it, or up to the frame at which its drain ended
                j.led = led[e];
                j.stream.insert(j.stream.end(), out.begin() + (size_t) s * stride, out.begin() + (size_t) s * stride + j.led.call_bytes);
            }
            if (loaded || !(j.led.ended || (size_t) j.led.fed >= j.nc + DRAIN)) continue;
            // -slots: the file is written and freed, and its slot goes to the next file that waits
            if (!job_write(j, files[2 * held[s] + 1], opt)) rc = 1;
            j = Job();
            held[s] = -1;
            if (next == S) continue;
            const int i = next++;
            if (!load_input(files[2 * i], opt, &jobs[i].in, false) || !job_control(jobs[i], files[2 * i], opt, conv) || !job_calls(jobs[i], files[2 * i], opt, conv)) { hx_multi_destroy(b); return 1; }
            held[s] = i;
            take_slot.push_back(s); take_cfg.push_back(file_cfg[i]); take_open.push_back(job_ledger(jobs[i], opt));
            hx_ledger_open(&jobs[i].led, take_open.back().ncalls, 1, take_open.back().head_bytes, take_open.back().flags);
        }
        if (!take_slot.empty() && (hx_multi_assign_streams(b, take_slot.data(), take_cfg.data(), (int) take_slot.size()) != 0 ||
                                   hx_multi_ledger_begin(b, take_slot.data(), take_open.data(), (int) take_slot.size()) != 0)) {
            fprintf(stderr, "\n ENCODE FAIL: %s\n", hx_last_error());
            hx_multi_destroy(b);
            return 1;
        }
    }
    if (hx_multi_status(b) != 0) fprintf(stderr, "\n WARNING: kernel status %d\n", hx_multi_status(b));
    hx_multi_destroy(b);
    for (int i = 0; i < S && loaded; i++) if (!job_write(jobs[i], files[2 * i + 1], opt)) rc = 1;
    fprintf(stderr, "\n");
    return rc;
}

}  // namespace

int main(int argc, char **argv)
{
    Options opt;
    hx_default_control(&opt.ec);        // the reference CLI's defaults (tomp3.cpp:357-384)
    opt.ec.bitrate = -1;
    std::vector<const char *> files;
    bool batch = false;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (a[0] != '-' || a[1] == '\0') { files.push_back(a); continue; }
        if (!strcmp(a, "-batch")) { batch = true; continue; }
        if (!strncmp(a, "-slots", 6)) { opt.nslots = atoi(a + 6); continue; }      // (before the switch: -s... is -S<n>, the DC blocker)
        HX_E_CONTROL &ec = opt.ec;
        const char c = (char) (a[1] | 0x20), c2 = (char) (a[2] | 0x20);
        switch (c) {
        case 'h': if (c2 == 'f') ec.hf_flag = 1 | atoi(a + 3); else { usage(); return 0; } break;
        case 'e': if (c2 == 'c') opt.ec_display = 1; break;            // -EC: print the settings in use (tomp3.cpp:412-416)
        case 'g': opt.ngpus = atoi(a + 2); break;                      // -Gn: GPUs for -batch (default: all)
        case 'd': case 'p': case 'z': break;                            // -D progress display off, -P / -Z reserved (tomp3.cpp:438-441,470-472,508-511): nothing to do here
        case 'q': ec.quick = atoi(a + 2); break;
        case 'u': ec.cpu_select = atoi(a + 2); break;
        case 'x': opt.xing_flag = atoi(a + 2); if (opt.xing_flag == 2) opt.xing_flag = 3; break;
        case 'b': ec.bitrate = atoi(a + 2); break;
        case 'c': ec.cr_bit = atoi(a + 2); break;
        case 'o': ec.original = atoi(a + 2); break;
        case 'm': ec.mode = atoi(a + 2); break;
        case 'n': ec.nsbstereo = atoi(a + 2); break;
        case 's': if (c2 == 'b' && (a[3] | 0x20) == 't') ec.short_block_threshold = atoi(a + 4); else ec.filter_select = atoi(a + 2); break;
        case 'f': ec.freq_limit = atoi(a + 2); break;
        case 't': if (c2 == 'x') ec.test1 = atoi(a + 3); else ec.vbr_delta_mnr = atoi(a + 2); break;
        case 'i': if (c2 == 'l') opt.ignore_length = 1; else ec.chan_add_f0 = atoi(a + 2); break;
        case 'j': ec.chan_add_f1 = atoi(a + 2); break;
        case 'v': ec.vbr_flag = 1; ec.vbr_mnr = atoi(a + 2); break;
        case 'l': ec.vbr_br_limit = atoi(a + 2); break;
        case 'a': opt.mpeg_select = atoi(a + 2); if (opt.mpeg_select < 0) opt.mpeg_select = 0; break;
        case 'w': {                 // -W<file>: 21 per-band MNR offsets (tomp3.cpp:552-555, get_mnr_adjust :1203-1233)
            FILE *f = fopen(a + 2, "rt");
            if (!f) break;          // (the reference ignores a file it cannot open)
            for (int k = 0; k < 21; k++) ec.mnr_adjust[k] = 0;
            for (int k = 0, m = 0; k < 21 && fscanf(f, "%d", &m) == 1; k++) ec.mnr_adjust[k] = m;
            fclose(f);
            fprintf(stderr, "\nMNR adjust ");
            for (int k = 0; k < 21; k++) { ec.mnr_adjust[k] = std::max(-200, std::min(200, ec.mnr_adjust[k])); fprintf(stderr, " %d", ec.mnr_adjust[k]); }
            break;
        }
        default: break;             // unknown switches: ignored like the reference does
        }
    }
    opt.ec.vbr_flag = opt.ec.bitrate < 0 ? 1 : 0;
    if (batch) {
        if (files.empty() || (files.size() & 1)) { usage(); return 1; }
        return encode_batch(files, opt);
    }
    if (files.size() < 2) { usage(); return 1; }
    return encode_one_file(files[0], files[1], opt);
}
