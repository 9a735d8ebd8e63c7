// hx_multi.cpp - several GPUs of one node behind one handle: the streams are split into contiguous
// blocks, one hx_batch per device, and every call runs one host thread per device on its block of the
// caller's buffers.  Streams are independent, so nothing is exchanged between the devices.  With it, the host
// placement those threads need.  Launches no kernel: built by the host compiler.
#include <string>
#include <thread>
#include <sched.h>
#include <unistd.h>
#include "hx_rt.h"

// ---- host placement: the NUMA node of a device, and threads / page-locked buffers next to it ----
// A host-fed GPU takes 49 GB/s of PCM over PCIe (bench.py host_fed); eight of them read 394 GB/s of host memory.  That only
// works out of the memory of the socket the GPU hangs on: a rank (or a dispatcher thread) binds itself to the CPUs of its
// device's NUMA node before it allocates its page-locked buffers (first touch puts the pages there) and stays there for its
// copies' submission.  Everything here is best effort: no sysfs entry, one node, or a CPU set that the cgroup does not allow
// leaves the thread where it was and reports -1 / 0.
static int read_int_file(const char *path, int *v)
{
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    const int ok = fscanf(f, "%d", v) == 1;
    fclose(f);
    return ok ? 0 : -1;
}

// NUMA node of HIP device `device` (-1: unknown / not a NUMA machine), from its PCI address in sysfs
extern "C" int hx_device_numa_node(int device)
{
    char bus[64] = {0}, path[256];
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void) hipGetLastError(); return -1; }
    if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus), device) != hipSuccess) { (void) hipGetLastError(); return -1; }     // (the error is not left behind for the next launch check)
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char) (*c - 'A' + 'a');      // sysfs spells the address in lower case
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    int node = -1;
    if (read_int_file(path, &node) != 0) return -1;
    return node;
}

// The CPUs this process may use, captured once when the library is loaded (= before any thread was bound by it): a thread
// that was bound to one device's node must be able to move to another device's node afterwards, so a node's CPU list is
// intersected with this set, not with the calling thread's current mask.
static cpu_set_t g_proc_cpus;
static bool g_proc_cpus_ok = false;
__attribute__((constructor)) static void capture_process_cpus()
{
    CPU_ZERO(&g_proc_cpus);
    g_proc_cpus_ok = sched_getaffinity(0, sizeof(g_proc_cpus), &g_proc_cpus) == 0;
}
// A process whose CPU set changes after the library was loaded (a launcher that calls sched_setaffinity / taskset on the
// running process, a cpuset change; in Python the library loads lazily, so "when it was loaded" depends on import order)
// takes the set again from its main thread's current mask: returns the number of CPUs, 0 on failure.  The bind calls also
// do this once by themselves when the kernel refuses the mask they computed (EINVAL: none of its CPUs is allowed any more).
extern "C" int hx_refresh_process_cpus(void)
{
    cpu_set_t now;
    CPU_ZERO(&now);
    if (sched_getaffinity(getpid(), sizeof(now), &now) != 0) return 0;      // (pid = the main thread's id)
    g_proc_cpus = now;
    g_proc_cpus_ok = true;
    return CPU_COUNT(&now);
}

// the CPUs of a node that this process may use: parses /sys/devices/system/node/node<N>/cpulist ("0-15,128-143")
static int node_cpus_allowed(int node, cpu_set_t *out)
{
    char path[128], buf[4096];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return 0;
    const bool got = fgets(buf, sizeof(buf), f) != nullptr;
    fclose(f);
    if (!got || !g_proc_cpus_ok) return 0;
    CPU_ZERO(out);
    int n = 0;
    for (char *p = buf; *p;) {
        char *e;
        long a = strtol(p, &e, 10), z = a;
        if (e == p) break;
        if (*e == '-') { p = e + 1; z = strtol(p, &e, 10); }
        for (long c = a; c <= z && c < CPU_SETSIZE; c++) if (CPU_ISSET((int) c, &g_proc_cpus)) { CPU_SET((int) c, out); n++; }
        p = (*e == ',') ? e + 1 : e;
        if (*e != ',') break;
    }
    return n;
}

// bind the calling thread to the allowed CPUs of NUMA node `node`; returns how many CPUs that is (0: left as it was)
extern "C" int hx_bind_thread_to_node(int node)
{
    if (node < 0) return 0;
    cpu_set_t set;
    int n = node_cpus_allowed(node, &set);
    if (n > 0 && sched_setaffinity(0, sizeof(set), &set) == 0) return n;
    // the process's CPU set may have been narrowed since it was captured: take it again, try once more
    if (hx_refresh_process_cpus() <= 0) return 0;
    n = node_cpus_allowed(node, &set);
    if (n <= 0) return 0;
    return sched_setaffinity(0, sizeof(set), &set) == 0 ? n : 0;
}

// bind the calling thread to the allowed CPUs of `device`'s NUMA node; returns how many CPUs that is (0: left as it was)
extern "C" int hx_bind_thread_to_device(int device)
{
    return hx_bind_thread_to_node(hx_device_numa_node(device));
}

struct hx_multi {
    std::vector<hx_batch *> part;
    std::vector<int> first, count, device;
    std::vector<cpu_set_t> cpus;        // per device: the CPUs of its NUMA node this process may use (resolved once, at creation)
    std::vector<int> ncpus;             // ... and how many (0: unknown, the device's thread stays where it is)
    int S = 0, nchan = 2;               // nchan: the pitch of the PCM rows (hx_batch::nchan), the same for every block
};

extern "C" void hx_multi_destroy(hx_multi *m)
{
    if (!m) return;
    for (hx_batch *b : m->part) hx_batch_destroy(b);
    delete m;
}

// the blocks of streams and their batches; make(device, first, count) creates block k's batch
template <class Make>
static hx_multi *multi_create(int ndev, const int *devices, int nstreams, Make make)
{
    const int have = hx_device_count();
    if (ndev <= 0) ndev = have;
    if (ndev > nstreams) ndev = nstreams;
    if (ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return nullptr; }
    hx_multi *m = new hx_multi;
    m->S = nstreams;
    const int base = nstreams / ndev, rem = nstreams % ndev;       // block sizes differ by at most one (hmp3_amd/shard.py)
    for (int k = 0; k < ndev; k++) {
        const int first = k * base + (k < rem ? k : rem), count = base + (k < rem ? 1 : 0);
        const int dev = devices ? devices[k] : k;
        hx_batch *b = make(dev, first, count);
        if (!b) { hx_multi_destroy(m); return nullptr; }            // hx_last_error is hx_batch_create's
        m->part.push_back(b); m->first.push_back(first); m->count.push_back(count); m->device.push_back(dev);
        cpu_set_t cs;
        CPU_ZERO(&cs);
        const int node = hx_device_numa_node(dev);
        m->ncpus.push_back(node >= 0 ? node_cpus_allowed(node, &cs) : 0);
        m->cpus.push_back(cs);
        // (what the blocks must agree in - the rows' pitch and the frame positions per block, which size out_stride - is the
        // menu's, whichever entries a block's slots start with: blocks that get the whole menu agree, of whatever kinds it is)
        if (k == 0) m->nchan = b->nchan;
        else if (b->nchan != m->nchan || b->lsf != m->part[0]->lsf) { set_err("mono / stereo and MPEG-1 / MPEG-2 streams cannot share a batch"); hx_multi_destroy(m); return nullptr; }
    }
    return m;
}

extern "C" hx_multi *hx_multi_create(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int shared_control, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec) { set_err("bad arguments"); return nullptr; }
    return multi_create(ndev, devices, nstreams, [&](int dev, int first, int count) {
        return hx_batch_create(dev, count, shared_control ? ec : ec + first, shared_control, max_frames);
    });
}

// converting batches over several devices (stream numbers in hx_last_error are the block's)
extern "C" hx_multi *hx_multi_create_src(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int shared_control,
                                         const HX_SOURCE *src, int shared_source, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || !src) { set_err("bad arguments"); return nullptr; }
    return multi_create(ndev, devices, nstreams, [&](int dev, int first, int count) {
        return hx_batch_create_src(dev, count, shared_control ? ec : ec + first, shared_control, shared_source ? src : src + first, shared_source, max_frames);
    });
}

// every block's batch gets the whole menu, and its streams' part of cfg
extern "C" hx_multi *hx_multi_create_menu(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                                          const int *cfg, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || nmenu <= 0) { set_err("bad arguments"); return nullptr; }
    return multi_create(ndev, devices, nstreams, [&](int dev, int first, int count) {
        return hx_batch_create_menu(dev, count, ec, nmenu, src, cfg ? cfg + first : nullptr, max_frames);
    });
}

// ... entries of either channel count: every block's rows are pitched for the menu's widest entry, so the blocks agree
extern "C" hx_multi *hx_multi_create_mixed(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                                           const int *cfg, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || nmenu <= 0) { set_err("bad arguments"); return nullptr; }
    return multi_create(ndev, devices, nstreams, [&](int dev, int first, int count) {
        return hx_batch_create_mixed(dev, count, ec, nmenu, src, cfg ? cfg + first : nullptr, max_frames);
    });
}

// ... and of either MPEG version and allocator generation (hx_batch_create_any)
extern "C" hx_multi *hx_multi_create_any(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                                         const int *cfg, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || nmenu <= 0) { set_err("bad arguments"); return nullptr; }
    return multi_create(ndev, devices, nstreams, [&](int dev, int first, int count) {
        return hx_batch_create_any(dev, count, ec, nmenu, src, cfg ? cfg + first : nullptr, max_frames);
    });
}

// hx_batch_assign_streams over all streams.  All blocks or none: every refusal is made here, with the caller's entry
// numbers, before one block starts; then each block takes its part of the list, waits for its work in flight and is done
// when the call returns.
extern "C" int hx_multi_assign_streams(hx_multi *m, const int *idx, const int *cfg, int n)
{
    char msg[160];
#define REFUSE(...) do { snprintf(msg, sizeof msg, __VA_ARGS__); set_err("%s", msg); return -1; } while (0)
    if (!m) { set_err("null handle"); return -1; }
    for (hx_batch *b : m->part) if (check_poisoned(b) != 0) return -1;
    if (n < 0) REFUSE("n = %d: the number of listed slots cannot be negative", n);
    if (n > 0 && !idx) { set_err("idx is null with n > 0"); return -1; }
    if (n > 0 && !cfg) { set_err("cfg is null with n > 0"); return -1; }
    const int nmenu = hx_batch_nconfigs(m->part[0]);
    const size_t nb = m->part.size();
    std::vector<char> listed(m->S, 0);
    std::vector<std::vector<int>> bi(nb), bc(nb);
    for (int e = 0; e < n; e++) {
        if (idx[e] < 0 || idx[e] >= m->S) REFUSE("entry %d: slot %d out of range (0 .. %d)", e, idx[e], m->S - 1);
        if (listed[idx[e]]) REFUSE("entry %d: slot %d is listed twice", e, idx[e]);
        if (cfg[e] < 0 || cfg[e] >= nmenu) REFUSE("entry %d: configuration %d out of range (0 .. %d)", e, cfg[e], nmenu - 1);
        listed[idx[e]] = 1;
        size_t k = 0;
        while (k + 1 < nb && idx[e] >= m->first[k + 1]) k++;
        bi[k].push_back(idx[e] - m->first[k]);
        bc[k].push_back(cfg[e]);
    }
#undef REFUSE
    for (size_t k = 0; k < nb; k++)
        if (!bi[k].empty() && assign_slots(m->part[k], bi[k].data(), bc[k].data(), (int) bi[k].size(), nullptr, true) != 0) return -1;
    return 0;
}

// hx_batch_ledger_begin / hx_batch_ledger_read over all streams, like hx_multi_assign_streams: every refusal here, with the
// caller's entry numbers, before one block starts; then each block takes its part of the list and is done when the call
// returns.  where[e] = (block, position in the block's list) of entry e.
static int multi_ledger_split(hx_multi *m, const int *idx, const HX_LEDGER_OPEN *open, bool begin, const void *out, int n,
                              std::vector<std::vector<int>> &bi, std::vector<std::pair<size_t, size_t>> &where)
{
    char msg[160];
#define REFUSE(...) do { snprintf(msg, sizeof msg, __VA_ARGS__); set_err("%s", msg); return -1; } while (0)
    if (!m) { set_err("null handle"); return -1; }
    for (hx_batch *b : m->part) if (check_poisoned(b) != 0) return -1;
    if (n < 0) REFUSE("n = %d: the number of listed slots cannot be negative", n);
    if (n > 0 && !idx) { set_err("idx is null with n > 0"); return -1; }
    if (n > 0 && begin && !open) { set_err("open is null with n > 0"); return -1; }
    if (n > 0 && !begin && !out) { set_err("out is null with n > 0"); return -1; }
    const size_t nb = m->part.size();
    std::vector<char> listed(m->S, 0);
    bi.assign(nb, std::vector<int>());
    for (int e = 0; e < n; e++) {
        if (idx[e] < 0 || idx[e] >= m->S) REFUSE("entry %d: slot %d out of range (0 .. %d)", e, idx[e], m->S - 1);
        if (listed[idx[e]]) REFUSE("entry %d: slot %d is listed twice", e, idx[e]);
        if (begin && open[e].ncalls < 1) REFUSE("entry %d: ncalls < 1", e);
        if (begin && open[e].head_bytes < 0) REFUSE("entry %d: head_bytes < 0", e);
        listed[idx[e]] = 1;
        size_t k = 0;
        while (k + 1 < nb && idx[e] >= m->first[k + 1]) k++;
        where.push_back({k, bi[k].size()});
        bi[k].push_back(idx[e] - m->first[k]);
    }
#undef REFUSE
    return 0;
}
extern "C" int hx_multi_ledger_begin(hx_multi *m, const int *idx, const HX_LEDGER_OPEN *open, int n)
{
    std::vector<std::vector<int>> bi;
    std::vector<std::pair<size_t, size_t>> where;
    if (multi_ledger_split(m, idx, open, true, nullptr, n, bi, where) != 0) return -1;
    std::vector<std::vector<HX_LEDGER_OPEN>> bo(bi.size());
    for (int e = 0; e < n; e++) bo[where[e].first].push_back(open[e]);
    for (size_t k = 0; k < bi.size(); k++)
        if (!bi[k].empty() && ledger_begin(m->part[k], bi[k].data(), bo[k].data(), (int) bi[k].size(), nullptr, true) != 0) return -1;
    return 0;
}
extern "C" int hx_multi_ledger_read(hx_multi *m, const int *idx, int n, HX_LEDGER *out)
{
    std::vector<std::vector<int>> bi;
    std::vector<std::pair<size_t, size_t>> where;
    if (multi_ledger_split(m, idx, nullptr, false, out, n, bi, where) != 0) return -1;
    std::vector<std::vector<HX_LEDGER>> br(bi.size());
    for (size_t k = 0; k < bi.size(); k++) {
        br[k].resize(bi[k].size());
        if (!bi[k].empty() && ledger_read(m->part[k], bi[k].data(), (int) bi[k].size(), br[k].data()) != 0) return -1;
    }
    for (int e = 0; e < n; e++) out[e] = br[where[e].first][where[e].second];
    return 0;
}

extern "C" int hx_multi_ndevices(const hx_multi *m) { return m ? (int) m->part.size() : 0; }
extern "C" int hx_multi_nstreams(const hx_multi *m) { return m ? m->S : 0; }
extern "C" hx_batch *hx_multi_batch(hx_multi *m, int k) { return (m && k >= 0 && k < (int) m->part.size()) ? m->part[k] : nullptr; }
extern "C" int hx_multi_shard(const hx_multi *m, int k, int *device, int *first, int *count)
{
    if (!m || k < 0 || k >= (int) m->part.size()) return -1;
    if (device) *device = m->device[k];
    if (first) *first = m->first[k];
    if (count) *count = m->count[k];
    return 0;
}

extern "C" long long hx_multi_out_stride(const hx_multi *m, int nframes)
{
    long long n = 0;
    if (m) for (hx_batch *b : m->part) { const long long v = hx_batch_out_stride(b, nframes); if (v > n) n = v; }
    return n;
}

// hx_batch_frame_counts over all streams: every block's batch takes its streams' part.  All blocks or none: what can fail
// (a converting batch, the first use's allocations) is settled for every block before one of them is set.
extern "C" int hx_multi_frame_counts(hx_multi *m, const int *nfr)
{
    if (!m) { set_err("null handle"); return -1; }
    for (hx_batch *b : m->part) if (counts_reserve(b, nfr != nullptr) != 0) return -1;
    for (size_t k = 0; k < m->part.size(); k++)
        if (hx_batch_frame_counts(m->part[k], nfr ? nfr + m->first[k] : nullptr) != 0) return -1;     // (cannot fail any more)
    return 0;
}

// hx_batch_pcm_segments over all streams, the same way: every block's batch takes its streams' offsets, which address the
// caller's one image - so every block keeps the image's size, and its calls get the image's base (multi_encode_host).
extern "C" int hx_multi_pcm_segments(hx_multi *m, const long long *off, long long in_bytes)
{
    if (!m) { set_err("null handle"); return -1; }
    if (off && in_bytes < 0) { set_err("in_bytes < 0"); return -1; }
    for (hx_batch *b : m->part) if (segs_reserve(b, off != nullptr) != 0) return -1;
    for (size_t k = 0; k < m->part.size(); k++)
        if (hx_batch_pcm_segments(m->part[k], off ? off + m->first[k] : nullptr, in_bytes) != 0) return -1;     // (cannot fail any more)
    return 0;
}

// hx_batch_pcm_planes over all streams, the same way
extern "C" int hx_multi_pcm_planes(hx_multi *m, const long long *off, const long long *chan_stride, long long in_bytes, int unit_scale)
{
    if (!m) { set_err("null handle"); return -1; }
    for (hx_batch *b : m->part) if (segs_reserve(b, off != nullptr) != 0) return -1;
    if (planes_args(off, in_bytes, unit_scale) != 0) return -1;
    for (size_t k = 0; k < m->part.size(); k++)
        if (hx_batch_pcm_planes(m->part[k], off ? off + m->first[k] : nullptr, off && chan_stride ? chan_stride + m->first[k] : nullptr, in_bytes, unit_scale) != 0)
            return -1;      // (cannot fail any more)
    return 0;
}

// Argument checks of the calls over all devices, the per-stream frame counts of every block included: a call that one
// block would refuse for its counts starts on no block, and its message names the stream by the caller's number.
// Then fn(k) on one thread per device, bound to the CPUs next to it.
// Returns the first failing block's code, with its message as the caller's hx_last_error.
template <class Fn>
static int multi_fanout(hx_multi *m, bool buffers_ok, int nframes, long long out_stride, Fn fn)
{
    if (!m || !buffers_ok) { set_err("null buffer"); return -1; }
    if (out_stride < hx_multi_out_stride(m, nframes)) { set_err("out_stride is smaller than hx_multi_out_stride(m, nframes)"); return -1; }
    const size_t n = m->part.size();
    if (nframes <= 0 || nframes > m->part[0]->maxF) { set_err("nframes out of range (1 .. max_frames of hx_multi_create)"); return -1; }     // (one max_frames for all blocks)
    for (size_t k = 0; k < n; k++) if (check_counts(m->part[k], nframes, m->first[k]) != 0) return -1;
    std::vector<int> rc(n, 0);
    std::vector<std::string> err(n);
    std::vector<std::thread> th;
    for (size_t k = 0; k < n; k++)
        th.emplace_back([&, k]() {
            if (m->ncpus[k] > 0) sched_setaffinity(0, sizeof(cpu_set_t), &m->cpus[k]);     // this device's copies are issued from its own socket (best effort)
            rc[k] = fn(k);
            if (rc[k]) err[k] = hx_last_error();        // the message is thread-local: hand it to the caller's thread
        });
    for (std::thread &t : th) t.join();
    for (size_t k = 0; k < n; k++) if (rc[k]) { set_err("%s", err[k].c_str()); return rc[k]; }
    return 0;
}

// the optional outputs every block's call would take (stats / crc: the host call's own; nfr: [S] a converting call's counts,
// null: each block's counts in force), checked for all blocks before one starts: a block with a live ledger record refuses
// a call without counters and CRCs, and its message names the stream by the caller's number
static int multi_check_opt(const hx_multi *m, const int *stats, const unsigned short *crc, const int *nfr)
{
    for (size_t k = 0; k < m->part.size(); k++) {
        const hx_batch *b = m->part[k];
        OptOut o = b->opt;
        if (stats) o.frame_stats = (int *) stats;
        if (crc) o.crc = (unsigned short *) crc;
        if (check_opt(b, o, nfr ? nfr + m->first[k] : counts_in_force(b), m->first[k]) != 0) return -1;
    }
    return 0;
}

// the PCM calls: each device on its block's rows of the caller's buffers
static int multi_encode_host(hx_multi *m, PcmIn in, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats,
                             unsigned short *crc = nullptr)
{
    if (m && multi_check_opt(m, stats, crc, nullptr) != 0) return -1;
    // PCM segments: checked for all blocks, with the caller's stream numbers, before one starts - behind the counts, which
    // a segment's length comes from (an nframes out of range is multi_fanout's to refuse); each block then gets the image's
    // base and copies its own span
    const bool segs = m && (!m->part[0]->seg_off.empty() || !m->part[0]->pl_off.empty());      // (segments or planes: one image)
    if (segs && nframes > 0 && nframes <= m->part[0]->maxF)
        for (size_t k = 0; k < m->part.size(); k++)
            if (check_counts(m->part[k], nframes, m->first[k]) != 0 || check_image(m->part[k], nframes, in.sample_bytes(), m->first[k]) != 0) return -1;
    return multi_fanout(m, in.p && out && out_bytes, nframes, out_stride, [&](size_t k) {
        const long long f = m->first[k];
        const char *p = (const char *) in.p + (segs ? 0 : in.bytes(f, nframes, m->nchan));
        return encode_host(m->part[k], {p, in.f32}, nframes, out + f * out_stride, out_stride, out_bytes + f, stats ? stats + f * nframes * 2 : nullptr,
                           nullptr, crc ? crc + f * nframes : nullptr);
    });
}
extern "C" int hx_multi_encode_s16_host(hx_multi *m, const int16_t *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes)
{
    return multi_encode_host(m, {pcm, false}, nframes, out, out_stride, out_bytes, nullptr);
}
extern "C" int hx_multi_encode_f32_host(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes)
{
    return multi_encode_host(m, {pcm, true}, nframes, out, out_stride, out_bytes, nullptr);
}
extern "C" int hx_multi_encode_f32_host_stats(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats)
{
    if (!stats) { set_err("null buffer"); return -1; }
    return multi_encode_host(m, {pcm, true}, nframes, out, out_stride, out_bytes, stats);
}
extern "C" int hx_multi_encode_f32_host_crc(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats,
                                            unsigned short *crc)
{
    if (!stats || !crc) { set_err("null buffer"); return -1; }
    return multi_encode_host(m, {pcm, true}, nframes, out, out_stride, out_bytes, stats, crc);
}
extern "C" long long hx_multi_src_in_stride(const hx_multi *m, int nframes)
{
    long long n = 0;
    if (m) for (hx_batch *b : m->part) n = std::max(n, hx_batch_src_in_stride(b, nframes));
    return n;
}

// hx_batch_encode_src_counts_host over all streams.  All blocks or none: the counts' range, the optional outputs and every
// stream's input extent are checked for all blocks, with the caller's stream numbers, before one block starts.
extern "C" int hx_multi_encode_src_counts_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                                               const int *nfr, unsigned char *out, long long out_stride, int *out_bytes, long long *in_used,
                                               int *stats, unsigned short *crc)
{
    if (m && nframes > 0 && in_stride > 0) {
        if (crc && !stats) { set_err("crc needs stats: the CRCs follow from the call's frame counters"); return -1; }
        if (check_counts_arg(nfr, m->S, nframes, 0) != 0 || multi_check_opt(m, stats, crc, nfr) != 0) return -1;
        for (size_t k = 0; k < m->part.size(); k++) {
            const long long f = m->first[k];
            if (!m->part[k]->nsrc) { set_err("not a converting batch (hx_multi_create_src)"); return -1; }
            if (src_extents(m->part[k], in_stride, frame_off ? frame_off + f * nframes : nullptr, nframes, nfr ? nfr + f : nullptr, (int) f, nullptr) != 0) return -1;
        }
    }
    return multi_fanout(m, in && out && out_bytes, nframes, out_stride, [&](size_t k) {
        const long long f = m->first[k];
        return hx_batch_encode_src_counts_host(m->part[k], in + f * in_stride, in_stride, frame_off ? frame_off + f * nframes : nullptr, nframes,
                                               nfr ? nfr + f : nullptr, out + f * out_stride, out_stride, out_bytes + f, in_used ? in_used + f : nullptr,
                                               stats ? stats + f * nframes * 2 : nullptr, crc ? crc + f * nframes : nullptr);
    });
}
extern "C" int hx_multi_encode_src_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                                        unsigned char *out, long long out_stride, int *out_bytes, long long *in_used, int *stats)
{
    return hx_multi_encode_src_counts_host(m, in, in_stride, frame_off, nframes, nullptr, out, out_stride, out_bytes, in_used, stats, nullptr);
}

// ---- file images over all blocks (include/hmp3_amd.h, "file images") ----
// hx_batch_file_images: all blocks or none - every block's refusals and its allocation first (a live record is named by the
// caller's stream number), and only when all of them have theirs does one block switch
extern "C" int hx_multi_file_images(hx_multi *m, long long cap)
{
    if (!m) { set_err("null handle"); return -1; }
    const size_t nb = m->part.size();
    for (size_t k = 0; k < nb; k++)
        for (int s = 0; s < (int) m->part[k]->led_live.size(); s++)
            if (m->part[k]->led_live[s]) {
                char msg[160];
                snprintf(msg, sizeof msg, "stream %d has a live ledger record: file images are switched between files (read or poll the record's end first)", m->first[k] + s);
                set_err("%s", msg);
                return -1;
            }
    std::vector<FileImages> next(nb);
    for (size_t k = 0; k < nb; k++)
        if (images_reserve(m->part[k], cap, next[k]) != 0) {
            const std::string why = hx_last_error();
            for (size_t j = 0; j < k; j++) images_drop(m->part[j], next[j]);
            set_err("%s", why.c_str());
            return -1;
        }
    // (a commit fails on a device error only: the blocks before it have switched and stay so, the reservations of the blocks
    // behind it are released)
    for (size_t k = 0; k < nb; k++)
        if (images_commit(m->part[k], next[k]) != 0) {
            const std::string why = hx_last_error();
            for (size_t j = k; j < nb; j++) images_drop(m->part[j], next[j]);
            set_err("%s", why.c_str());
            return -1;
        }
    return 0;
}
extern "C" int hx_multi_ledger_poll(hx_multi *m, HX_LEDGER_BRIEF *out)
{
    if (!m) { set_err("null handle"); return -1; }
    if (!out) { set_err("out is null"); return -1; }
    for (hx_batch *b : m->part) if (check_poisoned(b) != 0) return -1;
    for (size_t k = 0; k < m->part.size(); k++) if (ledger_poll(m->part[k], out + m->first[k]) != 0) return -1;
    return 0;
}
extern "C" long long hx_multi_file_fetch(hx_multi *m, int i, unsigned char *dst, long long dst_cap)
{
    if (!m) { set_err("null handle"); return -1; }
    if (i < 0 || i >= m->S) { set_err("stream index out of range"); return -1; }
    size_t k = 0;
    while (k + 1 < m->part.size() && i >= m->first[k + 1]) k++;
    return hx_batch_file_fetch(m->part[k], i - m->first[k], dst, dst_cap);
}
// hx_batch_file_tags / hx_batch_file_fetch_many over all blocks ("finished files"): the list's own errors with the caller's
// entry numbers (multi_ledger_split), then what each block refuses about its files, for all blocks before one starts
static int multi_files_split(hx_multi *m, const int *idx, const HX_FILE_TAG *tags, int n, std::vector<std::vector<int>> &bi,
                             std::vector<std::pair<size_t, size_t>> &where, std::vector<std::vector<HX_FILE_TAG>> &bt)
{
    if (multi_ledger_split(m, idx, nullptr, false, idx, n, bi, where) != 0) return -1;      // (out: the callers have checked their own outputs; any non-null pointer passes the split's test)
    std::vector<std::vector<int>> entry(bi.size());
    bt.assign(bi.size(), std::vector<HX_FILE_TAG>());
    for (int e = 0; e < n; e++) {
        entry[where[e].first].push_back(e);
        if (tags) bt[where[e].first].push_back(tags[e]);
    }
    for (size_t k = 0; k < bi.size(); k++)
        if (!bi[k].empty() && files_refused(m->part[k], bi[k].data(), tags ? bt[k].data() : nullptr, (int) bi[k].size(), entry[k].data(), m->first[k]) != 0) return -1;
    return 0;
}
extern "C" int hx_multi_file_tags(hx_multi *m, const int *idx, const HX_FILE_TAG *tags, int n)
{
    if (m && n > 0 && !tags) { set_err("tags is null with n > 0"); return -1; }
    std::vector<std::vector<int>> bi;
    std::vector<std::pair<size_t, size_t>> where;
    std::vector<std::vector<HX_FILE_TAG>> bt;
    if (multi_files_split(m, idx, tags, n, bi, where, bt) != 0) return -1;
    for (size_t k = 0; k < bi.size(); k++)
        if (!bi[k].empty() && file_tags(m->part[k], bi[k].data(), bt[k].data(), (int) bi[k].size(), nullptr, true) != 0) return -1;
    return 0;
}
// every block scans its part of the list; the caller's offsets follow from the blocks' (a segment's rounded length is the
// difference of two of them); then every block brings its dense image down and the segments go to their places in dst, each
// with its zero padding
extern "C" long long hx_multi_file_fetch_many(hx_multi *m, const int *idx, int n, unsigned char *dst, long long dst_cap, long long *off)
{
    if (m && n > 0 && (!dst || !off)) { set_err("dst or off is null with n > 0"); return -1; }
    std::vector<std::vector<int>> bi;
    std::vector<std::pair<size_t, size_t>> where;
    std::vector<std::vector<HX_FILE_TAG>> bt;
    if (multi_files_split(m, idx, nullptr, n, bi, where, bt) != 0) return -1;
    if (n == 0) { if (off) off[0] = 0; return 0; }
    std::vector<std::vector<long long>> bo(bi.size());
    for (size_t k = 0; k < bi.size(); k++) {
        bo[k].assign(bi[k].size() + 1, 0);
        if (!bi[k].empty() && files_many_scan(m->part[k], bi[k].data(), (int) bi[k].size(), bo[k].data()) != 0) return -1;
    }
    off[0] = 0;
    for (int e = 0; e < n; e++) off[e + 1] = off[e] + bo[where[e].first][where[e].second + 1] - bo[where[e].first][where[e].second];
    if (off[n] > dst_cap) {
        char msg[128];
        snprintf(msg, sizeof msg, "the files' %lld bytes do not fit dst_cap %lld", off[n], dst_cap);
        set_err("%s", msg);
        return -1;
    }
    std::vector<std::vector<unsigned char>> img(bi.size());
    for (size_t k = 0; k < bi.size(); k++) {
        img[k].resize((size_t) bo[k].back());
        if (!bi[k].empty() && files_many_bring(m->part[k], (int) bi[k].size(), bo[k].back(), img[k].data()) != 0) return -1;
    }
    for (int e = 0; e < n; e++)
        if (off[e + 1] > off[e]) memcpy(dst + off[e], img[where[e].first].data() + bo[where[e].first][where[e].second], (size_t) (off[e + 1] - off[e]));
    return off[n];
}
// the *_host_files calls: ledger and images of every block checked before one starts; the blocks' status bits or'ed
static int multi_check_files(const hx_multi *m)
{
    if (!m) { set_err("null handle"); return -1; }
    for (const hx_batch *b : m->part) if (check_files(b) != 0) return -1;
    return 0;
}
static int multi_encode_host_files(hx_multi *m, PcmIn in, int nframes)
{
    if (multi_check_files(m) != 0) return -1;
    const bool segs = !m->part[0]->seg_off.empty() || !m->part[0]->pl_off.empty();
    if (segs && nframes > 0 && nframes <= m->part[0]->maxF)
        for (size_t k = 0; k < m->part.size(); k++)
            if (check_counts(m->part[k], nframes, m->first[k]) != 0 || check_image(m->part[k], nframes, in.sample_bytes(), m->first[k]) != 0) return -1;
    std::vector<int> st(m->part.size(), 0);
    const int rc = multi_fanout(m, in.p != nullptr, nframes, hx_multi_out_stride(m, nframes), [&](size_t k) {
        const char *p = (const char *) in.p + (segs ? 0 : in.bytes(m->first[k], nframes, m->nchan));
        st[k] = encode_host_files(m->part[k], {p, in.f32}, nframes);
        return st[k] < 0 ? -1 : 0;
    });
    if (rc != 0) return rc;
    int v = 0;
    for (int x : st) v |= x;
    return v;
}
extern "C" int hx_multi_encode_s16_host_files(hx_multi *m, const int16_t *pcm, int nframes) { return multi_encode_host_files(m, {pcm, false}, nframes); }
extern "C" int hx_multi_encode_f32_host_files(hx_multi *m, const float *pcm, int nframes) { return multi_encode_host_files(m, {pcm, true}, nframes); }
extern "C" int hx_multi_encode_src_files_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                                              const int *nfr, long long *in_used)
{
    if (multi_check_files(m) != 0) return -1;
    if (nframes > 0 && in_stride > 0) {
        if (check_counts_arg(nfr, m->S, nframes, 0) != 0) return -1;
        for (size_t k = 0; k < m->part.size(); k++) {
            const long long f = m->first[k];
            if (!m->part[k]->nsrc) { set_err("not a converting batch (hx_multi_create_src)"); return -1; }
            if (src_extents(m->part[k], in_stride, frame_off ? frame_off + f * nframes : nullptr, nframes, nfr ? nfr + f : nullptr, (int) f, nullptr) != 0) return -1;
        }
    }
    std::vector<int> st(m->part.size(), 0);
    const int rc = multi_fanout(m, in != nullptr, nframes, hx_multi_out_stride(m, nframes), [&](size_t k) {
        const long long f = m->first[k];
        st[k] = hx_batch_encode_src_files_host(m->part[k], in + f * in_stride, in_stride, frame_off ? frame_off + f * nframes : nullptr, nframes,
                                               nfr ? nfr + f : nullptr, in_used ? in_used + f : nullptr);
        return st[k] < 0 ? -1 : 0;
    });
    if (rc != 0) return rc;
    int v = 0;
    for (int x : st) v |= x;
    return v;
}

extern "C" int hx_multi_status(hx_multi *m)
{
    int v = 0;
    if (!m) return -1;
    for (hx_batch *b : m->part) v |= hx_batch_status(b);
    return v;
}
