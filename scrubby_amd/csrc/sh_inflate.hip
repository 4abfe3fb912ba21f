// sh_inflate.hip — BGZF members inflated on the device: the decoder behind .gz inputs.
//
// A BGZF file is a chain of gzip members of at most 64 KiB that refer to nothing before themselves; the host finds them by hopping from
// header to header (shin_bgzf_scan) and hands the kernel one descriptor per member.
//
//   k_inflate_member  one wave per member, members taken off a ticket.  Huffman decoding is serial, so the wave decodes wave-uniformly:
//                     every lane runs shin_inflate_member (sh_inflate.h, the code the host tests check) on the same values, what comes
//                     out of LDS is made scalar again, and the decode tables, a 1-KiB window of the compressed bytes (filled by all
//                     lanes) and a batch of 64 tokens live in LDS.  A full batch is written by all 64 lanes: a prefix sum of the token
//                     lengths gives every token its place, literals go out one byte per lane, and the matches are then copied in token
//                     order by the whole wave, byte i from out[pos - dist + i % dist], so a match that overlaps itself reads only bytes
//                     before its own first.  A match that reads bytes stored since the last fence (literals of this batch, an earlier
//                     match) waits for them first.  A stored block is copied by the wave.  At the end each lane takes the CRC-32 of
//                     an equal piece of the member's output and the pieces are combined as zlib's crc32_combine combines them.
//                     The kernel writes (status, crc, bytes produced, blocks by type) per member; the host compares with the trailers.
//
// Bounds: the decoder asks the source only for bytes below in_len and calls the sink only for bytes below out_len (ISIZE, untrusted) and
// distances inside what the member has produced; the host refuses extents that leave the buffers it was given before any launch.
#include "sh_common.h"
#include "sh_codec.h"
#include "sh_inflate.h"
#include "sh_wave.h"
#include <algorithm>
#include <atomic>
#include <chrono>

static_assert(sizeof(ShinMember) == sizeof(sh_gz_member) && offsetof(ShinMember, in_len) == offsetof(sh_gz_member, in_len) &&
              offsetof(ShinMember, status) == offsetof(sh_gz_member, status), "ShinMember is sh_gz_member");

namespace {

constexpr uint32_t INF_WIN = 1024;           // the window of compressed bytes in LDS
constexpr uint32_t INF_BATCH = 64;           // tokens per flush
constexpr uint32_t INF_WAVES_PER_CU = 16;    // 6.1 KiB of LDS and 79 VGPRs a wave: 24 fit a CU; the ticket makes a grid beyond what is resident pointless

struct InfDesc { uint64_t in_off, out_off; uint32_t in_len, out_len; };
struct InfRes { uint32_t status, crc, produced, n_stored, n_fixed, n_dynamic; };

struct DevSrc {
    const uint8_t *in;
    uint8_t *win;
    uint32_t in_len, base, lane;
    __device__ void load(uint32_t pos)
    {
        __syncthreads();
        base = pos;
        for (uint32_t i = lane; i < INF_WIN && i < in_len - base; i += 64) win[i] = in[base + i];
        __syncthreads();
    }
    __device__ uint32_t byte(uint32_t pos)      // pos < in_len
    {
        if (pos - base >= INF_WIN) load(pos);
        return SHIN_UNI(win[pos - base]);
    }
};

struct DevSink {
    uint8_t *out;             // the member's first output byte
    const uint8_t *in;
    uint32_t *tok;            // LDS, INF_BATCH
    uint32_t pos, n_tok, lane;
    __device__ void flush()
    {
        __syncthreads();      // the tokens are in LDS, and every byte stored so far is visible to the wave
        const bool have = lane < n_tok;
        const uint32_t t = have ? tok[lane] : 0;
        const bool is_match = have && (t & 0x80000000u);
        const uint32_t mylen = !have ? 0 : is_match ? (t & 0xffu) + 3 : 1;
        const uint32_t incl = (uint32_t)wave_scan_add_incl((int32_t)mylen), off = incl - mylen;
        const uint32_t total = (uint32_t)wave_bcast((int32_t)incl, 63);
        if (have && !is_match) out[pos + off] = (uint8_t)t;
        uint32_t visible = pos;      // bytes below are visible; the literals above and the matches below are in flight until the next fence
        for (uint64_t todo = __ballot(is_match); todo; todo &= todo - 1) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            const uint32_t mt = (uint32_t)wave_bcast((int32_t)t, l), p = pos + (uint32_t)wave_bcast((int32_t)off, l);
            const uint32_t len = (mt & 0xffu) + 3, dist = ((mt >> 8) & 0x7fffu) + 1;
            const uint32_t src = p - dist, src_end = src + (len < dist ? len : dist);
            if (src_end > visible) { __syncthreads(); visible = p; }
            for (uint32_t i = lane; i < len; i += 64) out[p + i] = out[src + (dist >= len ? i : i % dist)];
        }
        pos += total;
        n_tok = 0;
        __syncthreads();
    }
    __device__ void lit(uint32_t c)
    {
        if (lane == 0) tok[n_tok] = c;
        if (++n_tok == INF_BATCH) flush();
    }
    __device__ void match(uint32_t len, uint32_t dist)
    {
        if (lane == 0) tok[n_tok] = 0x80000000u | (dist - 1) << 8 | (len - 3);
        if (++n_tok == INF_BATCH) flush();
    }
    __device__ void raw(uint32_t in_pos, uint32_t n)
    {
        if (n_tok) flush();
        for (uint32_t i = lane; i < n; i += 64) out[pos + i] = in[in_pos + i];
        pos += n;
    }
};

__global__ __launch_bounds__(64) void k_inflate_member(const uint8_t *__restrict__ d_in, const InfDesc *__restrict__ desc, uint32_t n_members, uint8_t *d_out,
                                                       InfRes *__restrict__ res, uint32_t *__restrict__ ticket)
{
    __shared__ ShinTables s_tab;
    __shared__ uint8_t s_win[INF_WIN];
    __shared__ uint32_t s_tok[INF_BATCH];
    __shared__ uint32_t s_crc[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) s_crc[i] = shin_crc_table_entry(i);
    __syncthreads();
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(ticket, 1u);
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        if (m >= n_members) break;
        const InfDesc d = desc[m];
        const uint8_t *in = d_in + d.in_off;
        uint8_t *out = d_out + d.out_off;
        DevSrc src{in, s_win, d.in_len, 0, lane};
        if (d.in_len) src.load(0);
        DevSink sink{out, in, s_tok, 0, 0, lane};
        ShinResult r;
        shin_inflate_member(src, d.in_len, sink, d.out_len, &s_tab, &r);
        uint32_t crc = 0;
        if (r.status == SHIN_OK) {
            if (sink.n_tok) sink.flush();
            __syncthreads();
            const uint32_t n = r.produced, piece = (n + 63) / 64;
            const uint32_t lo = lane * piece < n ? lane * piece : n, hi = lo + piece < n ? lo + piece : n;
            if (hi > lo) crc = shin_crc_shift(shin_crc_piece(s_crc, out + lo, hi - lo), n - hi);
            for (int k = 1; k < 64; k <<= 1) crc ^= (uint32_t)__shfl_xor((int)crc, k);
        }
        if (lane == 0) res[m] = InfRes{r.status, crc, r.produced, r.n_stored, r.n_fixed, r.n_dynamic};
        __syncthreads();
    }
}

const char *status_name(uint32_t s)
{
    static const char *const names[] = {"ok", "bad block type", "bad code lengths", "invalid symbol", "distance too far back", "input overrun", "output overrun",
                                        "output short of ISIZE", "stored LEN/NLEN mismatch", "CRC mismatch"};
    return s < sizeof names / sizeof *names ? names[s] : "unknown";
}

// The inflater's device for the length of a call; the calling thread's current device is put back on every way out.  Readers
// (shc::In) call from threads that work on another device: their allocations and launches after a read must not move.
struct DeviceScope {
    int prev = 0;
    bool have = false;
    hipError_t err;
    explicit DeviceScope(int device)
    {
        have = hipGetDevice(&prev) == hipSuccess;
        err = hipSetDevice(device);
    }
    ~DeviceScope() { if (have) hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
};

}      // namespace

struct sh_inflater {
    int32_t device = 0;
    uint64_t max_in = 0, max_out = 0, max_members = 0;
    uint32_t max_grid = 0;
    InfDesc *d_desc = nullptr, *h_desc = nullptr;      // h_*: pinned
    InfRes *d_res = nullptr, *h_res = nullptr;
    uint32_t *d_ticket = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the staging of sh_gunzip_bgzf, allocated by its first call
    uint8_t *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
    hipStream_t stream = nullptr;
};

extern "C" sh_status sh_bgzf_scan(const uint8_t *buf, uint64_t n, sh_gz_member *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed, int32_t *stopped)
{
    SH_CHECK((buf || n == 0) && (members || cap == 0) && n_members && consumed && stopped, SH_ERR_BAD_ARG, "sh_bgzf_scan: null argument");
    *stopped = shin_bgzf_scan(buf, n, (ShinMember *)members, cap, n_members, consumed);
    return SH_OK;
}

extern "C" sh_status sh_inflater_free(sh_inflater *inf)
{
    if (!inf) return SH_OK;
    DeviceScope scope(inf->device);
    if (inf->d_desc) hipFree(inf->d_desc);
    if (inf->d_res) hipFree(inf->d_res);
    if (inf->d_ticket) hipFree(inf->d_ticket);
    if (inf->h_desc) hipHostFree(inf->h_desc);
    if (inf->h_res) hipHostFree(inf->h_res);
    if (inf->d_in) hipFree(inf->d_in);
    if (inf->d_out) hipFree(inf->d_out);
    if (inf->h_in) hipHostFree(inf->h_in);
    if (inf->h_out) hipHostFree(inf->h_out);
    if (inf->ev0) hipEventDestroy(inf->ev0);
    if (inf->ev1) hipEventDestroy(inf->ev1);
    if (inf->stream) hipStreamDestroy(inf->stream);
    delete inf;
    return SH_OK;
}

extern "C" sh_status sh_inflater_create(int32_t device, uint64_t max_in_bytes, uint64_t max_out_bytes, uint64_t max_members, sh_inflater **out)
{
    SH_CHECK(out, SH_ERR_BAD_ARG, "sh_inflater_create: null argument");
    *out = nullptr;
    SH_CHECK(max_members >= 1 && max_members < (1ull << 31), SH_ERR_BAD_ARG, "sh_inflater_create: %llu members are not what one launch takes", (unsigned long long)max_members);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || n_dev <= device) { sh_set_error("no HIP device %d", device); return SH_ERR_NO_DEVICE; }
    DeviceScope scope(device);
    SH_HIP(scope.err);
    int n_cu = 0;
    SH_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    sh_inflater *inf = new sh_inflater;
    inf->device = device; inf->max_in = max_in_bytes; inf->max_out = max_out_bytes; inf->max_members = max_members;
    inf->max_grid = (uint32_t)std::max(1, n_cu) * INF_WAVES_PER_CU;
    auto fail = [&](hipError_t e, const char *what, uint64_t bytes) {
        sh_set_error("sh_inflater_create: %s of %llu bytes -> %s", what, (unsigned long long)bytes, hipGetErrorString(e));
        sh_inflater_free(inf);
        return e == hipErrorOutOfMemory ? SH_ERR_OOM : SH_ERR_HIP;
    };
    hipError_t e;
    uint64_t bytes = max_members * sizeof(InfDesc);
    if ((e = hipMalloc(&inf->d_desc, bytes)) != hipSuccess) return fail(e, "member descriptors", bytes);
    if ((e = hipHostMalloc(&inf->h_desc, bytes)) != hipSuccess) return fail(e, "pinned member descriptors", bytes);
    bytes = max_members * sizeof(InfRes);
    if ((e = hipMalloc(&inf->d_res, bytes)) != hipSuccess) return fail(e, "member results", bytes);
    if ((e = hipHostMalloc(&inf->h_res, bytes)) != hipSuccess) return fail(e, "pinned member results", bytes);
    if ((e = hipMalloc(&inf->d_ticket, 4)) != hipSuccess) return fail(e, "ticket", 4);
    if ((e = hipEventCreate(&inf->ev0)) != hipSuccess || (e = hipEventCreate(&inf->ev1)) != hipSuccess) return fail(e, "events", 0);
    *out = inf;
    return SH_OK;
}

extern "C" sh_status sh_inflate_members_device(sh_inflater *inf, const uint8_t *d_in, sh_gz_member *members, uint64_t n_members, uint8_t *d_out, uint64_t out_cap,
                                               void *stream, sh_inflate_stats *stats)
{
    SH_CHECK(inf && (members || n_members == 0), SH_ERR_BAD_ARG, "sh_inflate_members_device: null argument");
    SH_CHECK(n_members <= inf->max_members, SH_ERR_BAD_ARG, "sh_inflate_members_device: %llu members, the inflater was made for %llu", (unsigned long long)n_members,
             (unsigned long long)inf->max_members);
    if (stats) memset(stats, 0, sizeof *stats);
    uint64_t in_end = 0, in_bytes = 0, out_bytes = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        const sh_gz_member &m = members[i];
        SH_CHECK(m.out_len <= SHIN_MAX_ISIZE, SH_ERR_BAD_ARG, "sh_inflate_members_device: member %llu at file offset %llu has ISIZE %u, a BGZF member holds at most %u",
                 (unsigned long long)i, (unsigned long long)m.file_off, m.out_len, SHIN_MAX_ISIZE);
        SH_CHECK(m.in_off <= inf->max_in && m.in_len <= inf->max_in - m.in_off, SH_ERR_BAD_ARG,
                 "sh_inflate_members_device: member %llu at file offset %llu ends at input byte %llu, the inflater was made for %llu", (unsigned long long)i,
                 (unsigned long long)m.file_off, (unsigned long long)(m.in_off + m.in_len), (unsigned long long)inf->max_in);
        in_end = std::max(in_end, m.in_off + m.in_len);
        in_bytes += m.in_len; out_bytes += m.out_len;
    }
    SH_CHECK(out_bytes <= inf->max_out, SH_ERR_BAD_ARG, "sh_inflate_members_device: %llu bytes out, the inflater was made for %llu", (unsigned long long)out_bytes,
             (unsigned long long)inf->max_out);
    SH_CHECK(out_bytes <= out_cap, SH_ERR_BAD_ARG, "sh_inflate_members_device: room for %llu bytes, the members hold %llu", (unsigned long long)out_cap, (unsigned long long)out_bytes);
    SH_CHECK((d_in || in_end == 0) && (d_out || out_bytes == 0), SH_ERR_BAD_ARG, "sh_inflate_members_device: null argument");
    for (uint64_t i = 0; i < n_members; ++i) members[i].status = SHIN_OK;
    if (n_members == 0) return SH_OK;
    hipStream_t hs = (hipStream_t)stream;
    DeviceScope scope(inf->device);
    SH_HIP(scope.err);
    uint64_t off = 0;
    for (uint64_t i = 0; i < n_members; ++i) { inf->h_desc[i] = InfDesc{members[i].in_off, off, members[i].in_len, members[i].out_len}; off += members[i].out_len; }
    SH_HIP(hipMemcpyAsync(inf->d_desc, inf->h_desc, n_members * sizeof(InfDesc), hipMemcpyHostToDevice, hs));
    SH_HIP(hipMemsetAsync(inf->d_ticket, 0, 4, hs));
    SH_HIP(hipEventRecord(inf->ev0, hs));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_members, inf->max_grid);
    k_inflate_member<<<grid, 64, 0, hs>>>(d_in, inf->d_desc, (uint32_t)n_members, d_out, inf->d_res, inf->d_ticket);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(inf->ev1, hs));
    SH_HIP(hipMemcpyAsync(inf->h_res, inf->d_res, n_members * sizeof(InfRes), hipMemcpyDeviceToHost, hs));
    SH_HIP(hipStreamSynchronize(hs));
    float ms = 0;
    SH_HIP(hipEventElapsedTime(&ms, inf->ev0, inf->ev1));
    uint64_t first_bad = n_members, n_st = 0, n_fx = 0, n_dy = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        const InfRes &r = inf->h_res[i];
        uint32_t st = r.status;
        if (st == SHIN_OK && r.crc != members[i].crc32) st = SHIN_CRC;
        members[i].status = st;
        if (st != SHIN_OK && first_bad == n_members) first_bad = i;
        n_st += r.n_stored; n_fx += r.n_fixed; n_dy += r.n_dynamic;
    }
    if (stats) {
        stats->n_members = n_members; stats->n_stored_blocks = n_st; stats->n_fixed_blocks = n_fx; stats->n_dynamic_blocks = n_dy;
        stats->in_bytes = in_bytes; stats->out_bytes = out_bytes; stats->ms = ms;
    }
    SH_CHECK(first_bad == n_members, SH_ERR_IO, "gzip member at file offset %llu does not inflate: status %u (%s)", (unsigned long long)members[first_bad].file_off,
             members[first_bad].status, status_name(members[first_bad].status));
    return SH_OK;
}

sh_status shi_gunzip_members(sh_inflater *inf, const uint8_t *in, uint64_t n, sh_gz_member *members, uint64_t n_members, uint8_t *out, uint8_t *d_out, uint64_t out_cap,
                             uint64_t *out_len, sh_inflate_stats *stats)
{
    SH_CHECK(n <= inf->max_in, SH_ERR_BAD_ARG, "sh_gunzip_bgzf: %llu bytes, the inflater was made for %llu", (unsigned long long)n, (unsigned long long)inf->max_in);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        SH_CHECK(members[i].in_off <= n && members[i].in_len <= n - members[i].in_off, SH_ERR_BAD_ARG, "sh_gunzip_bgzf: member %llu leaves the buffer of %llu bytes",
                 (unsigned long long)i, (unsigned long long)n);
        total += members[i].out_len;
    }
    SH_CHECK(total <= out_cap, SH_ERR_BAD_ARG, "sh_gunzip_bgzf: room for %llu bytes, the members hold %llu", (unsigned long long)out_cap, (unsigned long long)total);
    DeviceScope scope(inf->device);
    SH_HIP(scope.err);
    if (!inf->stream) SH_HIP(hipStreamCreateWithFlags(&inf->stream, hipStreamNonBlocking));
    if (!inf->d_in) SH_HIP(hipMalloc(&inf->d_in, inf->max_in + 16));
    if (!inf->h_in) SH_HIP(hipHostMalloc(&inf->h_in, inf->max_in + 16));
    if (!d_out) {
        if (!inf->d_out) SH_HIP(hipMalloc(&inf->d_out, inf->max_out + 16));
        if (!inf->h_out) SH_HIP(hipHostMalloc(&inf->h_out, inf->max_out + 16));
    }
    if (n) {
        memcpy(inf->h_in, in, n);
        SH_HIP(hipMemcpyAsync(inf->d_in, inf->h_in, n, hipMemcpyHostToDevice, inf->stream));
    }
    const sh_status rc = sh_inflate_members_device(inf, inf->d_in, members, n_members, d_out ? d_out : inf->d_out, d_out ? out_cap : std::min(out_cap, inf->max_out),
                                                   inf->stream, stats);
    if (rc != SH_OK) { hipStreamSynchronize(inf->stream); return rc; }      // a refused call leaves no copy out of h_in in flight for the next one to overwrite
    if (!d_out && total) {
        SH_HIP(hipMemcpyAsync(inf->h_out, inf->d_out, total, hipMemcpyDeviceToHost, inf->stream));
        SH_HIP(hipStreamSynchronize(inf->stream));
        memcpy(out, inf->h_out, total);
    }
    if (out_len) *out_len = total;
    return SH_OK;
}

extern "C" sh_status sh_gunzip_bgzf(sh_inflater *inf, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len, sh_inflate_stats *stats)
{
    SH_CHECK(inf && out_len && (in || n == 0) && (out || out_cap == 0), SH_ERR_BAD_ARG, "sh_gunzip_bgzf: null argument");
    *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    SH_CHECK(n <= inf->max_in, SH_ERR_BAD_ARG, "sh_gunzip_bgzf: %llu bytes, the inflater was made for %llu", (unsigned long long)n, (unsigned long long)inf->max_in);
    std::vector<sh_gz_member> members(inf->max_members);
    uint64_t n_members = 0, consumed = 0;
    const int stopped = shin_bgzf_scan(in, n, (ShinMember *)members.data(), inf->max_members, &n_members, &consumed);
    SH_CHECK(consumed == n || stopped != 0, SH_ERR_BAD_ARG, "sh_gunzip_bgzf: more than %llu members, the inflater was made for that many", (unsigned long long)inf->max_members);
    SH_CHECK(consumed == n, SH_ERR_IO, "sh_gunzip_bgzf: %s at offset %llu", stopped == 1 ? "incomplete member" : "not a BGZF member", (unsigned long long)consumed);
    return shi_gunzip_members(inf, in, n, members.data(), n_members, out, nullptr, out_cap, out_len, stats);
}

// ---- the per-process pool behind shc::In (sh_codec.h) and the index build, and what a run reports ------------------------------------
namespace shc {

namespace {
std::mutex g_mu;
std::vector<sh_inflater *> g_idle;
std::atomic<int> g_device{0}, g_depth{0};
std::atomic<bool> g_said{false};
std::atomic<uint64_t> g_members{0}, g_bytes{0}, g_zlib_files{0}, g_created{0};
}

bool gunzip_device_wanted() { const char *e = getenv("SCRUBBY_HIP_GUNZIP_DEVICE"); return e && e[0] == '1' && e[1] == 0; }

// The device a reader's inflater works on: the run's while a run is open (its reader threads never set a device of their own), else
// the calling thread's current one.  A reader's output is host memory, so the choice decides where the work is done, never what is read.
int gunzip_reader_device()
{
    if (g_depth.load() > 0) return g_device.load();
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}

// the pool is keyed by device: an inflater of another device is neither handed out nor made
sh_inflater *gunzip_pool_acquire(int device)
{
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (size_t i = 0; i < g_idle.size(); ++i)
            if (g_idle[i]->device == device) { sh_inflater *inf = g_idle[i]; g_idle.erase(g_idle.begin() + (long)i); return inf; }
    }
    sh_inflater *inf = nullptr;
    if (sh_inflater_create(device, GUNZIP_WINDOW_BYTES, GUNZIP_OUT_BYTES, GUNZIP_MAX_MEMBERS, &inf) != SH_OK) return nullptr;
    ++g_created;
    return inf;
}

void gunzip_pool_release(sh_inflater *inf)
{
    if (!inf) return;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_idle.size() < 4) { g_idle.push_back(inf); return; }
    sh_inflater_free(inf);
}

void gunzip_note_zlib(const char *path, uint64_t file_off, const char *why)
{
    ++g_zlib_files;
    if (!g_said.exchange(true))
        fprintf(stderr, "[scrubby-hip] SCRUBBY_HIP_GUNZIP_DEVICE: %s at offset %llu: %s; zlib inflates what the device does not\n", path, (unsigned long long)file_off, why);
}

void gunzip_count(uint64_t members, uint64_t bytes) { g_members += members; g_bytes += bytes; }

GunzipRun::GunzipRun(int device)
{
    if (g_depth.fetch_add(1) == 0) { g_device = device; g_members = 0; g_bytes = 0; g_zlib_files = 0; }
}

GunzipRun::~GunzipRun()
{
    if (g_depth.fetch_sub(1) != 1 || !gunzip_device_wanted()) return;
    if (const char *e = getenv("SCRUBBY_HIP_DBG_HOST")) if (*e == '1')
        fprintf(stderr, "[scrubby-hip] gunzip on the device: %llu members, %llu bytes out, %llu files through zlib\n", (unsigned long long)g_members.load(),
                (unsigned long long)g_bytes.load(), (unsigned long long)g_zlib_files.load());
}

}      // namespace shc
