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
#include "sh_gunzip.h"
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
                                        "output short of ISIZE", "stored LEN/NLEN mismatch", "CRC mismatch", "end of the stream", "too many members in one span",
                                        "bad gzip header", "second decode differs from the first", "ISIZE mismatch"};
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
    // the scratch of the general-gzip path (sh_gunzip_*), allocated by the first sh_gunzip_open
    struct GzScratch *gz = nullptr;
};

static void gz_scratch_free(struct GzScratch *sc);

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
    gz_scratch_free(inf->gz);
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

// the pinned staging of the calls that take host memory, allocated by the first of them (the inflater's device is current)
static sh_status inf_staging(sh_inflater *inf, bool with_out)
{
    if (!inf->stream) SH_HIP(hipStreamCreateWithFlags(&inf->stream, hipStreamNonBlocking));
    if (!inf->d_in) SH_HIP(hipMalloc(&inf->d_in, inf->max_in + 16));
    if (!inf->h_in) SH_HIP(hipHostMalloc(&inf->h_in, inf->max_in + 16));
    if (with_out) {
        if (!inf->d_out) SH_HIP(hipMalloc(&inf->d_out, inf->max_out + 16));
        if (!inf->h_out) SH_HIP(hipHostMalloc(&inf->h_out, inf->max_out + 16));
    }
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
    const sh_status staged = inf_staging(inf, !d_out);
    if (staged != SH_OK) return staged;
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

// ---- any gzip stream (sh_gunzip_*): the stages of shgz::feed (sh_gunzip.h) as kernels ----------------------------------------------------
//
//   k_gz_find     one wave per chunk j >= 1 off a ticket.  The lanes test 64 consecutive bit positions at a time with shin_candidate_quick
//                 (plain arithmetic on 128 bits out of an LDS window); what passes is then decided one position at a time, in order,
//                 by the whole wave with shin_block_candidate, the decoder's own header checks.  The first candidate ends the chunk.
//   k_gz_size     one wave per job off a ticket: shin_inflate_span with the sink that only counts.  LDS as k_inflate_member less the tokens.
//   k_gz_markers  the same decode of the chain's spans with the marker sink: 16-bit symbols, a batch of 64 tokens written by the wave.
//   k_gz_tails    one block per span: where the span's last 32 KiB hold no marker they are the window behind it, written at once.
//   k_gz_windows  ONE block; span after span it writes the 32 KiB that end with the span from the span's symbols and the 32 KiB before,
//                 but for the spans k_gz_tails settled.
//   k_gz_resolve  one block per span: symbols to bytes with the span's incoming window, and the CRC-32 of each of its pieces.
// Every dependency is a launch boundary.  Bounds: the decoder reads input below in_len only; the marker pass is given the size pass's
// byte count as its output extent, so it cannot write past the place the host laid out for it; windows and resolve index by the host's
// items alone, and a marker indexes the 32 KiB window by its low 15 bits.
namespace {

constexpr uint32_t GZ_FWIN = 2048;           // the finder's window of compressed bytes in LDS
constexpr uint32_t GZ_FNEED = 24;            // bytes a lane reads from its position's byte on

__global__ __launch_bounds__(64) void k_gz_find(const uint8_t *__restrict__ d_in, uint32_t in_len, uint32_t chunk_bytes, uint32_t n_chunks, uint64_t *__restrict__ found,
                                                uint32_t *__restrict__ ticket)
{
    __shared__ ShinTables s_tab;
    __shared__ uint8_t s_win[INF_WIN];
    __shared__ uint8_t s_fwin[GZ_FWIN];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        uint32_t j = 0;
        if (lane == 0) j = atomicAdd(ticket, 1u);
        j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j) + 1;
        if (j >= n_chunks) break;
        const uint64_t lo_bit = 8ull * chunk_bytes * j, n_bits = 8ull * in_len, hi_bit = lo_bit + 8ull * chunk_bytes < n_bits ? lo_bit + 8ull * chunk_bytes : n_bits;
        DevSrc src{d_in, s_win, in_len, 0, lane};
        src.load((uint32_t)(lo_bit >> 3));      // j < n_chunks: the chunk's first byte is inside the input
        uint64_t hit = SHIN_NO_START;
        uint32_t fbase = 0, fend = 0;           // s_fwin holds input bytes [fbase, fend), zeros behind the input
        for (uint64_t g = lo_bit; g < hi_bit && hit == SHIN_NO_START; g += 64) {
            const uint32_t byte0 = (uint32_t)(g >> 3);
            if (byte0 + 8 + GZ_FNEED > fend) {
                __syncthreads();
                fbase = byte0; fend = byte0 + GZ_FWIN;
                for (uint32_t i = lane; i < GZ_FWIN; i += 64) s_fwin[i] = (uint64_t)fbase + i < in_len ? d_in[fbase + i] : (uint8_t)0;
                __syncthreads();
            }
            const uint64_t p = g + lane;
            const uint32_t k = (uint32_t)(p & 7), off = (uint32_t)(p >> 3) - fbase;      // off + 24 <= GZ_FWIN
            uint64_t w[3];
            for (uint32_t q = 0; q < 3; ++q) {
                uint64_t v = 0;
                for (uint32_t i = 0; i < 8; ++i) v |= (uint64_t)s_fwin[off + 8 * q + i] << (8 * i);
                w[q] = v;
            }
            const uint64_t lo = k ? w[0] >> k | w[1] << (64 - k) : w[0], hi = k ? w[1] >> k | w[2] << (64 - k) : w[1];
            const uint32_t quick = p < hi_bit ? shin_candidate_quick(lo, hi, n_bits - p, k) : 0;
            for (uint64_t todo = __ballot(quick != 0); todo && hit == SHIN_NO_START; todo &= todo - 1) {
                const int l = __ffsll((unsigned long long)todo) - 1;
                const uint32_t ql = (uint32_t)wave_bcast((int32_t)quick, l);
                if (ql == 2 || shin_block_candidate(src, in_len, g + (uint32_t)l, &s_tab)) hit = g + (uint32_t)l;
            }
        }
        if (lane == 0) found[j] = hit;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_gz_size(const uint8_t *__restrict__ d_in, uint32_t in_len, uint32_t in_is_end, const shgz::Job *__restrict__ jobs, uint32_t n_jobs,
                                                ShinSpan *__restrict__ res, uint32_t *__restrict__ ticket)
{
    __shared__ ShinTables s_tab;
    __shared__ uint8_t s_win[INF_WIN];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(ticket, 1u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        if (i >= n_jobs) break;
        const shgz::Job job = jobs[i];
        DevSrc src{d_in, s_win, in_len, 0, lane};
        src.load(0);      // in_len > 0
        ShinSizeSink sink;
        ShinSpan r;
        shin_inflate_span(src, in_len, in_is_end != 0, job.start_bit, job.at_header != 0, job.stop_bit, sink, SHIN_SPAN_MAX_OUT, &s_tab, &r, res[i].ends);
        if (lane == 0) { res[i].status = r.status; res[i].produced = r.produced; res[i].n_ends = r.n_ends; res[i].pad = 0; res[i].end_bit = r.end_bit; }
        __syncthreads();
    }
}

// DevSink for 16-bit symbols: a source before the span's first symbol gives a marker
struct DevMarkSink {
    uint16_t *out;            // the span's first symbol
    const uint8_t *in;
    uint32_t *tok;            // LDS, INF_BATCH
    uint32_t pos, n_tok, lane;
    __device__ uint16_t from(uint32_t at, uint32_t dist) const { return at < dist ? (uint16_t)shin_marker(at, dist) : out[at - dist]; }
    __device__ void flush()
    {
        __syncthreads();
        const bool have = lane < n_tok;
        const uint32_t t = have ? tok[lane] : 0;
        const bool is_match = have && (t & 0x80000000u);
        const uint32_t mylen = !have ? 0 : is_match ? (t & 0xffu) + 3 : 1;
        const uint32_t incl = (uint32_t)wave_scan_add_incl((int32_t)mylen), off = incl - mylen;
        const uint32_t total = (uint32_t)wave_bcast((int32_t)incl, 63);
        if (have && !is_match) out[pos + off] = (uint16_t)(t & 0xffu);
        uint32_t visible = pos;
        for (uint64_t todo = __ballot(is_match); todo; todo &= todo - 1) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            const uint32_t mt = (uint32_t)wave_bcast((int32_t)t, l), p = pos + (uint32_t)wave_bcast((int32_t)off, l);
            const uint32_t len = (mt & 0xffu) + 3, dist = ((mt >> 8) & 0x7fffu) + 1;
            const uint32_t span = len < dist ? len : dist;      // symbols [p - dist, p - dist + span) are read, those before the span as markers
            if (p + span > dist && p + span - dist > visible) { __syncthreads(); visible = p; }
            for (uint32_t i = lane; i < len; i += 64) out[p + i] = from(p + (dist >= len ? i : i % dist), dist);
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

__global__ __launch_bounds__(64) void k_gz_markers(const uint8_t *__restrict__ d_in, uint32_t in_len, uint32_t in_is_end, const shgz::Item *__restrict__ items, uint32_t n_items,
                                                   uint16_t *d_sym, ShinSpan *__restrict__ res, uint32_t *__restrict__ ticket)
{
    __shared__ ShinTables s_tab;
    __shared__ uint8_t s_win[INF_WIN];
    __shared__ uint32_t s_tok[INF_BATCH];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(ticket, 1u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        if (i >= n_items) break;
        const shgz::Item it = items[i];
        DevSrc src{d_in, s_win, in_len, 0, lane};
        src.load(0);
        DevMarkSink sink{d_sym + it.out_off, d_in, s_tok, 0, 0, lane};
        ShinSpan r;
        shin_inflate_span(src, in_len, in_is_end != 0, it.start_bit, it.at_header != 0, it.stop_bit, sink, it.produced, &s_tab, &r, res[i].ends);      // it.produced: the extent
        if (sink.n_tok) sink.flush();
        if (lane == 0) { res[i].status = r.status; res[i].produced = r.produced; res[i].n_ends = r.n_ends; res[i].pad = 0; res[i].end_bit = r.end_bit; }
        __syncthreads();
    }
}

constexpr uint32_t GZ_WIN_THREADS = 1024, GZ_RES_THREADS = 256;

// One block per span: a span of 32 KiB or more whose last 32 KiB hold no marker gives the window behind it without the window before
// it, so it is written here, by all such spans at once, and k_gz_windows passes over it: the chain is broken there for free.
__global__ __launch_bounds__(GZ_RES_THREADS) void k_gz_tails(const uint16_t *__restrict__ d_sym, const shgz::Item *__restrict__ items, uint8_t *wins, uint32_t *__restrict__ is_free)
{
    __shared__ uint32_t s_marker;
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const shgz::Item it = items[i];
    if (it.produced < SHIN_WINDOW) { if (tid == 0) is_free[i] = 0; return; }
    if (tid == 0) s_marker = 0;
    __syncthreads();
    const uint16_t *tail = d_sym + it.out_off + (it.produced - SHIN_WINDOW);
    uint32_t marker = 0;
    for (uint32_t b = tid; b < SHIN_WINDOW; b += GZ_RES_THREADS) marker |= tail[b] >= 256;
    if (marker) atomicOr(&s_marker, 1u);
    __syncthreads();
    const bool free_of_markers = s_marker == 0;
    if (free_of_markers) {
        uint8_t *next = wins + (size_t)(i + 1) * SHIN_WINDOW;
        for (uint32_t b = tid; b < SHIN_WINDOW; b += GZ_RES_THREADS) next[b] = (uint8_t)tail[b];
    }
    if (tid == 0) is_free[i] = free_of_markers;
}

// wins: n_items + 1 windows of 32 KiB; window 0 is what the feed came with, window i + 1 ends with span i's last byte
__global__ __launch_bounds__(GZ_WIN_THREADS) void k_gz_windows(const uint16_t *__restrict__ d_sym, const shgz::Item *__restrict__ items, uint32_t n_items, uint8_t *wins, uint32_t *bad,
                                                               const uint32_t *__restrict__ is_free)
{
    for (uint32_t i = 0; i < n_items; ++i) {
        if (is_free[i]) continue;      // k_gz_tails wrote window i + 1
        const shgz::Item it = items[i];
        const uint8_t *prev = wins + (size_t)i * SHIN_WINDOW;
        uint8_t *next = wins + (size_t)(i + 1) * SHIN_WINDOW;
        uint32_t b_bad = 0;
        for (uint32_t b = threadIdx.x; b < SHIN_WINDOW; b += GZ_WIN_THREADS) next[b] = (uint8_t)shin_window_byte(b, prev, it.valid_in, d_sym + it.out_off, it.produced, &b_bad);
        if (b_bad) bad[i] = b_bad;
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(GZ_RES_THREADS) void k_gz_resolve(const uint16_t *__restrict__ d_sym, const shgz::Item *__restrict__ items, const uint8_t *__restrict__ wins,
                                                               uint8_t *__restrict__ d_out, uint32_t *__restrict__ crc_out, uint32_t *bad, unsigned long long *n_markers)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_part[GZ_RES_THREADS / 64];
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const shgz::Item it = items[i];
    const uint8_t *win = wins + (size_t)i * SHIN_WINDOW;
    const uint16_t *sym = d_sym + it.out_off;
    s_crc[tid] = shin_crc_table_entry(tid);      // GZ_RES_THREADS == 256
    uint32_t b_bad = 0, markers = 0;
    for (uint32_t p = tid; p < it.produced; p += GZ_RES_THREADS) {
        const uint32_t s = sym[p];
        markers += s >= 256;
        d_out[it.out_off + p] = (uint8_t)shin_resolve(s, win, it.valid_in, &b_bad);
    }
    if (b_bad) bad[i] = b_bad;
    if (markers) atomicAdd(n_markers, (unsigned long long)markers);
    __syncthreads();
    for (uint32_t k = 0; k < it.n_seg; ++k) {      // each thread an equal piece of the segment, shifted by the bytes behind it
        const uint32_t lo = it.seg[k], hi = it.seg[k + 1], n = hi - lo, piece = (n + GZ_RES_THREADS - 1) / GZ_RES_THREADS;
        const uint32_t a = lo + (tid * (uint64_t)piece < n ? tid * piece : n), b = a + piece < hi ? a + piece : hi;
        uint32_t c = 0, ignored = 0;
        if (b > a) {
            c = 0xffffffffu;
            for (uint32_t p = a; p < b; ++p) c = s_crc[(c ^ shin_resolve(sym[p], win, it.valid_in, &ignored)) & 0xff] ^ (c >> 8);
            c = shin_crc_shift(~c, hi - b);
        }
        for (int sh = 1; sh < 64; sh <<= 1) c ^= (uint32_t)__shfl_xor((int)c, sh);
        if ((tid & 63) == 0) s_part[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) { for (uint32_t w = 1; w < GZ_RES_THREADS / 64; ++w) c ^= s_part[w]; crc_out[(size_t)i * shgz::MAX_PIECES + k] = c; }
        __syncthreads();
    }
}

}      // namespace

// device and pinned arrays of one feed: max_chunks chunks, sym_cap symbols
struct GzScratch {
    uint32_t max_chunks = 0;
    uint64_t sym_cap = 0;
    uint64_t *d_found = nullptr, *h_found = nullptr;
    shgz::Job *d_jobs = nullptr, *h_jobs = nullptr;
    shgz::Item *d_items = nullptr, *h_items = nullptr;
    ShinSpan *d_res = nullptr, *h_res = nullptr;
    uint32_t *d_crc = nullptr, *h_crc = nullptr, *d_bad = nullptr, *h_bad = nullptr, *d_ticket = nullptr, *d_free = nullptr;
    unsigned long long *d_markers = nullptr, *h_markers = nullptr;
    uint16_t *d_sym = nullptr;
    uint8_t *d_wins = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

static void gz_scratch_free(GzScratch *sc)
{
    if (!sc) return;
    for (void *p : {(void *)sc->d_found, (void *)sc->d_jobs, (void *)sc->d_items, (void *)sc->d_res, (void *)sc->d_crc, (void *)sc->d_bad, (void *)sc->d_ticket, (void *)sc->d_free, (void *)sc->d_markers,
                    (void *)sc->d_sym, (void *)sc->d_wins})
        if (p) hipFree(p);
    for (void *p : {(void *)sc->h_found, (void *)sc->h_jobs, (void *)sc->h_items, (void *)sc->h_res, (void *)sc->h_crc, (void *)sc->h_bad, (void *)sc->h_markers})
        if (p) hipHostFree(p);
    for (hipEvent_t e : sc->ev) if (e) hipEventDestroy(e);
    delete sc;
}

// the inflater's device is current
static sh_status gz_scratch_fill(GzScratch *sc, uint32_t max_chunks, uint64_t sym_cap)
{
    sc->max_chunks = max_chunks; sc->sym_cap = sym_cap;
    const uint64_t c = max_chunks;
    SH_HIP(hipMalloc(&sc->d_found, c * 8)); SH_HIP(hipHostMalloc(&sc->h_found, c * 8));
    SH_HIP(hipMalloc(&sc->d_jobs, c * sizeof(shgz::Job))); SH_HIP(hipHostMalloc(&sc->h_jobs, c * sizeof(shgz::Job)));
    SH_HIP(hipMalloc(&sc->d_items, c * sizeof(shgz::Item))); SH_HIP(hipHostMalloc(&sc->h_items, c * sizeof(shgz::Item)));
    SH_HIP(hipMalloc(&sc->d_res, c * sizeof(ShinSpan))); SH_HIP(hipHostMalloc(&sc->h_res, c * sizeof(ShinSpan)));
    SH_HIP(hipMalloc(&sc->d_crc, c * shgz::MAX_PIECES * 4)); SH_HIP(hipHostMalloc(&sc->h_crc, c * shgz::MAX_PIECES * 4));
    SH_HIP(hipMalloc(&sc->d_bad, c * 4)); SH_HIP(hipHostMalloc(&sc->h_bad, c * 4));
    SH_HIP(hipMalloc(&sc->d_ticket, 4));
    SH_HIP(hipMalloc(&sc->d_free, c * 4));
    SH_HIP(hipMalloc(&sc->d_markers, 8)); SH_HIP(hipHostMalloc(&sc->h_markers, 8));
    SH_HIP(hipMalloc(&sc->d_sym, (sc->sym_cap + 8) * 2));
    SH_HIP(hipMalloc(&sc->d_wins, (c + 1) * SHIN_WINDOW));
    for (hipEvent_t &e : sc->ev) SH_HIP(hipEventCreate(&e));
    return SH_OK;
}

// A scratch for max_chunks chunks.  A larger one replaces the inflater's only once it is complete: an sh_gunzip that is open on the
// inflater reads inf->gz at its next feed, so a failed growth must leave the old scratch in place.
static sh_status gz_scratch_make(sh_inflater *inf, uint32_t max_chunks)
{
    if (inf->gz && inf->gz->max_chunks >= max_chunks) return SH_OK;
    GzScratch *sc = new GzScratch;
    const sh_status rc = gz_scratch_fill(sc, max_chunks, inf->max_out);
    if (rc != SH_OK) { gz_scratch_free(sc); return rc; }
    gz_scratch_free(inf->gz);
    inf->gz = sc;
    return SH_OK;
}

struct sh_gunzip {
    sh_inflater *inf = nullptr;
    shgz::State S;
    uint8_t *d_win = nullptr;      // the 32 KiB of output before the resume point
    bool dead = false;
};

namespace {

#define GZ_HIP(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            sh_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));        \
            return e_ == hipErrorOutOfMemory ? (int)SH_ERR_OOM : (int)SH_ERR_HIP;                     \
        }                                                                                             \
    } while (0)

// the backend of shgz::feed on the device; every stage ends with the stream synchronised, since the host reads what it wrote
struct DevBackend {
    sh_inflater *inf;
    GzScratch *sc;
    sh_gunzip *gz;
    const uint8_t *d_in;
    uint32_t n;
    bool last;
    uint8_t *d_out;
    hipStream_t hs;
    float ms_find = 0, ms_size = 0, ms_markers = 0, ms_windows = 0, ms_resolve = 0;

    uint32_t grid(uint32_t waves) const { return std::max(1u, std::min(waves, inf->max_grid)); }
    int find(uint32_t chunk_bytes, uint32_t n_chunks, uint64_t *found)
    {
        GZ_HIP(hipMemsetAsync(sc->d_ticket, 0, 4, hs));
        GZ_HIP(hipEventRecord(sc->ev[0], hs));
        k_gz_find<<<grid(n_chunks - 1), 64, 0, hs>>>(d_in, n, chunk_bytes, n_chunks, sc->d_found, sc->d_ticket);
        GZ_HIP(hipGetLastError());
        GZ_HIP(hipEventRecord(sc->ev[1], hs));
        GZ_HIP(hipMemcpyAsync(sc->h_found, sc->d_found, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipStreamSynchronize(hs));
        GZ_HIP(hipEventElapsedTime(&ms_find, sc->ev[0], sc->ev[1]));
        for (uint32_t j = 1; j < n_chunks; ++j) found[j] = sc->h_found[j];
        return 0;
    }
    int size(const shgz::Job *jobs, uint32_t n_jobs, ShinSpan *res)
    {
        if (n_jobs == 0) return 0;
        memcpy(sc->h_jobs, jobs, (size_t)n_jobs * sizeof(shgz::Job));
        GZ_HIP(hipMemcpyAsync(sc->d_jobs, sc->h_jobs, (size_t)n_jobs * sizeof(shgz::Job), hipMemcpyHostToDevice, hs));
        GZ_HIP(hipMemsetAsync(sc->d_ticket, 0, 4, hs));
        GZ_HIP(hipMemsetAsync(sc->d_res, 0, (size_t)n_jobs * sizeof(ShinSpan), hs));
        GZ_HIP(hipEventRecord(sc->ev[0], hs));
        k_gz_size<<<grid(n_jobs), 64, 0, hs>>>(d_in, n, last, sc->d_jobs, n_jobs, sc->d_res, sc->d_ticket);
        GZ_HIP(hipGetLastError());
        GZ_HIP(hipEventRecord(sc->ev[1], hs));
        GZ_HIP(hipMemcpyAsync(sc->h_res, sc->d_res, (size_t)n_jobs * sizeof(ShinSpan), hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipStreamSynchronize(hs));
        float ms = 0;
        GZ_HIP(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1]));
        ms_size += ms;
        memcpy(res, sc->h_res, (size_t)n_jobs * sizeof(ShinSpan));
        return 0;
    }
    int decode(const shgz::Item *items, uint32_t m, uint64_t total, ShinSpan *res, uint32_t *bad, uint32_t *crc, uint64_t *n_markers)
    {
        if (total > sc->sym_cap || m > sc->max_chunks) { sh_set_error("sh_gunzip: %llu bytes in %u chunks leave the scratch", (unsigned long long)total, m); return SH_ERR_BAD_ARG; }
        memcpy(sc->h_items, items, (size_t)m * sizeof(shgz::Item));
        GZ_HIP(hipMemcpyAsync(sc->d_items, sc->h_items, (size_t)m * sizeof(shgz::Item), hipMemcpyHostToDevice, hs));
        GZ_HIP(hipMemsetAsync(sc->d_ticket, 0, 4, hs));
        GZ_HIP(hipMemsetAsync(sc->d_res, 0, (size_t)m * sizeof(ShinSpan), hs));
        GZ_HIP(hipMemsetAsync(sc->d_bad, 0, (size_t)m * 4, hs));
        GZ_HIP(hipMemsetAsync(sc->d_markers, 0, 8, hs));
        GZ_HIP(hipMemcpyAsync(sc->d_wins, gz->d_win, SHIN_WINDOW, hipMemcpyDeviceToDevice, hs));
        GZ_HIP(hipEventRecord(sc->ev[0], hs));
        k_gz_markers<<<grid(m), 64, 0, hs>>>(d_in, n, last, sc->d_items, m, sc->d_sym, sc->d_res, sc->d_ticket);
        GZ_HIP(hipGetLastError());
        GZ_HIP(hipEventRecord(sc->ev[1], hs));
        k_gz_tails<<<m, GZ_RES_THREADS, 0, hs>>>(sc->d_sym, sc->d_items, sc->d_wins, sc->d_free);
        GZ_HIP(hipGetLastError());
        k_gz_windows<<<1, GZ_WIN_THREADS, 0, hs>>>(sc->d_sym, sc->d_items, m, sc->d_wins, sc->d_bad, sc->d_free);
        GZ_HIP(hipGetLastError());
        GZ_HIP(hipEventRecord(sc->ev[2], hs));
        k_gz_resolve<<<m, GZ_RES_THREADS, 0, hs>>>(sc->d_sym, sc->d_items, sc->d_wins, d_out, sc->d_crc, sc->d_bad, sc->d_markers);
        GZ_HIP(hipGetLastError());
        GZ_HIP(hipEventRecord(sc->ev[3], hs));
        GZ_HIP(hipMemcpyAsync(sc->h_res, sc->d_res, (size_t)m * sizeof(ShinSpan), hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipMemcpyAsync(sc->h_bad, sc->d_bad, (size_t)m * 4, hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipMemcpyAsync(sc->h_crc, sc->d_crc, (size_t)m * shgz::MAX_PIECES * 4, hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipMemcpyAsync(sc->h_markers, sc->d_markers, 8, hipMemcpyDeviceToHost, hs));
        GZ_HIP(hipMemcpyAsync(gz->d_win, sc->d_wins + (size_t)m * SHIN_WINDOW, SHIN_WINDOW, hipMemcpyDeviceToDevice, hs));
        GZ_HIP(hipStreamSynchronize(hs));
        GZ_HIP(hipEventElapsedTime(&ms_markers, sc->ev[0], sc->ev[1]));
        GZ_HIP(hipEventElapsedTime(&ms_windows, sc->ev[1], sc->ev[2]));
        GZ_HIP(hipEventElapsedTime(&ms_resolve, sc->ev[2], sc->ev[3]));
        memcpy(res, sc->h_res, (size_t)m * sizeof(ShinSpan));
        memcpy(bad, sc->h_bad, (size_t)m * 4);
        memcpy(crc, sc->h_crc, (size_t)m * shgz::MAX_PIECES * 4);
        *n_markers = *sc->h_markers;
        return 0;
    }
};

sh_status gz_feed(sh_gunzip *gz, const uint8_t *d_in, uint64_t n, int32_t last, uint8_t *d_out, uint64_t out_cap, const uint64_t *starts, uint64_t *consumed, uint64_t *out_len,
                  hipStream_t hs, sh_gunzip_stats *stats)
{
    sh_inflater *inf = gz->inf;
    *consumed = 0; *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    SH_CHECK(inf->gz, SH_ERR_BAD_ARG, "sh_gunzip_feed: the inflater has no scratch");
    SH_CHECK(!gz->dead, SH_ERR_BAD_ARG, "sh_gunzip_feed: the stream has ended with a status, it takes no further feed");
    SH_CHECK(n <= inf->max_in && n < (1ull << 32) - 64, SH_ERR_BAD_ARG, "sh_gunzip_feed: %llu bytes, the inflater was made for %llu", (unsigned long long)n, (unsigned long long)inf->max_in);
    SH_CHECK((n + gz->S.chunk_bytes - 1) / gz->S.chunk_bytes <= inf->gz->max_chunks, SH_ERR_BAD_ARG, "sh_gunzip_feed: %llu bytes are more chunks of %u than the scratch holds",
             (unsigned long long)n, gz->S.chunk_bytes);
    DeviceScope scope(inf->device);
    SH_HIP(scope.err);
    const auto t0 = std::chrono::steady_clock::now();
    DevBackend be{inf, inf->gz, gz, d_in, (uint32_t)n, last != 0, d_out, hs};
    shgz::Feed F;
    const uint64_t file_off = gz->S.file_off;
    const shgz::Outcome rc = shgz::feed(gz->S, be, n, last != 0, std::min<uint64_t>(out_cap, inf->gz->sym_cap), starts, F);
    *consumed = F.consumed; *out_len = F.out_len;
    if (stats) {
        stats->n_chunks = F.c.n_chunks; stats->n_skipped = F.c.n_skipped; stats->n_redone = F.c.n_redone; stats->n_rounds = F.c.n_rounds; stats->n_members = F.c.n_members;
        stats->n_marker_symbols = F.c.n_marker_symbols; stats->n_window_steps = F.c.n_window_steps; stats->in_bytes = F.c.in_bytes; stats->out_bytes = F.c.out_bytes;
        stats->ms_find = be.ms_find; stats->ms_size = be.ms_size; stats->ms_markers = be.ms_markers; stats->ms_windows = be.ms_windows; stats->ms_resolve = be.ms_resolve;
        stats->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (rc == shgz::FEED_OK) return SH_OK;
    gz->dead = true;
    switch (rc) {
    case shgz::FEED_ROUNDS:
        sh_set_error("sh_gunzip: %u rounds left a chunk without a block start behind file offset %llu", shgz::MAX_ROUNDS, (unsigned long long)(file_off + F.consumed));
        return SH_GUNZIP_FALLBACK;
    case shgz::FEED_ENDS:
        sh_set_error("sh_gunzip: more than %u members end in one chunk behind file offset %llu", SHIN_MAX_ENDS, (unsigned long long)(file_off + F.consumed));
        return SH_GUNZIP_FALLBACK;
    case shgz::FEED_DATA:
        sh_set_error("gzip member at file offset %llu does not inflate: status %u (%s)", (unsigned long long)F.err_off, F.status, status_name(F.status));
        return SH_ERR_IO;
    case shgz::FEED_TRUNCATED:
        sh_set_error("gzip stream ends inside a member: truncated at file offset %llu", (unsigned long long)F.err_off);
        return SH_ERR_IO;
    case shgz::FEED_NOT_GZIP:
        sh_set_error("no gzip member at file offset %llu", (unsigned long long)F.err_off);
        return SH_ERR_IO;
    case shgz::FEED_OUT_CAP:
        *consumed = 0; *out_len = 0;
        gz->dead = false;      // nothing was decoded into the caller's memory: a larger output may follow
        sh_set_error("sh_gunzip_feed: room for %llu bytes, the first chunk holds %llu", (unsigned long long)out_cap, (unsigned long long)F.need);
        return SH_ERR_BAD_ARG;
    default:
        return (sh_status)F.backend_rc;
    }
}

}      // namespace

extern "C" sh_status sh_gunzip_open(sh_inflater *inf, uint32_t chunk_bytes, sh_gunzip **out)
{
    SH_CHECK(inf && out, SH_ERR_BAD_ARG, "sh_gunzip_open: null argument");
    *out = nullptr;
    if (chunk_bytes == 0) chunk_bytes = shgz::DEFAULT_CHUNK;
    SH_CHECK(chunk_bytes >= shgz::MIN_CHUNK && chunk_bytes <= shgz::MAX_CHUNK, SH_ERR_BAD_ARG, "sh_gunzip_open: chunks of %u bytes, %u .. %u are taken", chunk_bytes, shgz::MIN_CHUNK,
             shgz::MAX_CHUNK);
    DeviceScope scope(inf->device);
    SH_HIP(scope.err);
    const sh_status rc = gz_scratch_make(inf, (uint32_t)((inf->max_in + chunk_bytes - 1) / chunk_bytes) + 1);
    if (rc != SH_OK) return rc;
    sh_gunzip *gz = new sh_gunzip;
    gz->inf = inf; gz->S.chunk_bytes = chunk_bytes;
    // The window starts as zeros for tidiness only: with win_valid = 0 no byte of it is ever read as data, so the memset (null stream)
    // needs no ordering against the feeds' stream.
    hipError_t e = hipMalloc(&gz->d_win, SHIN_WINDOW);
    const bool have = e == hipSuccess;
    if (have) e = hipMemset(gz->d_win, 0, SHIN_WINDOW);
    if (e != hipSuccess) {
        if (have) hipFree(gz->d_win);
        delete gz;
        sh_set_error("sh_gunzip_open: the window of %u bytes -> %s", SHIN_WINDOW, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SH_ERR_OOM : SH_ERR_HIP;
    }
    *out = gz;
    return SH_OK;
}

// the stream's first byte is byte file_off of its file (a plain member behind BGZF ones): the offsets in errors are the file's
void shi_gunzip_set_offset(sh_gunzip *gz, uint64_t file_off) { if (gz->S.at_header && gz->S.n_members == 0) gz->S.file_off = gz->S.member_off = file_off; }

extern "C" sh_status sh_gunzip_close(sh_gunzip *gz)
{
    if (!gz) return SH_OK;
    DeviceScope scope(gz->inf->device);
    if (gz->d_win) hipFree(gz->d_win);
    delete gz;
    return SH_OK;
}

extern "C" sh_status sh_gunzip_feed_device(sh_gunzip *gz, const uint8_t *d_in, uint64_t n, int32_t last, uint8_t *d_out, uint64_t out_cap, uint64_t *consumed, uint64_t *out_len,
                                           void *stream, sh_gunzip_stats *stats)
{
    SH_CHECK(gz && consumed && out_len && (d_in || n == 0) && (d_out || out_cap == 0), SH_ERR_BAD_ARG, "sh_gunzip_feed_device: null argument");
    return gz_feed(gz, d_in, n, last, d_out, out_cap, nullptr, consumed, out_len, (hipStream_t)stream, stats);
}

extern "C" sh_status sh_gunzip_feed(sh_gunzip *gz, const uint8_t *in, uint64_t n, int32_t last, uint8_t *out, uint64_t out_cap, uint64_t *consumed, uint64_t *out_len,
                                    sh_gunzip_stats *stats)
{
    SH_CHECK(gz && consumed && out_len && (in || n == 0) && (out || out_cap == 0), SH_ERR_BAD_ARG, "sh_gunzip_feed: null argument");
    *consumed = 0; *out_len = 0;
    sh_inflater *inf = gz->inf;
    SH_CHECK(n <= inf->max_in, SH_ERR_BAD_ARG, "sh_gunzip_feed: %llu bytes, the inflater was made for %llu", (unsigned long long)n, (unsigned long long)inf->max_in);
    DeviceScope scope(inf->device);
    SH_HIP(scope.err);
    const sh_status staged = inf_staging(inf, true);
    if (staged != SH_OK) return staged;
    if (n) {
        memcpy(inf->h_in, in, n);
        SH_HIP(hipMemcpyAsync(inf->d_in, inf->h_in, n, hipMemcpyHostToDevice, inf->stream));
    }
    const sh_status rc = gz_feed(gz, inf->d_in, n, last, inf->d_out, std::min(out_cap, inf->max_out), nullptr, consumed, out_len, inf->stream, stats);
    if (*out_len) {      // also behind SH_GUNZIP_FALLBACK: what was decoded before is the caller's
        SH_HIP(hipMemcpyAsync(inf->h_out, inf->d_out, *out_len, hipMemcpyDeviceToHost, inf->stream));
        SH_HIP(hipStreamSynchronize(inf->stream));
        memcpy(out, inf->h_out, *out_len);
    } else hipStreamSynchronize(inf->stream);
    return rc;
}

extern "C" sh_status sh_dbg_gunzip_starts(sh_inflater *inf, uint32_t chunk_bytes, const uint8_t *d_in, uint64_t n, const uint64_t *starts, uint64_t n_starts, uint8_t *d_out,
                                          uint64_t out_cap, uint64_t *out_len, void *stream, sh_gunzip_stats *stats)
{
    SH_CHECK(inf && starts && out_len && (d_in || n == 0) && (d_out || out_cap == 0), SH_ERR_BAD_ARG, "sh_dbg_gunzip_starts: null argument");
    sh_gunzip *gz = nullptr;
    sh_status rc = sh_gunzip_open(inf, chunk_bytes, &gz);
    if (rc != SH_OK) return rc;
    const uint64_t n_chunks = (n + gz->S.chunk_bytes - 1) / gz->S.chunk_bytes;
    uint64_t consumed = 0;
    if (n_starts != n_chunks) { sh_set_error("sh_dbg_gunzip_starts: %llu starts, the stream has %llu chunks", (unsigned long long)n_starts, (unsigned long long)n_chunks); rc = SH_ERR_BAD_ARG; }
    else rc = gz_feed(gz, d_in, n, 1, d_out, out_cap, starts, &consumed, out_len, (hipStream_t)stream, stats);
    if (rc == SH_OK && !gz->S.ended) { sh_set_error("sh_dbg_gunzip_starts: room for %llu bytes, the stream holds more", (unsigned long long)out_cap); rc = SH_ERR_BAD_ARG; }
    sh_gunzip_close(gz);
    return rc;
}

// ---- the per-process pool behind shc::In (sh_codec.h) and the index build, and what a run reports ------------------------------------
namespace shc {

namespace {
std::mutex g_mu;
std::vector<sh_inflater *> g_idle;
std::atomic<int> g_device{0}, g_depth{0};
std::atomic<bool> g_said{false};
std::atomic<uint64_t> g_members{0}, g_bytes{0}, g_zlib_files{0}, g_created{0};
std::atomic<uint64_t> g_any_chunks{0}, g_any_redone{0}, g_any_bytes{0}, g_any_feeds{0};
std::atomic<uint64_t> g_any_us[8];      // microseconds: reading the file, in sh_gunzip_feed, inside it on the device path, find, size, markers, windows, resolve
}

int gunzip_device_level() { const char *e = getenv("SCRUBBY_HIP_GUNZIP_DEVICE"); return e && (e[0] == '1' || e[0] == '2') && e[1] == 0 ? e[0] - '0' : 0; }

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
void gunzip_count_any(uint64_t chunks, uint64_t redone, uint64_t bytes) { g_any_chunks += chunks; g_any_redone += redone; g_any_bytes += bytes; }
void gunzip_time_any(double ms_read, double ms_feed, const sh_gunzip_stats &st)
{
    const double ms[8] = {ms_read, ms_feed, st.ms, st.ms_find, st.ms_size, st.ms_markers, st.ms_windows, st.ms_resolve};
    for (int i = 0; i < 8; ++i) g_any_us[i] += (uint64_t)(ms[i] * 1000.0);
    ++g_any_feeds;
}

GunzipRun::GunzipRun(int device)
{
    if (g_depth.fetch_add(1) == 0) { g_device = device; g_members = 0; g_bytes = 0; g_zlib_files = 0; g_any_chunks = 0; g_any_redone = 0; g_any_bytes = 0; g_any_feeds = 0; for (auto &u : g_any_us) u = 0; }
}

GunzipRun::~GunzipRun()
{
    if (g_depth.fetch_sub(1) != 1 || !gunzip_device_wanted()) return;
    if (const char *e = getenv("SCRUBBY_HIP_DBG_HOST")) if (*e == '1') {
        fprintf(stderr, "[scrubby-hip] gunzip on the device: %llu members, %llu bytes out, %llu files through zlib", (unsigned long long)g_members.load(),
                (unsigned long long)g_bytes.load(), (unsigned long long)g_zlib_files.load());
        if (gunzip_device_level() == 2)      // the second sentence: what went through sh_gunzip
            fprintf(stderr, ". Any gzip stream: %llu chunks, %llu redone, %llu bytes out, %llu files through zlib", (unsigned long long)g_any_chunks.load(),
                    (unsigned long long)g_any_redone.load(), (unsigned long long)g_any_bytes.load(), (unsigned long long)g_zlib_files.load());
        if (gunzip_device_level() == 2) {      // where the readers' time went, summed over the readers
            double ms[8];
            for (int i = 0; i < 8; ++i) ms[i] = (double)g_any_us[i].load() / 1000.0;
            fprintf(stderr, "; %llu feeds, ms reading %.1f, in feeds %.1f (staging copies %.1f, host walk and waits %.1f, find %.1f, size %.1f, markers %.1f, windows %.1f, resolve %.1f)",
                    (unsigned long long)g_any_feeds.load(), ms[0], ms[1], ms[1] - ms[2], ms[2] - ms[3] - ms[4] - ms[5] - ms[6] - ms[7], ms[3], ms[4], ms[5], ms[6], ms[7]);
        }
        fputc('\n', stderr);
    }
}

}      // namespace shc
