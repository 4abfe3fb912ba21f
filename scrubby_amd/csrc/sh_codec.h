// sh_codec.h — byte sources and sinks by container, the set niffler gives the reference: plain, gzip, bzip2, xz.
//
// The reference opens its inputs through needletail / niffler, which sniff the container by its magic bytes
// (/root/reference/src/utils.rs:377-383 parse_fastx_file_with_check; gzip 1f 8b, bzip2 "BZh", xz fd 37 7a 58 5a 00), and picks the
// container of an OUTPUT by the file's extension (CompressionExt::from_path, utils.rs:28-36: .gz -> gzip, .bz / .bz2 -> bzip2,
// .lzma / .xz -> niffler's "Lzma", which is the xz container of the xz2 crate; get_fastx_writer :56-74).
// zlib is linked; bzip2 and xz come from the system's libbz2.so.1.0 / liblzma.so.5, loaded on first use (this image ships the
// libraries without their headers, so the few entry points and the two stream structs are declared here as their ABI has them).
// A host without one of the libraries gets an error that names it when such a file is met - nothing else depends on them.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>
#include "sh_common.h"
#include "sh_inflate.h"

namespace shc {

// ---- SCRUBBY_HIP_GUNZIP_DEVICE=1: BGZF inputs inflated on the device (sh_inflate.hip) ----------------------------------------------------
// A reader takes a window of compressed bytes, scans its member headers, and has a pooled inflater inflate the whole members of the
// window; what the scan does not take goes through zlib from that member's file offset on.
constexpr uint64_t GUNZIP_WINDOW_BYTES = 32ull << 20;      // compressed bytes per window: ~2000 members of FASTQ, one per wave the device holds
constexpr uint64_t GUNZIP_OUT_BYTES = 192ull << 20;        // inflated bytes per call; a window that holds more is inflated in several calls
constexpr uint64_t GUNZIP_MAX_MEMBERS = 1ull << 18;
constexpr uint64_t GUNZIP_READER_MEMBERS = 1ull << 15;     // members a reader takes per fill (1 MiB of descriptors); a window with more is served in several fills
constexpr uint64_t GUNZIP_FIRST_WINDOW_BYTES = 256ull << 10;      // the first window of a file is small: file_is_empty opens every input for one byte
int gunzip_device_level();                        // the switch, read at every call: 1 = BGZF members on the device, 2 = any gzip stream as well, else 0
inline bool gunzip_device_wanted() { return gunzip_device_level() >= 1; }
// A reader of a general gzip stream (level 2) feeds windows of 16 MiB and takes a whole inflater call's output per feed: one feed drains
// a window up to a ratio of 12, so the window is not found and sized again for the part a smaller output would have cut off.
constexpr uint64_t GUNZIP_ANY_WINDOW_BYTES = 16ull << 20;
constexpr uint64_t GUNZIP_ANY_OUT_BYTES = GUNZIP_OUT_BYTES;
void gunzip_count_any(uint64_t chunks, uint64_t redone, uint64_t bytes);
void gunzip_time_any(double ms_read, double ms_feed, const sh_gunzip_stats &st);
int gunzip_reader_device();                       // the open run's device, else the calling thread's current one
sh_inflater *gunzip_pool_acquire(int device);     // an idle inflater of that device, else a new one on it; nullptr: no device or no memory
void gunzip_pool_release(sh_inflater *inf);
void gunzip_note_zlib(const char *path, uint64_t file_off, const char *why);      // a file handed to zlib: counted, announced once per process
void gunzip_count(uint64_t members, uint64_t bytes);
struct GunzipRun {      // around a run: zeroes the counts, and at the end prints the SCRUBBY_HIP_DBG_HOST=1 line when the switch is on
    explicit GunzipRun(int device);
    ~GunzipRun();
    GunzipRun(const GunzipRun &) = delete;
};

// the members of win[0, n) in calls that fit the inflater, appended to `out` (host) or written to d_out (device, contiguous); file_off of
// the members is what an error names
inline sh_status gunzip_window(sh_inflater *inf, const uint8_t *win, sh_gz_member *m, uint64_t n_members, std::vector<uint8_t> *out, uint8_t *d_out)
{
    for (uint64_t i = 0; i < n_members;) {
        uint64_t j = i, bytes = 0;
        while (j < n_members && j - i < GUNZIP_MAX_MEMBERS && bytes + m[j].out_len <= GUNZIP_OUT_BYTES) bytes += m[j++].out_len;
        // the call's input is the stretch of the window its members lie in
        const uint64_t base = m[i].in_off, end = m[j - 1].in_off + m[j - 1].in_len;
        for (uint64_t k = i; k < j; ++k) m[k].in_off -= base;
        size_t at = 0;
        if (out) { at = out->size(); out->resize(at + bytes); }
        uint64_t got = 0;
        const sh_status rc = shi_gunzip_members(inf, win + base, end - base, m + i, j - i, out ? out->data() + at : nullptr, d_out, bytes, &got, nullptr);
        for (uint64_t k = i; k < j; ++k) m[k].in_off += base;
        if (rc != SH_OK) return rc;
        if (d_out) d_out += bytes;
        gunzip_count(j - i, bytes);
        i = j;
    }
    return SH_OK;
}

// ---- libbz2 ---------------------------------------------------------------------------------------------------------------------
struct bz_stream_t {
    char *next_in; unsigned int avail_in, total_in_lo32, total_in_hi32;
    char *next_out; unsigned int avail_out, total_out_lo32, total_out_hi32;
    void *state; void *(*bzalloc)(void *, int, int); void (*bzfree)(void *, void *); void *opaque;
};
enum { BZ_RUN_ = 0, BZ_FINISH_ = 2, BZ_OK_ = 0, BZ_RUN_OK_ = 1, BZ_FINISH_OK_ = 3, BZ_STREAM_END_ = 4 };
struct Bz2Api {
    int (*DecompressInit)(bz_stream_t *, int, int) = nullptr; int (*Decompress)(bz_stream_t *) = nullptr; int (*DecompressEnd)(bz_stream_t *) = nullptr;
    int (*CompressInit)(bz_stream_t *, int, int, int) = nullptr; int (*Compress)(bz_stream_t *, int) = nullptr; int (*CompressEnd)(bz_stream_t *) = nullptr;
    bool ok = false;
    static const Bz2Api &get()
    {
        static Bz2Api a = [] {
            Bz2Api x;
            void *h = dlopen("libbz2.so.1.0", RTLD_NOW | RTLD_LOCAL);
            if (!h) h = dlopen("libbz2.so.1", RTLD_NOW | RTLD_LOCAL);
            if (!h) return x;
            x.DecompressInit = (int (*)(bz_stream_t *, int, int))dlsym(h, "BZ2_bzDecompressInit");
            x.Decompress = (int (*)(bz_stream_t *))dlsym(h, "BZ2_bzDecompress");
            x.DecompressEnd = (int (*)(bz_stream_t *))dlsym(h, "BZ2_bzDecompressEnd");
            x.CompressInit = (int (*)(bz_stream_t *, int, int, int))dlsym(h, "BZ2_bzCompressInit");
            x.Compress = (int (*)(bz_stream_t *, int))dlsym(h, "BZ2_bzCompress");
            x.CompressEnd = (int (*)(bz_stream_t *))dlsym(h, "BZ2_bzCompressEnd");
            x.ok = x.DecompressInit && x.Decompress && x.DecompressEnd && x.CompressInit && x.Compress && x.CompressEnd;
            return x;
        }();
        return a;
    }
};

// ---- liblzma --------------------------------------------------------------------------------------------------------------------
struct lzma_stream_t {
    const uint8_t *next_in; size_t avail_in; uint64_t total_in;
    uint8_t *next_out; size_t avail_out; uint64_t total_out;
    const void *allocator; void *internal;
    void *reserved_ptr1, *reserved_ptr2, *reserved_ptr3, *reserved_ptr4;
    uint64_t reserved_int1, reserved_int2; size_t reserved_int3, reserved_int4;
    int reserved_enum1, reserved_enum2;
};
enum { LZMA_RUN_ = 0, LZMA_FINISH_ = 3, LZMA_OK_ = 0, LZMA_STREAM_END_ = 1, LZMA_CHECK_CRC64_ = 4, LZMA_CONCATENATED_ = 0x08 };
struct LzmaApi {
    int (*stream_decoder)(lzma_stream_t *, uint64_t, uint32_t) = nullptr; int (*easy_encoder)(lzma_stream_t *, uint32_t, int) = nullptr;
    int (*code)(lzma_stream_t *, int) = nullptr; void (*end)(lzma_stream_t *) = nullptr;
    bool ok = false;
    static const LzmaApi &get()
    {
        static LzmaApi a = [] {
            LzmaApi x;
            void *h = dlopen("liblzma.so.5", RTLD_NOW | RTLD_LOCAL);
            if (!h) return x;
            x.stream_decoder = (int (*)(lzma_stream_t *, uint64_t, uint32_t))dlsym(h, "lzma_stream_decoder");
            x.easy_encoder = (int (*)(lzma_stream_t *, uint32_t, int))dlsym(h, "lzma_easy_encoder");
            x.code = (int (*)(lzma_stream_t *, int))dlsym(h, "lzma_code");
            x.end = (void (*)(lzma_stream_t *))dlsym(h, "lzma_end");
            x.ok = x.stream_decoder && x.easy_encoder && x.code && x.end;
            return x;
        }();
        return a;
    }
};

enum class Kind { Plain, Gzip, Bzip2, Xz };

inline Kind kind_by_extension(const std::string &p)
{   // CompressionExt::from_path (utils.rs:28-36): the LAST extension decides
    auto ends = [&](const char *s) { const size_t k = strlen(s); return p.size() >= k && p.compare(p.size() - k, k, s) == 0; };
    if (ends(".gz")) return Kind::Gzip;
    if (ends(".bz") || ends(".bz2")) return Kind::Bzip2;
    if (ends(".lzma") || ends(".xz")) return Kind::Xz;
    return Kind::Plain;
}

// ---- a sequential, decompressing reader (what gzread is for plain and gzip files) -----------------------------------------------------
class In {
    Kind kind_ = Kind::Plain;
    gzFile gz_ = nullptr;
    FILE *fp_ = nullptr;
    bz_stream_t bz_{}; lzma_stream_t xz_{};
    bool codec_open_ = false, src_eof_ = false, end_ = false;
    std::vector<uint8_t> in_;
    // SCRUBBY_HIP_GUNZIP_DEVICE=1 and a file whose first member is BGZF: fp_ is the file, in_[0, win_n_) the window of compressed bytes
    // that begins at file offset foff_, inflated_[served_, ...) what the last window gave and has not been served yet
    bool bgzf_ = false, first_window_ = true;
    std::string path_;
    uint64_t foff_ = 0;
    size_t win_n_ = 0, served_ = 0;
    std::vector<uint8_t> inflated_;
    size_t inflated_n_ = 0;      // inflated_[served_, inflated_n_) is what is left to serve
    std::vector<sh_gz_member> members_;
    // SCRUBBY_HIP_GUNZIP_DEVICE=2 and a gzip member that is not BGZF (the file's first, or one behind BGZF members): the same window of
    // the file is fed to a sh_gunzip on a pooled inflater, which the reader keeps until the file is closed.  served_total_ counts what
    // the reader has handed out, for the fallback: zlib then reads the file again from its start and passes over that many bytes.
    bool any_ = false;
    sh_inflater *any_inf_ = nullptr;
    sh_gunzip *any_gz_ = nullptr;
    uint64_t served_total_ = 0;
    size_t any_window_ = (size_t)GUNZIP_ANY_WINDOW_BYTES;

    // what gzread does for the plain and gzip files: -1 = error
    long read_gz(void *buf, size_t n)
    {
        size_t done = 0;
        while (done < n) {
            const unsigned want = (unsigned)std::min<size_t>(n - done, 1u << 30);
            const int got = gzread(gz_, (char *)buf + done, want);
            if (got < 0) { int e; error = std::string("read error: ") + gzerror(gz_, &e); return -1; }
            done += (size_t)got;
            if ((unsigned)got < want) {
                int e = Z_OK;
                const char *msg = gzerror(gz_, &e);      // a truncated .gz ends with Z_BUF_ERROR, not with a clean end of stream
                if (e != Z_OK && e != Z_STREAM_END) { error = std::string("read error: ") + (msg && *msg ? msg : "truncated gzip stream"); return -1; }
                break;
            }
        }
        return (long)done;
    }
    // the rest of the file, from the member at foff_ on, goes through zlib.  1 = gz_ reads on, 0 = what follows is no gzip member (zlib
    // ignores such a tail behind a member), -1 = error
    int bgzf_to_zlib(const char *why)
    {
        const bool gzip_here = win_n_ >= 2 && in_[0] == 0x1f && in_[1] == 0x8b;
        bgzf_ = false;
        fclose(fp_); fp_ = nullptr;
        if (!gzip_here) { end_ = true; return 0; }
        gunzip_note_zlib(path_.c_str(), foff_, why);
        const int fd = ::open(path_.c_str(), O_RDONLY);
        if (fd < 0 || lseek(fd, (off_t)foff_, SEEK_SET) < 0 || !(gz_ = gzdopen(fd, "rb"))) { if (fd >= 0) ::close(fd); error = "cannot open " + path_; return -1; }
        gzbuffer(gz_, 1 << 20);
        return 1;
    }
    void any_release()
    {
        if (any_gz_) { sh_gunzip_close(any_gz_); any_gz_ = nullptr; }
        if (any_inf_) { gunzip_pool_release(any_inf_); any_inf_ = nullptr; }
    }
    // the whole file goes through zlib, which passes over what was served.  2 = gz_ reads on, -1 = error
    int any_to_zlib(const char *why)
    {
        any_release();
        any_ = false;
        if (fp_) { fclose(fp_); fp_ = nullptr; }
        gunzip_note_zlib(path_.c_str(), foff_, why);
        gz_ = gzopen(path_.c_str(), "rb");
        if (!gz_) { error = "cannot open " + path_; return -1; }
        gzbuffer(gz_, 1 << 20);
        std::vector<char> skip(1 << 20);
        for (uint64_t left = served_total_; left;) {
            const int got = gzread(gz_, skip.data(), (unsigned)std::min<uint64_t>(left, skip.size()));
            if (got <= 0) { error = "read error: " + path_ + " does not hold again what was read from it"; return -1; }
            left -= (uint64_t)got;
        }
        return 2;
    }
    // the next window of a general gzip stream: as bgzf_fill
    int any_fill()
    {
        if (!any_gz_) {
            any_inf_ = gunzip_pool_acquire(gunzip_reader_device());
            if (!any_inf_ || sh_gunzip_open(any_inf_, 0, &any_gz_) != SH_OK) return any_to_zlib("no device inflater");
            shi_gunzip_set_offset(any_gz_, foff_);
        }
        if (inflated_.size() < GUNZIP_ANY_OUT_BYTES) inflated_.resize((size_t)GUNZIP_ANY_OUT_BYTES);
        for (;;) {
            const size_t want = first_window_ ? (size_t)GUNZIP_FIRST_WINDOW_BYTES : any_window_;
            if (in_.size() < want) in_.resize(want);
            const auto t0 = std::chrono::steady_clock::now();
            while (win_n_ < want && !src_eof_) {
                const size_t got = fread(in_.data() + win_n_, 1, want - win_n_, fp_);
                if (got == 0) { if (ferror(fp_)) { error = "read error"; return -1; } src_eof_ = true; }
                win_n_ += got;
            }
            uint64_t consumed = 0, out_len = 0;
            sh_gunzip_stats st;
            const auto t1 = std::chrono::steady_clock::now();
            const sh_status rc = sh_gunzip_feed(any_gz_, in_.data(), win_n_, src_eof_ ? 1 : 0, inflated_.data(), GUNZIP_ANY_OUT_BYTES, &consumed, &out_len, &st);
            if (rc == SH_GUNZIP_FALLBACK) return any_to_zlib("a gzip stream the device finds no block starts in");
            if (rc == SH_ERR_BAD_ARG) return any_to_zlib("a chunk that holds more than a reader takes");
            if (rc != SH_OK) { error = std::string("read error: ") + sh_last_error(); return -1; }
            gunzip_count_any(st.n_chunks, st.n_redone, out_len);
            gunzip_time_any(std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(), st);
            memmove(in_.data(), in_.data() + consumed, win_n_ - consumed);
            win_n_ -= consumed; foff_ += consumed;
            served_ = 0; inflated_n_ = out_len;
            if (out_len) { first_window_ = false; return 1; }
            if (src_eof_) { end_ = true; return 0; }      // a last feed that gives nothing and no error: the stream is over
            if (consumed) continue;
            if (first_window_) { first_window_ = false; continue; }      // a block larger than the first window
            if (any_window_ < (size_t)GUNZIP_WINDOW_BYTES) { any_window_ = (size_t)GUNZIP_WINDOW_BYTES; continue; }      // or than 16 MiB: all an inflater takes
            return any_to_zlib("a block larger than the window");
        }
    }
    // the next window: 1 = inflated_ holds bytes, 2 = handed to zlib, 3 = what follows is for any_fill, 0 = end of the file, -1 = error
    int bgzf_fill()
    {
        for (;;) {
            const size_t want = first_window_ ? (size_t)GUNZIP_FIRST_WINDOW_BYTES : (size_t)GUNZIP_WINDOW_BYTES;
            if (in_.size() < want) in_.resize(want);
            while (win_n_ < want && !src_eof_) {
                const size_t got = fread(in_.data() + win_n_, 1, want - win_n_, fp_);
                if (got == 0) { if (ferror(fp_)) { error = "read error"; return -1; } src_eof_ = true; }
                win_n_ += got;
            }
            if (win_n_ == 0) { end_ = true; return 0; }
            if (members_.empty()) members_.resize(GUNZIP_READER_MEMBERS);
            uint64_t n_members = 0, consumed = 0;
            const int stopped = shin_bgzf_scan(in_.data(), win_n_, (ShinMember *)members_.data(), members_.size(), &n_members, &consumed);
            // one inflate call's worth of output at a time: the members past GUNZIP_OUT_BYTES of ISIZE stay in the window for the next fill,
            // so inflated_ never holds more than that, however well the file compresses
            for (uint64_t i = 0, bytes = 0; i < n_members; ++i) {
                bytes += members_[i].out_len;
                if (bytes > GUNZIP_OUT_BYTES) { n_members = i; consumed = members_[i].file_off; break; }
            }
            if (n_members == 0) {
                if (stopped == 1 && src_eof_) { error = "read error: truncated BGZF member at file offset " + std::to_string(foff_); return -1; }
                if (stopped == 1) { first_window_ = false; continue; }      // a member larger than the first window
                if (gunzip_device_level() == 2 && win_n_ >= 2 && in_[0] == 0x1f && in_[1] == 0x8b) { bgzf_ = false; any_ = true; served_ = inflated_n_ = 0; return 3; }
                const int r = bgzf_to_zlib("a gzip member that is not BGZF");
                return r > 0 ? 2 : r;
            }
            sh_inflater *inf = gunzip_pool_acquire(gunzip_reader_device());
            if (!inf) { const int r = bgzf_to_zlib("no device inflater"); return r > 0 ? 2 : r; }
            for (uint64_t i = 0; i < n_members; ++i) members_[i].file_off += foff_;
            inflated_.clear();
            served_ = 0;
            const sh_status rc = gunzip_window(inf, in_.data(), members_.data(), n_members, &inflated_, nullptr);
            gunzip_pool_release(inf);
            if (rc != SH_OK) { error = std::string("read error: ") + sh_last_error(); return -1; }
            memmove(in_.data(), in_.data() + consumed, win_n_ - consumed);
            win_n_ -= consumed; foff_ += consumed;
            first_window_ = false;
            inflated_n_ = inflated_.size();
            if (!inflated_.empty()) return 1;
        }
    }
public:
    std::string error;
    In() = default;
    In(const In &) = delete;
    ~In() { close(); }
    bool open(const char *path)
    {
        close();
        error.clear();
        FILE *f = fopen(path, "rb");
        if (!f) { error = std::string("cannot open ") + path; return false; }
        unsigned char m[6] = {0, 0, 0, 0, 0, 0};
        const size_t n = fread(m, 1, 6, f);
        if (n >= 3 && m[0] == 'B' && m[1] == 'Z' && m[2] == 'h') kind_ = Kind::Bzip2;
        else if (n >= 6 && m[0] == 0xFD && m[1] == '7' && m[2] == 'z' && m[3] == 'X' && m[4] == 'Z' && m[5] == 0x00) kind_ = Kind::Xz;
        else kind_ = Kind::Plain;      // (gzip and plain alike: gzread passes plain bytes through)
        if (kind_ == Kind::Plain && n >= 2 && m[0] == 0x1f && m[1] == 0x8b && gunzip_device_wanted()) {
            rewind(f);
            in_.resize((size_t)GUNZIP_FIRST_WINDOW_BYTES);
            win_n_ = fread(in_.data(), 1, in_.size(), f);
            sh_gz_member first;
            uint64_t n_members = 0, consumed = 0;
            const int stopped = shin_bgzf_scan(in_.data(), win_n_, (ShinMember *)&first, 1, &n_members, &consumed);
            if (n_members == 1 || stopped == 1) {      // the first member is BGZF (or the beginning of one): the inflater is taken at the first read
                fp_ = f; path_ = path; bgzf_ = true; first_window_ = true; foff_ = 0; served_ = 0; inflated_n_ = 0; served_total_ = 0;
                inflated_.clear();
                return true;
            }
            if (gunzip_device_level() == 2) {      // an ordinary gzip file: the sh_gunzip is taken at the first read
                fp_ = f; path_ = path; any_ = true; first_window_ = true; foff_ = 0; served_ = 0; inflated_n_ = 0; served_total_ = 0;
                return true;
            }
            win_n_ = 0;
        }
        if (kind_ == Kind::Plain) {
            fclose(f);
            gz_ = gzopen(path, "rb");
            if (!gz_) { error = std::string("cannot open ") + path; return false; }
            gzbuffer(gz_, 1 << 20);
            return true;
        }
        rewind(f);
        fp_ = f;
        in_.resize(1 << 20);
        if (kind_ == Kind::Bzip2) {
            const Bz2Api &A = Bz2Api::get();
            if (!A.ok) { error = std::string("bzip2-compressed input, but libbz2.so.1.0 could not be loaded: ") + path; close(); return false; }
            memset(&bz_, 0, sizeof(bz_));
            if (A.DecompressInit(&bz_, 0, 0) != BZ_OK_) { error = "BZ2_bzDecompressInit failed"; close(); return false; }
        } else {
            const LzmaApi &A = LzmaApi::get();
            if (!A.ok) { error = std::string("xz-compressed input, but liblzma.so.5 could not be loaded: ") + path; close(); return false; }
            memset(&xz_, 0, sizeof(xz_));
            if (A.stream_decoder(&xz_, UINT64_MAX, LZMA_CONCATENATED_) != LZMA_OK_) { error = "lzma_stream_decoder failed"; close(); return false; }
        }
        codec_open_ = true;
        return true;
    }
    bool is_open() const { return gz_ != nullptr || fp_ != nullptr; }
    // up to n bytes; 0 = end of the stream; -1 = error (message in `error`: a truncated or corrupt stream is an error, never a short input)
    long read(void *buf, size_t n)
    {
        if (n == 0) return 0;
        if (bgzf_ || any_) {
            size_t done = 0;
            while (done < n) {
                if (served_ == inflated_n_) {
                    if (end_) break;
                    const int r = bgzf_ ? bgzf_fill() : any_fill();
                    if (r < 0) return -1;
                    if (r == 0) break;
                    if (r == 2) { const long g = read_gz((char *)buf + done, n - done); return g < 0 ? -1 : (long)done + g; }
                    if (r == 3) continue;
                }
                const size_t k = std::min(n - done, inflated_n_ - served_);
                memcpy((char *)buf + done, inflated_.data() + served_, k);
                done += k; served_ += k; served_total_ += k;
            }
            return (long)done;
        }
        if (gz_) return read_gz(buf, n);
        if (!fp_ || end_) return 0;
        size_t done = 0;
        while (done < n && !end_) {
            const bool bz = kind_ == Kind::Bzip2;
            const size_t avail_in = bz ? bz_.avail_in : xz_.avail_in;
            if (avail_in == 0 && !src_eof_) {
                const size_t got = fread(in_.data(), 1, in_.size(), fp_);
                if (got < in_.size()) { if (ferror(fp_)) { error = "read error"; return -1; } src_eof_ = true; }
                if (bz) { bz_.next_in = (char *)in_.data(); bz_.avail_in = (unsigned)got; } else { xz_.next_in = in_.data(); xz_.avail_in = got; }
            }
            if (bz) {
                const Bz2Api &A = Bz2Api::get();
                bz_.next_out = (char *)buf + done; bz_.avail_out = (unsigned)std::min<size_t>(n - done, 1u << 30);
                const unsigned before = bz_.avail_out;
                const int rc = A.Decompress(&bz_);
                done += before - bz_.avail_out;
                if (rc == BZ_STREAM_END_) {
                    // concatenated streams (bzip2 -c a b, pbzip2): go on with the next one if input is left
                    if (bz_.avail_in == 0 && src_eof_) { end_ = true; break; }
                    if (bz_.avail_in == 0) { const size_t got = fread(in_.data(), 1, in_.size(), fp_); if (got < in_.size()) src_eof_ = true; bz_.next_in = (char *)in_.data(); bz_.avail_in = (unsigned)got; if (got == 0) { end_ = true; break; } }
                    std::vector<uint8_t> rest(bz_.next_in, bz_.next_in + bz_.avail_in);
                    A.DecompressEnd(&bz_);
                    memset(&bz_, 0, sizeof(bz_));
                    if (A.DecompressInit(&bz_, 0, 0) != BZ_OK_) { error = "BZ2_bzDecompressInit failed"; return -1; }
                    memcpy(in_.data(), rest.data(), rest.size());
                    bz_.next_in = (char *)in_.data(); bz_.avail_in = (unsigned)rest.size();
                } else if (rc != BZ_OK_) { error = "read error: corrupt bzip2 stream"; return -1; }
                else if (before == bz_.avail_out && bz_.avail_in == 0 && src_eof_) { error = "read error: truncated bzip2 stream"; return -1; }
            } else {
                const LzmaApi &A = LzmaApi::get();
                xz_.next_out = (uint8_t *)buf + done; xz_.avail_out = n - done;
                const size_t before = xz_.avail_out;
                const int rc = A.code(&xz_, src_eof_ && xz_.avail_in == 0 ? LZMA_FINISH_ : LZMA_RUN_);
                done += before - xz_.avail_out;
                if (rc == LZMA_STREAM_END_) { end_ = true; break; }
                if (rc != LZMA_OK_) { error = rc == 10 /* LZMA_BUF_ERROR */ ? "read error: truncated xz stream" : "read error: corrupt xz stream"; return -1; }
            }
        }
        return (long)done;
    }
    void close()
    {
        if (gz_) { gzclose(gz_); gz_ = nullptr; }
        if (codec_open_) { if (kind_ == Kind::Bzip2) Bz2Api::get().DecompressEnd(&bz_); else if (kind_ == Kind::Xz) LzmaApi::get().end(&xz_); codec_open_ = false; }
        if (fp_) { fclose(fp_); fp_ = nullptr; }
        src_eof_ = end_ = false;
        any_release();
        bgzf_ = any_ = false; win_n_ = 0; served_ = 0; inflated_n_ = 0; foff_ = 0; served_total_ = 0;
        inflated_.clear();
    }
};

// ---- a sequential, compressing writer; the container by the path's extension, like the reference's get_fastx_writer ---------------------------
class Out {
    Kind kind_ = Kind::Plain;
    gzFile gz_ = nullptr;
    FILE *fp_ = nullptr;
    bz_stream_t bz_{}; lzma_stream_t xz_{};
    bool codec_open_ = false;
    std::vector<uint8_t> out_;
    bool pump(int action)      // run the encoder until it has taken all input (and, on finish, until the stream has ended)
    {
        for (;;) {
            int rc; size_t produced;
            if (kind_ == Kind::Bzip2) {
                bz_.next_out = (char *)out_.data(); bz_.avail_out = (unsigned)out_.size();
                rc = Bz2Api::get().Compress(&bz_, action ? BZ_FINISH_ : BZ_RUN_);
                produced = out_.size() - bz_.avail_out;
                if (rc < 0) { error = "bzip2 compression failed"; return false; }
                if (produced && fwrite(out_.data(), 1, produced, fp_) != produced) { error = "write error"; return false; }
                if (action ? rc == BZ_STREAM_END_ : bz_.avail_in == 0) return true;
            } else {
                xz_.next_out = out_.data(); xz_.avail_out = out_.size();
                rc = LzmaApi::get().code(&xz_, action ? LZMA_FINISH_ : LZMA_RUN_);
                produced = out_.size() - xz_.avail_out;
                if (rc != LZMA_OK_ && rc != LZMA_STREAM_END_) { error = "xz compression failed"; return false; }
                if (produced && fwrite(out_.data(), 1, produced, fp_) != produced) { error = "write error"; return false; }
                if (action ? rc == LZMA_STREAM_END_ : xz_.avail_in == 0) return true;
            }
        }
    }
public:
    std::string error;
    Out() = default;
    Out(const Out &) = delete;
    ~Out() { close(); }
    // level: niffler's compression level (the reference writes with Level::Six; the id table with Nine)
    bool open(const std::string &path, int level = 6)
    {
        kind_ = kind_by_extension(path);
        error.clear();
        if (kind_ == Kind::Gzip) {
            const std::string mode = "wb" + std::to_string(level);
            gz_ = gzopen(path.c_str(), mode.c_str());
            if (!gz_) error = "cannot open " + path;
            return gz_ != nullptr;
        }
        fp_ = fopen(path.c_str(), "wb");
        if (!fp_) { error = "cannot open " + path; return false; }
        if (kind_ == Kind::Plain) return true;
        out_.resize(1 << 20);
        if (kind_ == Kind::Bzip2) {
            const Bz2Api &A = Bz2Api::get();
            if (!A.ok) { error = "bzip2 output asked for, but libbz2.so.1.0 could not be loaded: " + path; return false; }
            memset(&bz_, 0, sizeof(bz_));
            if (A.CompressInit(&bz_, level < 1 ? 1 : (level > 9 ? 9 : level), 0, 0) != BZ_OK_) { error = "BZ2_bzCompressInit failed"; return false; }
        } else {
            const LzmaApi &A = LzmaApi::get();
            if (!A.ok) { error = "xz output asked for, but liblzma.so.5 could not be loaded: " + path; return false; }
            memset(&xz_, 0, sizeof(xz_));
            if (A.easy_encoder(&xz_, (uint32_t)(level < 0 ? 0 : (level > 9 ? 9 : level)), LZMA_CHECK_CRC64_) != LZMA_OK_) { error = "lzma_easy_encoder failed"; return false; }
        }
        codec_open_ = true;
        return true;
    }
    bool ok() const { return error.empty() && (gz_ || fp_); }
    bool write(const void *data, size_t n)
    {
        if (!error.empty()) return false;
        if (n == 0) return true;
        if (gz_) {
            for (size_t o = 0; o < n;) { const unsigned w = (unsigned)std::min<size_t>(n - o, 1u << 30); if (gzwrite(gz_, (const char *)data + o, w) != (int)w) { error = "write error"; return false; } o += w; }
            return true;
        }
        if (kind_ == Kind::Plain) { if (fwrite(data, 1, n, fp_) != n) { error = "write error"; return false; } return true; }
        for (size_t o = 0; o < n;) {
            const size_t w = std::min<size_t>(n - o, 1u << 30);
            if (kind_ == Kind::Bzip2) { bz_.next_in = (char *)data + o; bz_.avail_in = (unsigned)w; } else { xz_.next_in = (const uint8_t *)data + o; xz_.avail_in = w; }
            if (!pump(0)) return false;
            o += w;
        }
        return true;
    }
    bool close()
    {
        bool good = error.empty();
        if (gz_) { if (gzclose(gz_) != Z_OK) { error = "write error"; good = false; } gz_ = nullptr; }
        if (codec_open_) {
            if (good) { if (kind_ == Kind::Bzip2) { bz_.next_in = nullptr; bz_.avail_in = 0; } else { xz_.next_in = nullptr; xz_.avail_in = 0; } good = pump(1); }
            if (kind_ == Kind::Bzip2) Bz2Api::get().CompressEnd(&bz_); else LzmaApi::get().end(&xz_);
            codec_open_ = false;
        }
        if (fp_) { if (fclose(fp_) != 0) { error = "write error"; good = false; } fp_ = nullptr; }
        return good;
    }
};

}  // namespace shc
