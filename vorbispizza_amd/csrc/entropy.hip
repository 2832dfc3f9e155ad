// Entropy decode of Vorbis audio packets on the GPU (include/vorbispizza_entropy.h): Floor1.Unpack, the coupling fix-up
// of the no-residue flags and Residue0/1/2.Decode (Mapping.cs:109-163) for a planned batch of packets, bit for bit what
// the CPU front end's decode_packet writes (vorbispizza_amd/host/vorbis_front.cpp; every function below names the one
// it restates).  Built with -ffp-contract=off: the residue sums are plain float adds in the host's order.
//
// Work mapping: one lane per packet.  A packet's bit chain is serial -- every code's length decides
// where the next one starts -- and the parallelism is across packets, hundreds of thousands of them in a library.  The
// setup's tables (prefix tables, overflow lists, value lookups) live in global memory and are read through the caches:
// every stream of a setup shares them.  The residue regions are zeroed first by a coalesced pass (a workgroup per
// packet), so that the lane only adds into them.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "../../include/vorbispizza_entropy.h"

namespace vpz {
namespace {

// what the kernels know of a packet (24 bytes): where its bits are, where its residue goes, its flags and mapping
struct PacketDesc {
    int64_t payload_bit;     // bit offset of the packet in the payload
    int64_t residue_offset;  // value offset of its residue
    uint32_t size;           // bytes
    uint32_t info;           // flags | mapping << 8
};

constexpr int kBlock = 256;
constexpr int64_t kSmallLaunch = 65536;  // packets below which entropy_decode_kernel is launched with one wave per workgroup

// 256 one-bit flags in registers (a runtime-indexed array would live in scratch memory): channels of a packet
struct Mask256 {
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    __host__ __device__ bool get(int i) const
    {
        const uint64_t w = i < 64 ? m0 : i < 128 ? m1 : i < 192 ? m2 : m3;
        return (w >> (i & 63)) & 1u;
    }
    __host__ __device__ void put(int i, bool v)
    {
        const uint64_t bit = 1ull << (i & 63);
        if (i < 64) m0 = v ? (m0 | bit) : (m0 & ~bit);
        else if (i < 128) m1 = v ? (m1 | bit) : (m1 & ~bit);
        else if (i < 192) m2 = v ? (m2 | bit) : (m2 & ~bit);
        else m3 = v ? (m3 | bit) : (m3 & ~bit);
    }
};

// BitReader (host: try_peek / skip / read_bits): LSB first; a peek near the end returns the bits that are left,
// zero-padded; a skip past the end stops at the end.  Two aligned words of the payload per peek.
struct Bits {
    const uint32_t *words;
    uint64_t base;  // bit offset of the packet in the payload
    uint32_t pos, total;

    __host__ __device__ uint32_t peek(int count, int &n) const
    {
        const uint32_t rem = total - pos;
        n = rem < (uint32_t)count ? (int)rem : count;
        if (n <= 0) {
            n = 0;
            return 0;
        }
        const uint64_t ab = base + pos;
        const uint64_t q = ab >> 5;
        const uint64_t w = (uint64_t)words[q] | ((uint64_t)words[q + 1] << 32);
        const uint32_t v = (uint32_t)(w >> (ab & 31));
        return n >= 32 ? v : (v & ((1u << n) - 1u));
    }
    __host__ __device__ void skip(uint32_t count)
    {
        const uint32_t rem = total - pos;
        pos = rem >= count ? pos + count : total;
    }
    __host__ __device__ uint32_t read(int count)
    {
        int n;
        const uint32_t v = peek(count, n);
        pos += (uint32_t)n;
        return v;
    }
};

template <class T> __host__ __device__ const T *at(const uint8_t *img, uint32_t off) { return reinterpret_cast<const T *>(img + off); }

// Codebook::decode_scalar: the prefix table, then the overflow list in the host's order; -1 on a miss
__host__ __device__ int decode_scalar(const uint8_t *img, const vpz_entropy_book *b, Bits &p)
{
    int n;
    const int prefix_count = b->prefix_count;
    const uint32_t data = p.peek(b->prefix_bits, n);
    if (n != 0 && prefix_count != 0) {
        const uint32_t e = at<uint32_t>(img, b->prefix)[data];
        if (e & 63u) {
            p.skip(e & 63u);
            return (int)(e >> 6);
        }
    }
    const uint32_t d = p.peek(b->max_bits, n);
    if (n != 0) {
        const vpz_entropy_code *c = at<vpz_entropy_code>(img, b->overflow);
        const int count = b->overflow_count;
        for (int k = 0; k < count; ++k) {
            if (c[k].bits == (d & c[k].mask)) {
                p.skip(c[k].length);
                return (int)c[k].value;
            }
        }
    }
    return -1;
}

__host__ __device__ inline int16_t clamp16(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// Floor1::unpack -> the post count; posts are written to `out` as they are read (the record was zeroed), so that a
// miss leaves what was read before it, as the host's `raw` array does
__host__ __device__ int floor1_unpack(const uint8_t *img, const vpz_entropy_book *books, const vpz_entropy_floor1 *f, Bits &p,
                             int16_t *out)
{
    if (!p.read(1)) return 0;
    const int y_bits = f->y_bits;
    int post_count = 2;
    out[0] = clamp16((int)p.read(y_bits));
    out[1] = clamp16((int)p.read(y_bits));
    const int parts = f->partition_count;
    for (int i = 0; i < parts; ++i) {
        const int cls = f->partition_class[i];
        const int cdim = f->class_dimensions[cls];
        const int cbits = f->class_subclasses[cls];
        const uint32_t csub = (1u << cbits) - 1u;
        uint32_t cval = 0;
        if (cbits > 0) {
            const int v = decode_scalar(img, books + f->class_masterbooks[cls], p);
            if (v == -1) return 0;
            cval = (uint32_t)v;
        }
        for (int j = 0; j < cdim; ++j) {
            const int book_idx = f->subclass_books[cls * 8 + (cval & csub)];
            cval >>= cbits;
            int post = 0;
            if (book_idx >= 0) {
                post = decode_scalar(img, books + book_idx, p);
                if (post == -1) return 0;
            }
            if (post_count < 64) out[post_count] = clamp16(post);
            ++post_count;
        }
    }
    return post_count;
}

template <class T> __host__ __device__ const T *values(const uint8_t *img, const vpz_entropy_book *b);
template <> __host__ __device__ const float *values<float>(const uint8_t *img, const vpz_entropy_book *b) { return at<float>(img, b->lookup_f32); }
template <> __host__ __device__ const int16_t *values<int16_t>(const uint8_t *img, const vpz_entropy_book *b) { return at<int16_t>(img, b->lookup_i16); }

// Residue::write_vectors: type 0 sums an entry into ONE bin, every partial sum rounded (quirk q9); types 1 / 2 add the
// vector to consecutive bins.  true: the packet ran out
template <class T>
__host__ __device__ bool write_vectors(const uint8_t *img, const vpz_entropy_book *cb, Bits &p, T *chan, int chan_len, int offset, int type,
                              int partition_size)
{
    const T *lookup = values<T>(img, cb);
    const int dim = cb->dimensions;
    if (type == 0) {
        const int steps = partition_size / dim;
        for (int step = 0; step < steps; ++step) {
            const int entry = decode_scalar(img, cb, p);
            if (entry == -1) return true;
            T r = 0;
            const T *lk = lookup + (size_t)entry * dim;
            for (int d = 0; d < dim; ++d) r = (T)(r + lk[d]);
            if (offset + step < chan_len) chan[offset + step] = (T)(chan[offset + step] + r);
        }
        return false;
    }
    for (int i = 0; i < partition_size;) {
        const int entry = decode_scalar(img, cb, p);
        if (entry == -1) return true;
        const T *lk = lookup + (size_t)entry * dim;
        if (offset + i + dim > chan_len) return true;  // (never: the image's value books tile their partitions)
        for (int j = 0; j < dim; ++j) chan[offset + i + j] = (T)(chan[offset + i + j] + lk[j]);
        i += dim;
    }
    return false;
}

// Residue::decode: `count` vectors at `stride`; a class word that misses abandons every remaining stage, a vector that
// misses keeps the vectors already added.  cache: the class words of this decode (count * partition words)
template <class T>
__host__ __device__ void residue_decode(const uint8_t *img, const vpz_entropy_book *books, const vpz_entropy_residue *r, Bits &p,
                               const Mask256 &dnd, int count, int block_size, T *buffer, int stride, int32_t *cache)
{
    const int half = block_size / 2;
    const int b = r->begin < half ? r->begin : half;
    const int e = r->end < half ? r->end : half;
    const int n = e - b;
    if (n <= 0) return;
    const int psize = r->partition_size;
    const int partition_count = n / psize;
    const vpz_entropy_book *cb = books + r->class_book;
    const int dim = cb->dimensions;
    const int partition_words = (partition_count + dim - 1) / dim;
    const int words = r->decode_map_count / dim;
    const int16_t *stage_book = at<int16_t>(img, r->stage_book);
    const uint8_t *decode_map = img + r->decode_map;
    const int max_stages = r->max_stages, type = r->type;
    for (int stage = 0; stage < max_stages; ++stage) {
        for (int partition_idx = 0, entry_idx = 0; partition_idx < partition_count; ++entry_idx) {
            if (stage == 0) {
                for (int ch = 0; ch < count; ++ch) {
                    if (dnd.get(ch)) continue;
                    const int idx = decode_scalar(img, cb, p);
                    if (idx < 0 || idx >= words) return;
                    cache[ch * partition_words + entry_idx] = idx;
                }
            }
            for (int dim_idx = 0; partition_idx < partition_count && dim_idx < dim; ++dim_idx, ++partition_idx) {
                const int offset = b + partition_idx * psize;
                for (int ch = 0; ch < count; ++ch) {
                    if (dnd.get(ch)) continue;
                    const int idx = decode_map[cache[ch * partition_words + entry_idx] * dim + dim_idx];
                    const int bk = stage < 8 ? stage_book[idx * 8 + stage] : -1;
                    if (bk < 0) continue;
                    if (write_vectors<T>(img, books + bk, p, buffer + (size_t)ch * stride, stride, offset, type, psize)) return;
                }
            }
        }
    }
}

// decode_packet from the floors on, for packet k
template <class T>
__host__ __device__ void decode_one_packet(const uint8_t *img, const PacketDesc *pk, int64_t k, const uint32_t *payload, T *residue,
                                           int16_t *posts, uint8_t *post_counts, int32_t *cache, int cache_words, T *dbuf)
{
    const vpz_entropy_image_header *h = at<vpz_entropy_image_header>(img, 0);
    const int channels = h->channels;
    const PacketDesc d = pk[k];
    const uint32_t flags = d.info & 0xffu;
    const int64_t rec = k * channels;
    if (flags & VPZ_PKT_NOT_DECODED) {
        for (int c = 0; c < channels; ++c) post_counts[rec + c] = 0;
        return;
    }
    const bool bf = flags & VPZ_PKT_BLOCK_FLAG;
    const int block_size = bf ? h->block_size1 : h->block_size0;
    const int half = block_size / 2;
    const vpz_entropy_book *books = at<vpz_entropy_book>(img, h->books);
    const vpz_entropy_floor1 *floors = at<vpz_entropy_floor1>(img, h->floors);
    const vpz_entropy_residue *residues = at<vpz_entropy_residue>(img, h->residues);
    const vpz_entropy_mapping *map = at<vpz_entropy_mapping>(img, h->mappings) + (d.info >> 8);
    Bits p;
    p.words = payload;
    p.base = (uint64_t)d.payload_bit;
    p.total = d.size * 8u;
    // the floors begin after the header bits, or where the packet ends: the CPU front end's decode_packet starts at the same
    // bit (PacketHead::header_bits of host/vorbis_front.cpp, the same sum)
    const uint32_t header_bits = 1u + (uint32_t)h->mode_field_bits + (bf ? 2u : 0u);  // type bit, mode, window flags
    p.pos = header_bits < p.total ? header_bits : p.total;

    // floors, Mapping.cs:109-118
    Mask256 no_execute;
    for (int ch = 0; ch < channels; ++ch) {
        const int fl = map->submap_floor[map->mux[ch]];
        int pc = floor1_unpack(img, books, floors + fl, p, posts + (rec + ch) * 64);
        if (pc > 64) pc = 64;
        post_counts[rec + ch] = (uint8_t)pc;
        no_execute.put(ch, pc == 0);
    }
    // coupling fix-up, Mapping.cs:121-130
    const int steps = map->coupling_steps;
    for (int i = 0; i < steps; ++i) {
        const int mag = map->coupling_magnitude[i], ang = map->coupling_angle[i];
        if (!(no_execute.get(mag) && no_execute.get(ang))) {
            no_execute.put(mag, false);
            no_execute.put(ang, false);
        }
    }
    // residues, Mapping.cs:132-163
    T *dst = residue + d.residue_offset;
    int32_t *words = cache + k * cache_words;
    const int submaps = map->submaps;
    if (submaps == 1) {
        // one submap: every channel is a member in order and the decode buffer starts cleared -- decoding straight into
        // the zeroed output is decode_packet's copy of it (the Residue2 shortcut for more than one channel included)
        const vpz_entropy_residue *r = residues + map->submap_residue[0];
        if (r->type == 2) {
            bool any = false;
            for (int ch = 0; ch < channels; ++ch) any |= !no_execute.get(ch);
            if (any) residue_decode<T>(img, books, r, p, Mask256(), 1, block_size * channels, dst, half * channels, words);
        } else {
            residue_decode<T>(img, books, r, p, no_execute, channels, block_size, dst, half, words);
        }
        return;
    }
    // several submaps: decode_packet's decode buffer, reused by every submap without clearing (rows of `half` values:
    // nothing of a tiling residue reaches beyond), and the Residue2 temporary after it
    T *buf = dbuf + 2 * d.residue_offset;
    T *tmp = buf + (size_t)channels * half;
    for (int i = 0; i < channels * half; ++i) buf[i] = 0;
    for (int i = 0; i < submaps; ++i) {
        Mask256 dnd;
        int count = 0;
        for (int j = 0; j < channels; ++j)
            if (map->mux[j] == i) dnd.put(count++, no_execute.get(j));
        if (count == 0) continue;
        const vpz_entropy_residue *r = residues + map->submap_residue[i];
        if (r->type == 2) {  // Residue2.cs:12-52
            bool any = false;
            for (int kk = 0; kk < count; ++kk) any |= !dnd.get(kk);
            if (!any) {
                for (int kk = 0; kk < count * half; ++kk) buf[kk] = 0;
            } else {
                for (int kk = 0; kk < count * half; ++kk) tmp[kk] = 0;
                residue_decode<T>(img, books, r, p, Mask256(), 1, block_size * count, tmp, half * count, words);
                for (int kk = 0; kk < count; ++kk)
                    for (int bb = 0; bb < half; ++bb) buf[kk * half + bb] = tmp[bb * count + kk];
            }
        } else {
            residue_decode<T>(img, books, r, p, dnd, count, block_size, buf, half, words);
        }
        for (int j = 0, kk = 0; j < channels; ++j)
            if (map->mux[j] == i) {
                for (int bb = 0; bb < half; ++bb) dst[(size_t)j * half + bb] = buf[kk * half + bb];
                ++kk;
            }
    }
}

// one lane per packet
template <class T>
__global__ void __launch_bounds__(kBlock) entropy_decode_kernel(const uint8_t *__restrict__ img, const PacketDesc *__restrict__ pk,
                                                                int64_t n_packets, const uint32_t *__restrict__ payload, T *residue,
                                                                int16_t *posts, uint8_t *post_counts, int32_t *cache, int cache_words,
                                                                T *dbuf)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (the workgroup's size is the launch's choice, kBlock at most)
    if (k < n_packets) decode_one_packet<T>(img, pk, k, payload, residue, posts, post_counts, cache, cache_words, dbuf);
}

// the residue regions of the decoded packets, zeroed with whole rows (a workgroup per packet)
template <class T>
__global__ void __launch_bounds__(kBlock) entropy_zero_kernel(const PacketDesc *__restrict__ pk, int64_t n_packets, int channels,
                                                              int half0, int half1, T *residue)
{
    for (int64_t k = blockIdx.x; k < n_packets; k += gridDim.x) {
        const PacketDesc d = pk[k];
        if (d.info & VPZ_PKT_NOT_DECODED) continue;
        const int len = channels * ((d.info & VPZ_PKT_BLOCK_FLAG) ? half1 : half0);
        T *dst = residue + d.residue_offset;
        for (int i = threadIdx.x; i < len; i += kBlock) dst[i] = 0;
    }
}

}  // namespace
}  // namespace vpz

struct vpz_entropy_setup {
    vpz::Context *ctx = nullptr;
    std::vector<uint8_t> image;       // the validated image (host copy)
    vpz_entropy_image_header h{};
    uint8_t *d_image = nullptr;
    bool i16_ok = false;              // every residue value book has its int16 table and the image says integral
    bool multi_submap = false;        // some mapping has several submaps: the decode buffer is needed
    int cache_words = 1;              // class words one packet's residue decode keeps, at most
    // per call
    vpz::PacketDesc *h_desc = nullptr, *d_desc = nullptr;
    size_t desc_cap = 0;
    hipEvent_t desc_done = nullptr;
    bool desc_pending = false;
    void *d_cache = nullptr; size_t cache_bytes = 0;
    void *d_dbuf = nullptr; size_t dbuf_bytes = 0;
    // VPZ_MEM_HOST staging
    void *d_payload = nullptr; size_t payload_bytes = 0;
    void *d_residue = nullptr; size_t residue_bytes = 0;
    void *d_posts = nullptr; size_t posts_bytes = 0;
    void *d_counts = nullptr; size_t counts_bytes = 0;
};

namespace {

using vpz::set_error;

// bounds of the image: offset `off` holds `count` elements of T, aligned for T
template <class T> bool in_image(const std::vector<uint8_t> &img, uint32_t off, int64_t count)
{
    if (count < 0 || (off % alignof(T)) != 0) return false;
    return (uint64_t)off + (uint64_t)count * sizeof(T) <= img.size();
}
bool pow2_block(int n) { return n >= 64 && n <= 8192 && (n & (n - 1)) == 0; }

// every check the kernels rely on: nothing they index with a value from the image or the bit stream can leave the image
// or a packet's residue region
bool validate(vpz_entropy_setup &S, std::string &why)
{
    const std::vector<uint8_t> &img = S.image;
#define REQUIRE(cond, text) do { if (!(cond)) { why = text; return false; } } while (0)
    REQUIRE(img.size() >= sizeof(vpz_entropy_image_header), "image smaller than its header");
    memcpy(&S.h, img.data(), sizeof S.h);
    const vpz_entropy_image_header &h = S.h;
    REQUIRE(h.magic == VPZ_ENTROPY_IMAGE_MAGIC, "not an entropy setup image");
    REQUIRE(h.version == VPZ_ENTROPY_IMAGE_VERSION, "image version not supported");
    REQUIRE(h.total_bytes == img.size(), "image size does not match its header");
    REQUIRE(h.channels >= 1 && h.channels <= VPZ_MAX_CHANNELS, "channel count out of range");
    REQUIRE(pow2_block(h.block_size0) && pow2_block(h.block_size1) && h.block_size0 <= h.block_size1, "bad block sizes");
    REQUIRE(h.mode_field_bits >= 0 && h.mode_field_bits <= 8, "bad mode field width");
    REQUIRE(h.book_count >= 1 && h.book_count <= 256 && h.floor_count >= 1 && h.floor_count <= 64 && h.residue_count >= 1 &&
                h.residue_count <= 64 && h.mapping_count >= 1 && h.mapping_count <= 64 && h.mode_count >= 1 && h.mode_count <= 64,
            "record count out of range");
    REQUIRE(in_image<vpz_entropy_book>(img, h.books, h.book_count) && in_image<vpz_entropy_floor1>(img, h.floors, h.floor_count) &&
                in_image<vpz_entropy_residue>(img, h.residues, h.residue_count) &&
                in_image<vpz_entropy_mapping>(img, h.mappings, h.mapping_count) && in_image<vpz_entropy_mode>(img, h.modes, h.mode_count),
            "record array outside the image");
    auto rec = [&](uint32_t off, size_t i, size_t sz) { return img.data() + off + i * sz; };
    std::vector<vpz_entropy_book> books(h.book_count);
    for (int i = 0; i < h.book_count; ++i) {
        vpz_entropy_book &b = books[i];
        memcpy(&b, rec(h.books, i, sizeof b), sizeof b);
        REQUIRE(b.dimensions >= 0 && b.entries >= 0 && b.entries < (1 << 24) && b.max_bits >= 0 && b.max_bits <= 32, "bad codebook");
        REQUIRE(b.prefix_bits >= 0 && b.prefix_bits <= 10, "bad prefix table width");
        REQUIRE(b.prefix_count == 0 || (b.prefix_bits >= 1 && b.prefix_count == (1 << b.prefix_bits)), "bad prefix table size");
        REQUIRE(in_image<uint32_t>(img, b.prefix, b.prefix_count), "prefix table outside the image");
        for (int k = 0; k < b.prefix_count; ++k) {
            uint32_t wd;
            memcpy(&wd, img.data() + b.prefix + 4 * (size_t)k, 4);
            REQUIRE((wd & 63u) == 0 || ((int)(wd & 63u) <= b.prefix_bits && (wd >> 6) < (uint32_t)b.entries), "bad prefix table entry");
        }
        REQUIRE(in_image<vpz_entropy_code>(img, b.overflow, b.overflow_count), "overflow list outside the image");
        for (int k = 0; k < b.overflow_count; ++k) {
            vpz_entropy_code c;
            memcpy(&c, img.data() + b.overflow + sizeof c * (size_t)k, sizeof c);
            REQUIRE(c.value < (uint32_t)b.entries && c.length >= 1 && c.length <= 32, "bad overflow code");
        }
        const int64_t values = (int64_t)b.entries * b.dimensions;
        REQUIRE(b.lookup_count == 0 || b.lookup_count == values, "bad value table size");
        REQUIRE(b.lookup_i16_count == 0 || b.lookup_i16_count == b.lookup_count, "bad int16 value table size");
        REQUIRE(in_image<float>(img, b.lookup_f32, b.lookup_count) && in_image<int16_t>(img, b.lookup_i16, b.lookup_i16_count),
                "value table outside the image");
    }
    for (int i = 0; i < h.floor_count; ++i) {
        vpz_entropy_floor1 f;
        memcpy(&f, rec(h.floors, i, sizeof f), sizeof f);
        REQUIRE(f.partition_count >= 0 && f.partition_count <= VPZ_ENTROPY_MAX_FLOOR1_PARTITIONS && f.y_bits >= 0 && f.y_bits <= 16,
                "bad floor1 header");
        for (int k = 0; k < f.partition_count; ++k) {
            const int c = f.partition_class[k];
            REQUIRE(c < VPZ_ENTROPY_MAX_FLOOR1_CLASSES && f.class_dimensions[c] >= 1 && f.class_dimensions[c] <= 8 &&
                        f.class_subclasses[c] <= 3, "bad floor1 class");
            REQUIRE(f.class_subclasses[c] == 0 || f.class_masterbooks[c] < h.book_count, "floor1 master book out of range");
            for (int s = 0; s < (1 << f.class_subclasses[c]); ++s)
                REQUIRE(f.subclass_books[c * 8 + s] >= -1 && f.subclass_books[c * 8 + s] < h.book_count, "floor1 subclass book out of range");
        }
    }
    std::vector<vpz_entropy_residue> res(h.residue_count);
    bool i16_ok = h.residue_integral == 1;
    for (int i = 0; i < h.residue_count; ++i) {
        vpz_entropy_residue &r = res[i];
        memcpy(&r, rec(h.residues, i, sizeof r), sizeof r);
        REQUIRE(r.type >= 0 && r.type <= 2 && r.begin >= 0 && r.end >= 0 && r.partition_size >= 1 && r.classifications >= 1 &&
                    r.classifications <= 64 && r.max_stages >= 0 && r.max_stages <= 8, "bad residue header");
        REQUIRE(r.class_book >= 0 && r.class_book < h.book_count && books[r.class_book].dimensions >= 1 &&
                    r.class_dim == books[r.class_book].dimensions, "bad residue class book");
        REQUIRE(in_image<int16_t>(img, r.stage_book, (int64_t)r.classifications * 8), "stage books outside the image");
        for (int k = 0; k < r.classifications * 8; ++k) {
            int16_t bk;
            memcpy(&bk, img.data() + r.stage_book + 2 * (size_t)k, 2);
            REQUIRE(bk >= -1 && bk < h.book_count, "residue book out of range");
            if (bk < 0) continue;
            const vpz_entropy_book &vb = books[bk];
            REQUIRE(vb.dimensions >= 1 && vb.lookup_count > 0 && vb.dimensions <= r.partition_size && r.partition_size % vb.dimensions == 0,
                    "residue value book that does not tile its partitions");
            i16_ok = i16_ok && vb.lookup_i16_count == vb.lookup_count;
        }
        REQUIRE(r.decode_map_count >= 0 && r.decode_map_count % r.class_dim == 0 && in_image<uint8_t>(img, r.decode_map, r.decode_map_count),
                "bad decode map");
        for (int k = 0; k < r.decode_map_count; ++k) REQUIRE(img[r.decode_map + k] < r.classifications, "bad decode map entry");
        REQUIRE(in_image<uint32_t>(img, r.word_stage_mask, r.word_stage_mask_count), "stage masks outside the image");
    }
    S.i16_ok = i16_ok;
    S.cache_words = 1;
    for (int i = 0; i < h.mapping_count; ++i) {
        const vpz_entropy_mapping *m = reinterpret_cast<const vpz_entropy_mapping *>(rec(h.mappings, i, sizeof(vpz_entropy_mapping)));
        REQUIRE(m->submaps >= 1 && m->submaps <= VPZ_ENTROPY_MAX_SUBMAPS && m->coupling_steps >= 0 && m->coupling_steps <= VPZ_MAX_COUPLING,
                "bad mapping header");
        for (int c = 0; c < h.channels; ++c) REQUIRE(m->mux[c] < m->submaps, "mapping mux out of range");
        for (int k = 0; k < m->submaps; ++k)
            REQUIRE(m->submap_floor[k] < h.floor_count && m->submap_residue[k] < h.residue_count, "mapping submap out of range");
        for (int k = 0; k < m->coupling_steps; ++k)
            REQUIRE(m->coupling_magnitude[k] < h.channels && m->coupling_angle[k] < h.channels, "coupling channel out of range");
        S.multi_submap = S.multi_submap || m->submaps > 1;
        // the class words one packet of this mapping keeps (Residue::decode's part_word_cache)
        for (int k = 0; k < m->submaps; ++k) {
            int count = 0;
            for (int c = 0; c < h.channels; ++c) count += m->mux[c] == k;
            const vpz_entropy_residue &r = res[m->submap_residue[k]];
            for (int bs : {h.block_size0, h.block_size1}) {
                const int64_t half = r.type == 2 ? (int64_t)bs / 2 * count : bs / 2;
                const int64_t b = std::min<int64_t>(r.begin, half), e = std::min<int64_t>(r.end, half);
                if (e <= b) continue;
                const int64_t pcount = (e - b) / r.partition_size;
                const int64_t pw = (pcount + r.class_dim - 1) / r.class_dim;
                const int64_t need = (r.type == 2 ? 1 : count) * pw;
                if (need > S.cache_words) S.cache_words = (int)need;
            }
        }
    }
    for (int i = 0; i < h.mode_count; ++i) {
        vpz_entropy_mode md;
        memcpy(&md, rec(h.modes, i, sizeof md), sizeof md);
        REQUIRE((md.block_flag == 0 || md.block_flag == 1) && md.mapping >= 0 && md.mapping < h.mapping_count, "bad mode");
    }
#undef REQUIRE
    return true;
}

int grow(vpz::Context *ctx, void **buf, size_t *have, size_t need)
{
    return vpz::ensure_stage(ctx, buf, have, need < 16 ? 16 : need);
}

}  // namespace

extern "C" {

int vpz_entropy_version(void) { return VPZ_ENTROPY_VERSION; }

int vpz_entropy_setup_create(vpz_context *c, const void *image, uint64_t size, vpz_entropy_setup **out)
{
    if (!c || !image || !out || size > (1ull << 31)) return VPZ_E_INVALID_ARG;
    *out = nullptr;
    vpz::Context *ctx = &c->impl;
    vpz_entropy_setup *S = new (std::nothrow) vpz_entropy_setup();
    if (!S) return VPZ_E_NOMEM;
    S->ctx = ctx;
    S->image.assign(static_cast<const uint8_t *>(image), static_cast<const uint8_t *>(image) + size);
    std::string why;
    if (!validate(*S, why)) {
        delete S;
        return set_error(ctx, VPZ_E_INVALID_ARG, ("vpz_entropy_setup_create: " + why).c_str());
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&S->d_image), S->image.size());
    if (e == hipSuccess) e = hipMemcpy(S->d_image, S->image.data(), S->image.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&S->desc_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        vpz_entropy_setup_destroy(S);
        return set_error(ctx, VPZ_E_HIP, "vpz_entropy_setup_create", e);
    }
    *out = S;
    return VPZ_OK;
}

void vpz_entropy_setup_destroy(vpz_entropy_setup *S)
{
    if (!S) return;
    if (S->ctx) (void)hipStreamSynchronize(S->ctx->stream);
    for (void *p : {(void *)S->d_image, (void *)S->d_desc, S->d_cache, S->d_dbuf, S->d_payload, S->d_residue, S->d_posts, S->d_counts})
        if (p) (void)hipFree(p);
    if (S->h_desc) (void)hipHostFree(S->h_desc);
    if (S->desc_done) (void)hipEventDestroy(S->desc_done);
    delete S;
}

int vpz_entropy_decode(vpz_entropy_setup *S, int64_t n_packets, const vpz_packet *packets, const vpz_entropy_span *spans,
                       const uint8_t *payload, int64_t payload_bytes, int32_t residue_format, void *residue,
                       int64_t residue_values, int16_t *posts, uint8_t *post_counts, int64_t n_records, int32_t mem_space)
{
    if (!S) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = S->ctx;
    const vpz_entropy_image_header &h = S->h;
    const int C = h.channels;
    if (n_packets < 0 || payload_bytes < 0 || residue_values < 0 || n_records < 0)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: negative count or extent");
    if (mem_space != VPZ_MEM_HOST && mem_space != VPZ_MEM_DEVICE) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: bad mem_space");
    if (residue_format != VPZ_RESIDUE_F32 && residue_format != VPZ_RESIDUE_I16)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: bad residue format");
    if (residue_format == VPZ_RESIDUE_I16 && !S->i16_ok)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: int16 residue for a setup whose residue is not integral");
    if (n_packets == 0) return VPZ_OK;
    if (!packets || !spans || !payload || !posts || !post_counts)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: null argument");
    if (n_packets > (int64_t)1 << 40 || n_records < n_packets * C)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: fewer post records than packets * channels");
    const size_t esize = residue_format == VPZ_RESIDUE_I16 ? 2 : 4;
    if (mem_space == VPZ_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(payload) & 3) || (reinterpret_cast<uintptr_t>(residue) & (esize - 1)) ||
                                        (reinterpret_cast<uintptr_t>(posts) & 1)))
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: misaligned device buffer");
    // every bound first: an invalid batch writes nothing
    bool any_decoded = false;
    for (int64_t k = 0; k < n_packets; ++k) {
        const vpz_entropy_span &sp = spans[k];
        if (sp.offset < 0 || sp.size < 0 || sp.size >= ((int64_t)1 << 28) || sp.offset > payload_bytes - sp.size - 8)
            return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: a packet's span lies outside the payload");
        const vpz_packet &p = packets[k];
        if (p.flags & VPZ_PKT_NOT_DECODED) continue;
        any_decoded = true;
        if (p.mapping >= h.mapping_count) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: packet mapping index out of range");
        const int64_t len = (int64_t)C * ((p.flags & VPZ_PKT_BLOCK_FLAG) ? h.block_size1 : h.block_size0) / 2;
        if (p.residue_offset < 0 || p.residue_offset > residue_values - len)
            return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: a packet's residue lies beyond residue_values");
    }
    if (any_decoded && !residue) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: null residue");

    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc;
    // the packet descriptors, through a page-locked buffer (the previous call's copy has left it)
    if (S->desc_pending) {
        VPZ_HIP_TRY(ctx, hipEventSynchronize(S->desc_done));
        S->desc_pending = false;
    }
    if (S->desc_cap < (size_t)n_packets) {
        if (S->h_desc) VPZ_HIP_TRY(ctx, hipHostFree(S->h_desc));
        if (S->d_desc) VPZ_HIP_TRY(ctx, hipFree(S->d_desc));
        S->h_desc = nullptr;
        S->d_desc = nullptr;
        S->desc_cap = 0;
        const size_t cap = (size_t)n_packets + (size_t)n_packets / 4;
        VPZ_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&S->h_desc), cap * sizeof(vpz::PacketDesc)));
        VPZ_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&S->d_desc), cap * sizeof(vpz::PacketDesc)));
        S->desc_cap = cap;
    }
    for (int64_t k = 0; k < n_packets; ++k) {
        const vpz_packet &p = packets[k];
        vpz::PacketDesc &d = S->h_desc[k];
        d.payload_bit = spans[k].offset * 8;
        d.residue_offset = p.residue_offset;
        d.size = (uint32_t)spans[k].size;
        d.info = (uint32_t)p.flags | ((uint32_t)p.mapping << 8);
    }
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(S->d_desc, S->h_desc, sizeof(vpz::PacketDesc) * (size_t)n_packets, hipMemcpyHostToDevice, st));
    VPZ_HIP_TRY(ctx, hipEventRecord(S->desc_done, st));
    S->desc_pending = true;
    if ((rc = grow(ctx, &S->d_cache, &S->cache_bytes, sizeof(int32_t) * (size_t)n_packets * S->cache_words)) != VPZ_OK) return rc;
    if (S->multi_submap && (rc = grow(ctx, &S->d_dbuf, &S->dbuf_bytes, 2 * esize * (size_t)residue_values)) != VPZ_OK) return rc;

    const uint8_t *d_payload = payload;
    void *d_residue = residue;
    int16_t *d_posts = posts;
    uint8_t *d_counts = post_counts;
    const size_t recs = (size_t)n_packets * C;
    if (mem_space == VPZ_MEM_HOST) {
        if ((rc = grow(ctx, &S->d_payload, &S->payload_bytes, (size_t)payload_bytes + 8)) != VPZ_OK) return rc;
        if ((rc = grow(ctx, &S->d_residue, &S->residue_bytes, esize * (size_t)residue_values)) != VPZ_OK) return rc;
        if ((rc = grow(ctx, &S->d_posts, &S->posts_bytes, recs * 64 * sizeof(int16_t))) != VPZ_OK) return rc;
        if ((rc = grow(ctx, &S->d_counts, &S->counts_bytes, recs)) != VPZ_OK) return rc;
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(S->d_payload, payload, (size_t)payload_bytes, hipMemcpyHostToDevice, st));
        // (the whole extent goes both ways: what no packet writes comes back as it was)
        if (residue && residue_values)
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(S->d_residue, residue, esize * (size_t)residue_values, hipMemcpyHostToDevice, st));
        d_payload = static_cast<const uint8_t *>(S->d_payload);
        d_residue = S->d_residue;
        d_posts = static_cast<int16_t *>(S->d_posts);
        d_counts = static_cast<uint8_t *>(S->d_counts);
    }
    VPZ_HIP_TRY(ctx, hipMemsetAsync(d_posts, 0, recs * 64 * sizeof(int16_t), st));
    const unsigned zero_grid = (unsigned)std::min<int64_t>(n_packets, 8192);
    // One lane per packet, and a launch's time is the latency of its slowest lane's chain: a small launch gains from spreading its
    // waves over the CUs (a wave per workgroup: 39 000 packets are 600 workgroups on 256 CUs instead of 150 that hold four waves
    // each).  Launches of 2 900 to 39 000 packets: 2.62 / 2.73 / 2.99 ms at 64 lanes against 3.08 / 3.11 / 3.25 ms at 256
    // (tools/kbench_entropy.py, 16 / 64 / 128 streams); nothing larger was measured, so larger launches keep kBlock.
    const unsigned block = n_packets < vpz::kSmallLaunch ? 64u : (unsigned)vpz::kBlock;
    const unsigned grid = (unsigned)((n_packets + block - 1) / block);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(d_payload);
    int32_t *cache = static_cast<int32_t *>(S->d_cache);
    if (residue_format == VPZ_RESIDUE_I16) {
        if (any_decoded)
            hipLaunchKernelGGL(vpz::entropy_zero_kernel<int16_t>, dim3(zero_grid), dim3(vpz::kBlock), 0, st, S->d_desc, n_packets, C,
                               h.block_size0 / 2, h.block_size1 / 2, static_cast<int16_t *>(d_residue));
        hipLaunchKernelGGL(vpz::entropy_decode_kernel<int16_t>, dim3(grid), dim3(block), 0, st, S->d_image, S->d_desc, n_packets,
                           words, static_cast<int16_t *>(d_residue), d_posts, d_counts, cache, S->cache_words,
                           static_cast<int16_t *>(S->d_dbuf));
    } else {
        if (any_decoded)
            hipLaunchKernelGGL(vpz::entropy_zero_kernel<float>, dim3(zero_grid), dim3(vpz::kBlock), 0, st, S->d_desc, n_packets, C,
                               h.block_size0 / 2, h.block_size1 / 2, static_cast<float *>(d_residue));
        hipLaunchKernelGGL(vpz::entropy_decode_kernel<float>, dim3(grid), dim3(block), 0, st, S->d_image, S->d_desc, n_packets,
                           words, static_cast<float *>(d_residue), d_posts, d_counts, cache, S->cache_words,
                           static_cast<float *>(S->d_dbuf));
    }
    VPZ_HIP_TRY(ctx, hipGetLastError());
    if (mem_space == VPZ_MEM_HOST) {
        if (residue && residue_values)
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(residue, S->d_residue, esize * (size_t)residue_values, hipMemcpyDeviceToHost, st));
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(posts, S->d_posts, recs * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(post_counts, S->d_counts, recs, hipMemcpyDeviceToHost, st));
        VPZ_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return VPZ_OK;
}

}  // extern "C"
