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
#include "entropy_decode.hpp"
#include "../../include/vorbispizza_entropy_group.h"

namespace vpz {
namespace {

constexpr int kBlock = 256;
constexpr int64_t kSmallLaunch = 65536;  // packets below which entropy_decode_kernel is launched with one wave per workgroup

// one lane per packet
template <class T>
__global__ void __launch_bounds__(kBlock) entropy_decode_kernel(const uint8_t *__restrict__ img, const PacketDesc *__restrict__ pk,
                                                                int64_t n_packets, const uint32_t *__restrict__ payload, T *residue,
                                                                int16_t *posts, uint8_t *post_counts, int32_t *cache, int cache_words,
                                                                T *dbuf)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (the workgroup's size is the launch's choice, kBlock at most)
    if (k >= n_packets) return;
    const PacketDesc d = pk[k];
    decode_one_packet<T>(img, d, k, payload, residue, posts, post_counts, cache, cache_words, dbuf);
}

// A group call: one lane per entry of the lane list (entropy_decode.hpp), whose runs start on whole waves -- the setup of a wave is
// one, read once and made scalar, so that the image's address, its header fields and record arrays stay in scalar registers as
// they do above, where the image is a kernel argument.  (Both launch sizes are multiples of the wave size.)
// (The table's entries are typed as addresses of global memory: of a plain pointer read from memory the compiler knows no address
// space, and every load from the image would be a flat one.)
using ImageAddress = const __attribute__((address_space(1))) uint8_t *;
template <class T>
__global__ void __launch_bounds__(kBlock) entropy_group_kernel(const ImageAddress *__restrict__ images, const PacketDesc *__restrict__ lanes,
                                                               const int64_t *__restrict__ lane_packet, int64_t n_lanes,
                                                               const uint32_t *__restrict__ payload, T *residue, int16_t *posts,
                                                               uint8_t *post_counts, int32_t *cache, int cache_words, T *dbuf)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_lanes) return;
    const PacketDesc d = lanes[l];
    const uint8_t *img = (const uint8_t *)images[__builtin_amdgcn_readfirstlane((int)lane_setup(d.info))];
    decode_group_lane<T>(img, d, lane_packet[l], payload, residue, posts, post_counts, cache, cache_words, dbuf);
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

namespace vpz {
namespace {

// a validated setup image and what the launches need to know of it
struct EntropyImage {
    std::vector<uint8_t> image;       // the validated image (host copy)
    vpz_entropy_image_header h{};
    uint8_t *d_image = nullptr;
    bool i16_ok = false;              // every residue value book has its int16 table and the image says integral
    bool multi_submap = false;        // some mapping has several submaps: the decode buffer is needed
    int cache_words = 1;              // class words one packet's residue decode keeps, at most
};

// what a call needs on the device, kept between the calls of one setup or one group
struct CallScratch {
    PacketDesc *h_desc = nullptr, *d_desc = nullptr;    // the packet descriptors (a group: its lane list)
    int64_t *h_index = nullptr, *d_index = nullptr;     // a group: the packet of every lane
    size_t desc_cap = 0;
    hipEvent_t desc_done = nullptr;
    bool desc_pending = false;
    Scratch cache, dbuf;
    Scratch payload, residue, posts, counts;  // VPZ_MEM_HOST staging
};

}  // namespace
}  // namespace vpz

struct vpz_entropy_setup {
    vpz::Context *ctx = nullptr;
    vpz::EntropyImage img;
    vpz::CallScratch call;
};

struct vpz_entropy_group {
    vpz::Context *ctx = nullptr;
    std::vector<vpz::EntropyImage> images;
    void *d_table = nullptr;            // the images' device addresses (ImageAddress[n_setups])
    int channels = 0, block_size0 = 0, block_size1 = 0;
    bool i16_ok = true;                 // every setup allows the int16 residue
    bool multi_submap = false;          // any setup needs the decode buffer
    int cache_words = 1;                // the largest any setup needs
    std::vector<vpz::PacketDesc> desc;  // per call: the packets' descriptors before they are ordered
    vpz::CallScratch call;
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
bool validate(vpz::EntropyImage &S, std::string &why)
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

int grow(vpz::Context *ctx, vpz::Scratch &b, size_t need)
{
    return b.grow(ctx, need < 16 ? 16 : need, "hipMalloc(staging)");
}

int upload_image(vpz::Context *ctx, vpz::EntropyImage &I)
{
    VPZ_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&I.d_image), I.image.size()));
    VPZ_HIP_TRY(ctx, hipMemcpy(I.d_image, I.image.data(), I.image.size(), hipMemcpyHostToDevice));
    return VPZ_OK;
}

void release(vpz::CallScratch &K)
{
    for (void *p : {(void *)K.d_desc, (void *)K.d_index, K.cache.p, K.dbuf.p, K.payload.p, K.residue.p, K.posts.p, K.counts.p})
        if (p) (void)hipFree(p);
    if (K.h_desc) (void)hipHostFree(K.h_desc);
    if (K.h_index) (void)hipHostFree(K.h_index);
    if (K.desc_done) (void)hipEventDestroy(K.desc_done);
    K = vpz::CallScratch();
}

// the arguments both decode calls check alike, before anything that knows a setup
int check_call(vpz::Context *ctx, const char *who, int64_t n_packets, const vpz_packet *packets, const vpz_entropy_span *spans,
               const uint8_t *payload, int64_t payload_bytes, int32_t residue_format, bool i16_ok, const void *residue,
               int64_t residue_values, const int16_t *posts, const uint8_t *post_counts, int64_t n_records, int channels,
               int32_t mem_space)
{
    auto fail = [&](const char *text) { return set_error(ctx, VPZ_E_INVALID_ARG, (std::string(who) + ": " + text).c_str()); };
    if (n_packets < 0 || payload_bytes < 0 || residue_values < 0 || n_records < 0) return fail("negative count or extent");
    if (mem_space != VPZ_MEM_HOST && mem_space != VPZ_MEM_DEVICE) return fail("bad mem_space");
    if (residue_format != VPZ_RESIDUE_F32 && residue_format != VPZ_RESIDUE_I16) return fail("bad residue format");
    if (residue_format == VPZ_RESIDUE_I16 && !i16_ok) return fail("int16 residue for a setup whose residue is not integral");
    if (n_packets == 0) return VPZ_OK;
    if (!packets || !spans || !payload || !posts || !post_counts) return fail("null argument");
    if (n_packets > (int64_t)1 << 40 || n_records < n_packets * channels) return fail("fewer post records than packets * channels");
    const size_t esize = residue_format == VPZ_RESIDUE_I16 ? 2 : 4;
    if (mem_space == VPZ_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(payload) & 3) || (reinterpret_cast<uintptr_t>(residue) & (esize - 1)) ||
                                        (reinterpret_cast<uintptr_t>(posts) & 1)))
        return fail("misaligned device buffer");
    return VPZ_OK;
}

// the bounds of packet k that no setup decides: its span; for a decoded packet, its residue of `len` values
const char *check_packet(const vpz_packet &p, const vpz_entropy_span &sp, int64_t payload_bytes, int channels, int block_size0,
                         int block_size1, int64_t residue_values)
{
    if (sp.offset < 0 || sp.size < 0 || sp.size >= ((int64_t)1 << 28) || sp.offset > payload_bytes - sp.size - 8)
        return "a packet's span lies outside the payload";
    if (p.flags & VPZ_PKT_NOT_DECODED) return nullptr;
    const int64_t len = (int64_t)channels * ((p.flags & VPZ_PKT_BLOCK_FLAG) ? block_size1 : block_size0) / 2;
    if (p.residue_offset < 0 || p.residue_offset > residue_values - len) return "a packet's residue lies beyond residue_values";
    return nullptr;
}

vpz::PacketDesc describe(const vpz_packet &p, const vpz_entropy_span &sp, uint32_t mapping, uint32_t setup)
{
    return vpz::PacketDesc{sp.offset * 8, p.residue_offset, (uint32_t)sp.size, (uint32_t)p.flags | (mapping << 8) | (setup << 16)};
}

// room for n descriptors (and, for a group, n lane indices) in the page-locked buffer; the previous call's copy has left it
int desc_room(vpz::Context *ctx, vpz::CallScratch &K, int64_t n, bool with_index)
{
    if (K.desc_pending) {
        VPZ_HIP_TRY(ctx, hipEventSynchronize(K.desc_done));
        K.desc_pending = false;
    }
    if (K.desc_cap >= (size_t)n) return VPZ_OK;
    if (K.h_desc) VPZ_HIP_TRY(ctx, hipHostFree(K.h_desc));
    K.h_desc = nullptr;
    if (K.d_desc) VPZ_HIP_TRY(ctx, hipFree(K.d_desc));
    K.d_desc = nullptr;
    if (K.h_index) VPZ_HIP_TRY(ctx, hipHostFree(K.h_index));
    K.h_index = nullptr;
    if (K.d_index) VPZ_HIP_TRY(ctx, hipFree(K.d_index));
    K.d_index = nullptr;
    K.desc_cap = 0;
    const size_t cap = (size_t)n + (size_t)n / 4;
    VPZ_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&K.h_desc), cap * sizeof(vpz::PacketDesc)));
    VPZ_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&K.d_desc), cap * sizeof(vpz::PacketDesc)));
    if (with_index) {
        VPZ_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&K.h_index), cap * sizeof(int64_t)));
        VPZ_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&K.d_index), cap * sizeof(int64_t)));
    }
    K.desc_cap = cap;
    return VPZ_OK;
}

int upload_descs(vpz::Context *ctx, vpz::CallScratch &K, int64_t n, bool with_index)
{
    hipStream_t st = ctx->stream;
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(K.d_desc, K.h_desc, sizeof(vpz::PacketDesc) * (size_t)n, hipMemcpyHostToDevice, st));
    if (with_index) VPZ_HIP_TRY(ctx, hipMemcpyAsync(K.d_index, K.h_index, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    VPZ_HIP_TRY(ctx, hipEventRecord(K.desc_done, st));
    K.desc_pending = true;
    return VPZ_OK;
}

// the buffers the kernels work on: the caller's (VPZ_MEM_DEVICE) or the staging copies (VPZ_MEM_HOST)
struct Buffers {
    const uint8_t *payload;
    void *residue;
    int16_t *posts;
    uint8_t *counts;
};

// the class-word cache and the decode buffer, the staging copies in, the post records cleared
int stage_in(vpz::Context *ctx, vpz::CallScratch &K, int64_t n_packets, int channels, int cache_words, bool multi_submap, size_t esize,
             int32_t mem_space, const uint8_t *payload, int64_t payload_bytes, void *residue, int64_t residue_values, int16_t *posts,
             uint8_t *post_counts, Buffers &B)
{
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = grow(ctx, K.cache, sizeof(int32_t) * (size_t)n_packets * cache_words)) != VPZ_OK) return rc;
    if (multi_submap && (rc = grow(ctx, K.dbuf, 2 * esize * (size_t)residue_values)) != VPZ_OK) return rc;
    B = Buffers{payload, residue, posts, post_counts};
    const size_t recs = (size_t)n_packets * channels;
    if (mem_space == VPZ_MEM_HOST) {
        if ((rc = grow(ctx, K.payload, (size_t)payload_bytes + 8)) != VPZ_OK) return rc;
        if ((rc = grow(ctx, K.residue, esize * (size_t)residue_values)) != VPZ_OK) return rc;
        if ((rc = grow(ctx, K.posts, recs * 64 * sizeof(int16_t))) != VPZ_OK) return rc;
        if ((rc = grow(ctx, K.counts, recs)) != VPZ_OK) return rc;
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(K.payload.p, payload, (size_t)payload_bytes, hipMemcpyHostToDevice, st));
        // (the whole extent goes both ways: what no packet writes comes back as it was)
        if (residue && residue_values)
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(K.residue.p, residue, esize * (size_t)residue_values, hipMemcpyHostToDevice, st));
        B = Buffers{static_cast<const uint8_t *>(K.payload.p), K.residue.p, static_cast<int16_t *>(K.posts.p),
                    static_cast<uint8_t *>(K.counts.p)};
    }
    VPZ_HIP_TRY(ctx, hipMemsetAsync(B.posts, 0, recs * 64 * sizeof(int16_t), st));
    return VPZ_OK;
}

// after the launches: their status; VPZ_MEM_HOST: the staging copies out and a synchronise
int stage_out(vpz::Context *ctx, vpz::CallScratch &K, int64_t n_packets, int channels, size_t esize, int32_t mem_space, void *residue,
              int64_t residue_values, int16_t *posts, uint8_t *post_counts)
{
    hipStream_t st = ctx->stream;
    VPZ_HIP_TRY(ctx, hipGetLastError());
    if (mem_space != VPZ_MEM_HOST) return VPZ_OK;
    const size_t recs = (size_t)n_packets * channels;
    if (residue && residue_values)
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(residue, K.residue.p, esize * (size_t)residue_values, hipMemcpyDeviceToHost, st));
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(posts, K.posts.p, recs * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(post_counts, K.counts.p, recs, hipMemcpyDeviceToHost, st));
    VPZ_HIP_TRY(ctx, hipStreamSynchronize(st));
    return VPZ_OK;
}

// One lane per packet, and a launch's time is the latency of its slowest lane's chain: a small launch gains from spreading its
// waves over the CUs (a wave per workgroup: 39 000 packets are 600 workgroups on 256 CUs instead of 150 that hold four waves
// each).  Launches of 2 900 to 39 000 packets: 2.62 / 2.73 / 2.99 ms at 64 lanes against 3.08 / 3.11 / 3.25 ms at 256
// (tools/kbench_entropy.py, 16 / 64 / 128 streams); nothing larger was measured, so larger launches keep kBlock.
unsigned launch_block(int64_t lanes) { return lanes < vpz::kSmallLaunch ? 64u : (unsigned)vpz::kBlock; }

template <class T>
void launch_setup(vpz_entropy_setup *S, int64_t n_packets, bool any_decoded, const Buffers &B, hipStream_t st)
{
    const vpz_entropy_image_header &h = S->img.h;
    const unsigned zero_grid = (unsigned)std::min<int64_t>(n_packets, 8192);
    const unsigned block = launch_block(n_packets);
    const unsigned grid = (unsigned)((n_packets + block - 1) / block);
    if (any_decoded)
        hipLaunchKernelGGL(vpz::entropy_zero_kernel<T>, dim3(zero_grid), dim3(vpz::kBlock), 0, st, S->call.d_desc, n_packets, h.channels,
                           h.block_size0 / 2, h.block_size1 / 2, static_cast<T *>(B.residue));
    hipLaunchKernelGGL(vpz::entropy_decode_kernel<T>, dim3(grid), dim3(block), 0, st, S->img.d_image, S->call.d_desc, n_packets,
                       reinterpret_cast<const uint32_t *>(B.payload), static_cast<T *>(B.residue), B.posts, B.counts,
                       static_cast<int32_t *>(S->call.cache.p), S->img.cache_words, static_cast<T *>(S->call.dbuf.p));
}

// the same two passes over a group's lane list
template <class T>
void launch_group(vpz_entropy_group *G, int64_t n_lanes, bool any_decoded, const Buffers &B, hipStream_t st)
{
    const unsigned zero_grid = (unsigned)std::min<int64_t>(n_lanes, 8192);
    const unsigned block = launch_block(n_lanes);
    const unsigned grid = (unsigned)((n_lanes + block - 1) / block);
    if (any_decoded)
        hipLaunchKernelGGL(vpz::entropy_zero_kernel<T>, dim3(zero_grid), dim3(vpz::kBlock), 0, st, G->call.d_desc, n_lanes, G->channels,
                           G->block_size0 / 2, G->block_size1 / 2, static_cast<T *>(B.residue));
    hipLaunchKernelGGL(vpz::entropy_group_kernel<T>, dim3(grid), dim3(block), 0, st, static_cast<const vpz::ImageAddress *>(G->d_table), G->call.d_desc, G->call.d_index,
                       n_lanes,
                       reinterpret_cast<const uint32_t *>(B.payload), static_cast<T *>(B.residue), B.posts, B.counts,
                       static_cast<int32_t *>(G->call.cache.p), G->cache_words, static_cast<T *>(G->call.dbuf.p));
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
    try {  // (the host copy, validate's tables, the error text: no exception leaves the C ABI)
        S->img.image.assign(static_cast<const uint8_t *>(image), static_cast<const uint8_t *>(image) + size);
        std::string why;
        if (!validate(S->img, why)) {
            delete S;
            return set_error(ctx, VPZ_E_INVALID_ARG, ("vpz_entropy_setup_create: " + why).c_str());
        }
    } catch (const std::bad_alloc &) {
        delete S;
        return VPZ_E_NOMEM;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&S->img.d_image), S->img.image.size());
    if (e == hipSuccess) e = hipMemcpy(S->img.d_image, S->img.image.data(), S->img.image.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&S->call.desc_done, hipEventDisableTiming);
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
    if (S->img.d_image) (void)hipFree(S->img.d_image);
    release(S->call);
    delete S;
}

int vpz_entropy_decode(vpz_entropy_setup *S, int64_t n_packets, const vpz_packet *packets, const vpz_entropy_span *spans,
                       const uint8_t *payload, int64_t payload_bytes, int32_t residue_format, void *residue,
                       int64_t residue_values, int16_t *posts, uint8_t *post_counts, int64_t n_records, int32_t mem_space)
try {
    if (!S) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = S->ctx;
    const vpz_entropy_image_header &h = S->img.h;
    const int C = h.channels;
    int rc = check_call(ctx, "vpz_entropy_decode", n_packets, packets, spans, payload, payload_bytes, residue_format, S->img.i16_ok, residue,
                        residue_values, posts, post_counts, n_records, C, mem_space);
    if (rc != VPZ_OK || n_packets == 0) return rc;
    const size_t esize = residue_format == VPZ_RESIDUE_I16 ? 2 : 4;
    // every bound first: an invalid batch writes nothing
    bool any_decoded = false;
    for (int64_t k = 0; k < n_packets; ++k) {
        const vpz_packet &p = packets[k];
        if (const char *why = check_packet(p, spans[k], payload_bytes, C, h.block_size0, h.block_size1, residue_values))
            return set_error(ctx, VPZ_E_INVALID_ARG, (std::string("vpz_entropy_decode: ") + why).c_str());
        if (p.flags & VPZ_PKT_NOT_DECODED) continue;
        any_decoded = true;
        if (p.mapping >= h.mapping_count) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: packet mapping index out of range");
    }
    if (any_decoded && !residue) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_decode: null residue");

    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    vpz::CallScratch &K = S->call;
    if ((rc = desc_room(ctx, K, n_packets, false)) != VPZ_OK) return rc;
    for (int64_t k = 0; k < n_packets; ++k) K.h_desc[k] = describe(packets[k], spans[k], packets[k].mapping, 0);
    if ((rc = upload_descs(ctx, K, n_packets, false)) != VPZ_OK) return rc;
    Buffers B;
    if ((rc = stage_in(ctx, K, n_packets, C, S->img.cache_words, S->img.multi_submap, esize, mem_space, payload, payload_bytes, residue,
                       residue_values, posts, post_counts, B)) != VPZ_OK)
        return rc;
    if (residue_format == VPZ_RESIDUE_I16) launch_setup<int16_t>(S, n_packets, any_decoded, B, ctx->stream);
    else launch_setup<float>(S, n_packets, any_decoded, B, ctx->stream);
    return stage_out(ctx, K, n_packets, C, esize, mem_space, residue, residue_values, posts, post_counts);
} catch (const std::bad_alloc &) {  // (the descriptors, an error text: no exception leaves the C ABI)
    return VPZ_E_NOMEM;
}

}  // extern "C"

namespace {

// vpz_entropy_group_create once its arguments are there: the images validated and uploaded into *G (may throw std::bad_alloc;
// whatever it returns or throws, the caller destroys a group that is not VPZ_OK)
int fill_group(vpz::Context *ctx, vpz_entropy_group *G, const void *const *images, const uint64_t *sizes, int32_t n_setups)
{
    G->images.resize(n_setups);
    auto refuse = [&](const std::string &why) { return set_error(ctx, VPZ_E_INVALID_ARG, ("vpz_entropy_group_create: " + why).c_str()); };
    for (int s = 0; s < n_setups; ++s) {
        vpz::EntropyImage &I = G->images[s];
        if (!images[s] || sizes[s] > (1ull << 31)) return refuse("image " + std::to_string(s) + ": null or too large");
        I.image.assign(static_cast<const uint8_t *>(images[s]), static_cast<const uint8_t *>(images[s]) + sizes[s]);
        std::string why;
        if (!validate(I, why)) return refuse("image " + std::to_string(s) + ": " + why);
        const vpz_entropy_image_header &h0 = G->images[0].h;
        if (I.h.channels != h0.channels || I.h.block_size0 != h0.block_size0 || I.h.block_size1 != h0.block_size1)
            return refuse("image " + std::to_string(s) + ": channels or block sizes differ from image 0");
        G->i16_ok = G->i16_ok && I.i16_ok;
        G->multi_submap = G->multi_submap || I.multi_submap;
        G->cache_words = std::max(G->cache_words, I.cache_words);
    }
    G->channels = G->images[0].h.channels;
    G->block_size0 = G->images[0].h.block_size0;
    G->block_size1 = G->images[0].h.block_size1;
    auto upload = [&]() -> int {
        VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<const uint8_t *> table(n_setups);
        for (int s = 0; s < n_setups; ++s) {
            const int rc = upload_image(ctx, G->images[s]);
            if (rc != VPZ_OK) return rc;
            table[s] = G->images[s].d_image;
        }
        VPZ_HIP_TRY(ctx, hipMalloc(&G->d_table, sizeof(uint8_t *) * (size_t)n_setups));
        VPZ_HIP_TRY(ctx, hipMemcpy(G->d_table, table.data(), sizeof(uint8_t *) * (size_t)n_setups, hipMemcpyHostToDevice));
        VPZ_HIP_TRY(ctx, hipEventCreateWithFlags(&G->call.desc_done, hipEventDisableTiming));
        return VPZ_OK;
    };
    return upload();
}

}  // namespace

extern "C" {

int vpz_entropy_group_create(vpz_context *c, const void *const *images, const uint64_t *sizes, int32_t n_setups, vpz_entropy_group **out)
{
    if (!c || !out) return VPZ_E_INVALID_ARG;
    *out = nullptr;
    vpz::Context *ctx = &c->impl;
    if (!images || !sizes) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_group_create: null argument");
    if (n_setups < 1 || n_setups > VPZ_ENTROPY_GROUP_MAX_SETUPS)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_entropy_group_create: n_setups outside 1 .. 256");
    vpz_entropy_group *G = new (std::nothrow) vpz_entropy_group();
    if (!G) return VPZ_E_NOMEM;
    G->ctx = ctx;
    int rc;
    try {
        rc = fill_group(ctx, G, images, sizes, n_setups);
    } catch (const std::bad_alloc &) {  // (no exception leaves the C ABI)
        rc = VPZ_E_NOMEM;
    }
    if (rc != VPZ_OK) {
        vpz_entropy_group_destroy(G);  // (nothing stays allocated)
        return rc;
    }
    *out = G;
    return VPZ_OK;
}

void vpz_entropy_group_destroy(vpz_entropy_group *G)
{
    if (!G) return;
    if (G->ctx) (void)hipStreamSynchronize(G->ctx->stream);
    for (vpz::EntropyImage &I : G->images)
        if (I.d_image) (void)hipFree(I.d_image);
    if (G->d_table) (void)hipFree(G->d_table);
    release(G->call);
    delete G;
}

int vpz_entropy_group_decode(vpz_entropy_group *G, int32_t n_streams, const uint8_t *stream_setup, const uint8_t *stream_mapping_base,
                             int64_t n_packets, const vpz_packet *packets, const vpz_entropy_span *spans, const uint8_t *payload,
                             int64_t payload_bytes, int32_t residue_format, void *residue, int64_t residue_values, int16_t *posts,
                             uint8_t *post_counts, int64_t n_records, int32_t mem_space)
try {
    if (!G) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = G->ctx;
    const int C = G->channels, n_setups = (int)G->images.size();
    auto fail = [&](const char *why) { return set_error(ctx, VPZ_E_INVALID_ARG, (std::string("vpz_entropy_group_decode: ") + why).c_str()); };
    if (n_streams < 0) return fail("negative stream count");
    int rc = check_call(ctx, "vpz_entropy_group_decode", n_packets, packets, spans, payload, payload_bytes, residue_format, G->i16_ok, residue,
                        residue_values, posts, post_counts, n_records, C, mem_space);
    if (rc != VPZ_OK) return rc;
    if (n_streams > 0 && (!stream_setup || !stream_mapping_base)) return fail("null argument");
    for (int32_t s = 0; s < n_streams; ++s)
        if (stream_setup[s] >= n_setups) return fail("a stream's setup index out of range");
    if (n_packets == 0) return VPZ_OK;
    const size_t esize = residue_format == VPZ_RESIDUE_I16 ? 2 : 4;
    // every bound first: an invalid batch writes nothing.  The descriptors are written on the way, in packet order
    bool any_decoded = false;
    G->desc.resize((size_t)n_packets);
    int64_t per_setup[VPZ_ENTROPY_GROUP_MAX_SETUPS] = {0}, start[VPZ_ENTROPY_GROUP_MAX_SETUPS];
    for (int64_t k = 0; k < n_packets; ++k) {
        const vpz_packet &p = packets[k];
        if (p.stream < 0 || p.stream >= n_streams) return fail("a packet's stream index out of range");
        if (const char *why = check_packet(p, spans[k], payload_bytes, C, G->block_size0, G->block_size1, residue_values)) return fail(why);
        const int setup = stream_setup[p.stream];
        int mapping = 0;  // (a packet that is not decoded reads no mapping)
        if (!(p.flags & VPZ_PKT_NOT_DECODED)) {
            any_decoded = true;
            mapping = (int)p.mapping - (int)stream_mapping_base[p.stream];
            if (mapping < 0 || mapping >= G->images[setup].h.mapping_count) return fail("packet mapping index outside its setup's mappings");
        }
        G->desc[k] = describe(p, spans[k], (uint32_t)mapping, (uint32_t)setup);
        ++per_setup[setup];
    }
    if (any_decoded && !residue) return fail("null residue");
    const int64_t n_lanes = vpz::lane_list_starts(n_setups, per_setup, start);

    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    vpz::CallScratch &K = G->call;
    if ((rc = desc_room(ctx, K, n_lanes, true)) != VPZ_OK) return rc;
    vpz::lane_list_fill(n_setups, start, n_packets, G->desc.data(), n_lanes, K.h_desc, K.h_index);
    if ((rc = upload_descs(ctx, K, n_lanes, true)) != VPZ_OK) return rc;
    Buffers B;
    if ((rc = stage_in(ctx, K, n_packets, C, G->cache_words, G->multi_submap, esize, mem_space, payload, payload_bytes, residue,
                       residue_values, posts, post_counts, B)) != VPZ_OK)
        return rc;
    if (residue_format == VPZ_RESIDUE_I16) launch_group<int16_t>(G, n_lanes, any_decoded, B, ctx->stream);
    else launch_group<float>(G, n_lanes, any_decoded, B, ctx->stream);
    return stage_out(ctx, K, n_packets, C, esize, mem_space, residue, residue_values, posts, post_counts);
} catch (const std::bad_alloc &) {  // (the descriptors, an error text: no exception leaves the C ABI)
    return VPZ_E_NOMEM;
}

}  // extern "C"
