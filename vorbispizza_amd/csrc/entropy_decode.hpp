// The per-packet entropy decode shared by the kernels of entropy.hip (entropy_decode_kernel: one setup per call;
// entropy_group_kernel: a setup per wave): Floor1.Unpack, the coupling fix-up of the no-residue flags and Residue0/1/2.Decode
// (Mapping.cs:109-163), bit for bit what the CPU front end's decode_packet writes (vorbispizza_amd/host/vorbis_front.cpp; every
// function below names the one it restates), and the lane list of a group call.  Everything here compiles for the host too
// (VPZ_HD), so that the whole per-packet path can run on a CPU under sanitizers before it runs on a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vorbispizza_entropy.h"

#if defined(__HIPCC__)
#define VPZ_HD __host__ __device__
#else
#define VPZ_HD
#endif

namespace vpz {
namespace {

// what the kernels know of a packet (24 bytes): where its bits are, where its residue goes, its flags and mapping
struct PacketDesc {
    int64_t payload_bit;     // bit offset of the packet in the payload
    int64_t residue_offset;  // value offset of its residue
    uint32_t size;           // bytes
    uint32_t info;           // flags | mapping << 8; in a group's lane list also setup << 16 | kLaneSkip
};

// ---- the lane list of a group call (vorbispizza_entropy_group.h): the packets ordered by setup, stable in packet order, every
// setup's run starting on a multiple of the wave size, so that the setup of a wave is one.  A lane carries its packet's descriptor
// with the setup in bits 16..23 and, beside it, the packet's index; the lanes that pad a run carry kLaneSkip (and
// VPZ_PKT_NOT_DECODED, which keeps entropy_zero_kernel off them) and write nothing.
constexpr int kWave = 64;
constexpr uint32_t kLaneSkip = 1u << 24;
VPZ_HD inline uint32_t lane_setup(uint32_t info) { return (info >> 16) & 0xffu; }

// start[s]: the first lane of setup s, per_setup[s] packets long; returns the list's length (the last run is not padded)
inline int64_t lane_list_starts(int n_setups, const int64_t *per_setup, int64_t *start)
{
    int64_t at = 0, end = 0;
    for (int s = 0; s < n_setups; ++s) {
        start[s] = at;
        if (per_setup[s] == 0) continue;
        end = at + per_setup[s];
        at = (end + kWave - 1) / kWave * kWave;
    }
    return end;
}

// fills lanes[n_lanes] / lane_packet[n_lanes] from the packets' descriptors (setup in bits 16..23); start[] is advanced to
// the runs' ends
inline void lane_list_fill(int n_setups, int64_t *start, int64_t n_packets, const PacketDesc *desc, int64_t n_lanes, PacketDesc *lanes,
                           int64_t *lane_packet)
{
    for (int64_t k = 0; k < n_packets; ++k) {
        const int64_t l = start[lane_setup(desc[k].info)]++;
        lanes[l] = desc[k];
        lane_packet[l] = k;
    }
    for (int s = 0; s < n_setups; ++s) {
        const int64_t pad_end = (start[s] + kWave - 1) / kWave * kWave;
        for (int64_t l = start[s]; l < pad_end && l < n_lanes; ++l) {
            lanes[l] = PacketDesc{0, 0, 0, (uint32_t)VPZ_PKT_NOT_DECODED | kLaneSkip | ((uint32_t)s << 16)};
            lane_packet[l] = 0;
        }
    }
}

// 256 one-bit flags in registers (a runtime-indexed array would live in scratch memory): channels of a packet
struct Mask256 {
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    VPZ_HD bool get(int i) const
    {
        const uint64_t w = i < 64 ? m0 : i < 128 ? m1 : i < 192 ? m2 : m3;
        return (w >> (i & 63)) & 1u;
    }
    VPZ_HD void put(int i, bool v)
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

    VPZ_HD uint32_t peek(int count, int &n) const
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
    VPZ_HD void skip(uint32_t count)
    {
        const uint32_t rem = total - pos;
        pos = rem >= count ? pos + count : total;
    }
    VPZ_HD uint32_t read(int count)
    {
        int n;
        const uint32_t v = peek(count, n);
        pos += (uint32_t)n;
        return v;
    }
};

template <class T> VPZ_HD const T *at(const uint8_t *img, uint32_t off) { return reinterpret_cast<const T *>(img + off); }

// Codebook::decode_scalar: the prefix table, then the overflow list in the host's order; -1 on a miss
VPZ_HD int decode_scalar(const uint8_t *img, const vpz_entropy_book *b, Bits &p)
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

VPZ_HD inline int16_t clamp16(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// Floor1::unpack -> the post count; posts are written to `out` as they are read (the record was zeroed), so that a
// miss leaves what was read before it, as the host's `raw` array does
VPZ_HD int floor1_unpack(const uint8_t *img, const vpz_entropy_book *books, const vpz_entropy_floor1 *f, Bits &p,
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

template <class T> VPZ_HD const T *values(const uint8_t *img, const vpz_entropy_book *b);
template <> VPZ_HD const float *values<float>(const uint8_t *img, const vpz_entropy_book *b) { return at<float>(img, b->lookup_f32); }
template <> VPZ_HD const int16_t *values<int16_t>(const uint8_t *img, const vpz_entropy_book *b) { return at<int16_t>(img, b->lookup_i16); }

// Residue::write_vectors: type 0 sums an entry into ONE bin, every partial sum rounded (quirk q9); types 1 / 2 add the
// vector to consecutive bins.  true: the packet ran out
template <class T>
VPZ_HD bool write_vectors(const uint8_t *img, const vpz_entropy_book *cb, Bits &p, T *chan, int chan_len, int offset, int type,
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
VPZ_HD void residue_decode(const uint8_t *img, const vpz_entropy_book *books, const vpz_entropy_residue *r, Bits &p,
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

// decode_packet from the floors on, for packet k (its records and its cache slot) with the descriptor d
template <class T>
VPZ_HD void decode_one_packet(const uint8_t *img, const PacketDesc &d, int64_t k, const uint32_t *payload, T *residue, int16_t *posts,
                              uint8_t *post_counts, int32_t *cache, int cache_words, T *dbuf)
{
    const vpz_entropy_image_header *h = at<vpz_entropy_image_header>(img, 0);
    const int channels = h->channels;
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
    const vpz_entropy_mapping *map = at<vpz_entropy_mapping>(img, h->mappings) + ((d.info >> 8) & 0xffu);
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

// one lane of a group call; `img` is the image of the lane's setup
template <class T>
VPZ_HD void decode_group_lane(const uint8_t *img, const PacketDesc &d, int64_t packet, const uint32_t *payload, T *residue,
                              int16_t *posts, uint8_t *post_counts, int32_t *cache, int cache_words, T *dbuf)
{
    if (d.info & kLaneSkip) return;
    decode_one_packet<T>(img, d, packet, payload, residue, posts, post_counts, cache, cache_words, dbuf);
}

}  // namespace
}  // namespace vpz
