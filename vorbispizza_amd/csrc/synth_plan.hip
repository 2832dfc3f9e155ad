// The host plan of a vpz_decoder_synth call (synth_plan.hpp).  Mirrors, with integers only, what StreamDecoder.ReadNextPacket /
// Read and Mode.GetPacketInfo decide per packet (StreamDecoder.cs:418-498, 640-694; Mode.cs:30-66) and turns a batch of
// packets into frame / run descriptors for the kernels.  No sample arithmetic and no device work happens here.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "synth_plan.hpp"

namespace vpz {

// plan_runs, THE SKEW: how much heavier (per mille) the runs of the first half of a batch's work are cut
constexpr int kCutSkewPermille = 25;

namespace {

constexpr int64_t kNone = INT64_MAX;

// ---- the rules of ReadNextPacket, each stated once -------------------------------------------------------------------------

// What precedes a packet in its stream: the window of the block held in _prevPacketBuf
struct Prev {
    bool has_prev, prev_long;
    int prev_end, prev_stop;
};
inline Prev prev_of_state(const StreamState &S) { return Prev{S.has_prev, S.prev_long, S.prev_end, S.prev_stop}; }
// ... of packet p of a batch sorted by stream: the packet before it when that belongs to the same stream, else the stream's
// saved state
inline Prev prev_of(const Decoder &D, const vpz_packet *packets, int64_t p)
{
    if (p > 0 && packets[p - 1].stream == packets[p].stream) {
        const vpz_packet &pp = packets[p - 1];
        const PacketInfo &ppi = D.packet_info[pp.flags & 7];
        return Prev{true, (pp.flags & VPZ_PKT_BLOCK_FLAG) != 0, ppi.right_start, ppi.right_end};
    }
    return prev_of_state(D.states[packets[p].stream]);
}

// EOS trim (:658-666): the packet's rightStart, given the stream position in front of the packet
inline int trimmed_right_start(const PacketInfo &pi, const vpz_packet &pk, const Prev &pv, int64_t position)
{
    int right_start = pi.right_start;
    if (pk.granule != -1 && (pk.flags & VPZ_PKT_EOS)) {
        const int64_t actual_end = position + (pv.has_prev ? pv.prev_stop - pv.prev_end : 0);  // + packetLen (:654)
        const int diff = (int)(actual_end - pk.granule);
        if (diff > 0) right_start = std::max(right_start - diff, 0);
    }
    return right_start;
}

// The frame of one packet: what it overlaps with and what it emits
struct FrameGeom {
    bool mismatch;
    int packet_len, left_start, out_count;
};
inline FrameGeom frame_geometry(const Decoder &D, const PacketInfo &pi, const Prev &pv, int right_start)
{
    FrameGeom g{};
    if (pv.has_prev) {  // :670-675
        g.packet_len = pv.prev_stop - pv.prev_end;  // :654
        // windowSlope.AsSpan(0, packetLen) would throw (:778): that Read fails, the packet is
        // consumed and the decoder state stays as it was.  The rest of the batch is still
        // synthesised; the call reports the condition at the end.
        if (g.packet_len > (pi.left_use_size1 ? D.size1 : D.size0) / 2) {
            g.mismatch = true;
            g.packet_len = 0;
            return g;
        }
        g.left_start = pi.left_start;
    } else {
        g.left_start = right_start;  // :679 first packet has no valid data before rightStart
    }
    // a trim below LeftStart would make the reference spin (copyLen <= 0, :469-472): emit nothing
    g.out_count = std::max(0, right_start - g.left_start);
    return g;
}

// Granule pick-up (:459-463): a packet that carries a granule position gives a stream without a position one -- the granule is
// where the packet's `samples` end.  Sets the position in FRONT of them.
inline void pick_up_position(const vpz_packet &pk, int64_t samples, bool &has_position, int64_t &position)
{
    if (pk.granule == -1 || has_position) return;
    has_position = true;
    position = pk.granule - samples;
}

// The state a packet leaves: it is the block in _prevPacketBuf now, its tail runs from `end` to `stop`
inline void leave_state(StreamState &S, bool is_long, int end, int stop)
{
    S.has_prev = true;
    S.prev_long = is_long;
    S.prev_end = end;
    S.prev_stop = stop;
    S.prev_start = S.prev_end;  // everything readable is handed out by this call
}

// The per-record floor bytes of one packet: floor index | 0x40 type-0 | 0x80 long block, 0 for an already floored packet
inline void fill_rec_floor(const Decoder &D, const vpz_packet &pk, uint8_t *dst)
{
    if (pk.flags & VPZ_PKT_NO_FLOOR) {
        for (int ch = 0; ch < D.channels; ++ch) dst[ch] = 0;
        return;
    }
    const vpz_mapping_config &mc = D.mappings[pk.mapping];
    const uint8_t long_bit = (pk.flags & VPZ_PKT_BLOCK_FLAG) ? 0x80 : 0;
    for (int ch = 0; ch < D.channels; ++ch) {
        const uint8_t fl = mc.channel_floor[ch];
        const bool f0 = D.floor_types[fl] == 0;
        dst[ch] = (uint8_t)(fl | long_bit | (f0 ? 0x40 : 0));
    }
}

// flag bits of a decoded packet's frame: block / window selection, and what group mode needs to know about the
// packet's input (layout, coupling steps of its mapping)
inline uint32_t frame_flags(const Decoder &D, const vpz_packet &pk, const PacketInfo &pi)
{
    const bool bf = pk.flags & VPZ_PKT_BLOCK_FLAG, no_floor = pk.flags & VPZ_PKT_NO_FLOOR;
    uint32_t f = (bf ? kFrameLong : 0u) | (pi.left_use_size1 ? kFrameSlope1 : 0u) | (no_floor ? kFrameNoFloor : 0u);
    if (D.group_ok || D.dual_ok) {
        const int steps = no_floor ? 0 : D.mappings[pk.mapping].coupling_steps;
        if (pk.flags & VPZ_PKT_INTERLEAVED) f |= kFrameInterleaved;
        if (steps > 0 && D.wide_steps)  // (the pair route alone -- dual_ok on its own table's limits -- puts its own bits in)
            f |= ((uint32_t)steps << kFrameStepsShift) |
                 ((uint32_t)(D.mapping_steps_off[pk.mapping] / 2) << kFrameStepsOffShift);
    }
    if (!no_floor) f |= (uint32_t)D.mapping_skip[bf ? 1 : 0][pk.mapping] << kFrameSkipShift;
    return f;
}
// ... and its explicit descriptor
inline FrameDesc frame_desc(const Decoder &D, const vpz_packet &pk, int64_t p, const PacketInfo &pi, const Prev &pv,
                            const FrameGeom &g, int64_t out_off)
{
    FrameDesc fd{};
    fd.rec = (int32_t)(p * D.channels);
    fd.out_off = out_off;
    fd.flags = g.mismatch ? kFrameDrain : frame_flags(D, pk, pi);  // skipped packet (window mismatch): a frame that does nothing
    if (g.mismatch) return fd;
    fd.packet_len = (uint16_t)g.packet_len;
    fd.prev_end = (uint16_t)(pv.has_prev ? pv.prev_end : 0);
    fd.left_start = (uint16_t)g.left_start;  // emission starts at the new _prevPacketStart
    fd.out_count = (uint16_t)g.out_count;
    fd.spec_off = pk.residue_offset;  // replaced by the temp offset when the coupling pass runs
    return fd;
}

// What both passes start from
void begin_pass(SynthPlan &P)
{
    Decoder &D = P.D;
    D.plan.s_base.assign((size_t)D.n_streams + 1, 0);
    D.plan.s_cnt.assign((size_t)D.n_streams, 0);
    D.plan.out_count.assign((size_t)D.n_streams, 0);
    P.st = D.states;
    P.started_with_prev.resize(D.n_streams);
    P.started_prev_long.resize(D.n_streams);
    for (int s = 0; s < D.n_streams; ++s) {
        P.started_with_prev[s] = P.st[s].has_prev;
        P.started_prev_long[s] = P.st[s].prev_long;
    }
    P.facts = BatchFacts();
    P.facts.need_coupling = D.generic;  // the generic path always works on its own planar copy
}
// ... and end with
int end_pass(SynthPlan &P, int64_t *samples_written)
{
    Decoder &D = P.D;
    for (int s = 0; s < D.n_streams; ++s)
        if (D.plan.out_count[s] > P.capacity_of(s))
            return set_error(D.ctx, VPZ_E_CAPACITY, "vpz_decoder_synth: stream_out_capacity too small");
    for (int s = 0; s < D.n_streams; ++s) samples_written[s] = D.plan.out_count[s];
    if (P.facts.any_floor0) P.facts.need_coupling = true;  // type-0 floors are applied in place on the planar temp
    return VPZ_OK;
}

// ---- pass 1 for large batches ------------------------------------------------------------------------------------------------

struct Chunk {
    int64_t lo = 0, hi = 0;
    bool ok = true;
    int64_t lead_sum = 0;     // samples of the packets that continue the previous chunk's last stream
    int64_t lead_end = 0;     // first packet that does not
    int64_t lead_anchor = kNone;  // first packet with a granule position among them
    int64_t tail_sum = 0;     // samples of the chunk's last stream segment
    int64_t base = 0;         // filled between the sweeps: samples of the leading stream before this chunk
    BatchFacts facts;
    bool dense = true;        // every packet's residue starts where its predecessor's (same stream) ends
    char pad[64];
};

inline bool is_last_of_stream(const SynthPlan &P, int64_t p)
{
    return p + 1 == P.n_packets || P.packets[p + 1].stream != P.packets[p].stream;
}

// sweep A: validation, samples per packet (before any EOS trim), chunk-local sums
void sweep_a(SynthPlan &P, Chunk &K)
{
    Decoder &D = P.D;
    const vpz_packet *packets = P.packets;
    int32_t *psamples = D.packet_samples.data();
    int64_t run = 0;
    bool leading = true;
    K.lead_end = K.lo;
    for (int64_t p = K.lo; p < K.hi; ++p) {
        const vpz_packet &pk = packets[p];
        if (pk.stream < 0 || pk.stream >= D.n_streams || (pk.flags & (VPZ_PKT_NOT_DECODED | VPZ_PKT_RESYNC)) ||
            pk.residue_offset < 0 || (p > 0 && packets[p - 1].stream > pk.stream)) {
            K.ok = false;
            return;
        }
        const bool no_floor = pk.flags & VPZ_PKT_NO_FLOOR;
        if (!no_floor && (pk.mapping >= D.mappings.size() || !P.have_posts)) { K.ok = false; return; }
        const bool last = is_last_of_stream(P, p);
        if ((pk.flags & VPZ_PKT_EOS) && !last) { K.ok = false; return; }
        const bool new_stream = p == 0 || packets[p - 1].stream != pk.stream;
        if (new_stream) {
            if (D.states[pk.stream].eos_found) { K.ok = false; return; }  // Read() ignores the stream from here on
            if (leading) { K.lead_sum = run; K.lead_end = p; leading = false; }
            run = 0;
        }
        const PacketInfo &pi = D.packet_info[pk.flags & 7];
        const FrameGeom g = frame_geometry(D, pi, prev_of(D, packets, p), pi.right_start);
        if (g.mismatch && !last) { K.ok = false; return; }
        psamples[p] = g.out_count;
        run += g.out_count;
        if (pk.granule != -1 && !g.mismatch) {
            if (leading) { if (K.lead_anchor == kNone) K.lead_anchor = p; }
            else if (D.plan.anchor_pkt[pk.stream] == kNone) D.plan.anchor_pkt[pk.stream] = p;
        }
        K.facts.note(D, pk);
        if (!new_stream) {
            const vpz_packet &pp = packets[p - 1];
            const int64_t prev_floats = (int64_t)D.channels * (((pp.flags & VPZ_PKT_BLOCK_FLAG) ? D.size1 : D.size0) / 2);
            if (pk.residue_offset != pp.residue_offset + prev_floats) K.dense = false;
        }
    }
    if (leading) { K.lead_sum = run; K.lead_end = K.hi; }
    K.tail_sum = run;
}

// sweep B: the descriptors, the per-record floor info, where each stream's packets begin and end
void sweep_b(SynthPlan &P, const Chunk &K)
{
    Decoder &D = P.D;
    const vpz_packet *packets = P.packets;
    const int C = D.channels;
    const bool group_bits = D.group_ok || D.dual_ok;  // (frame_flags' rule: these bits only when the decoder can use them)
    int64_t run = K.base;
    for (int64_t p = K.lo; p < K.hi; ++p) {
        const vpz_packet &pk = packets[p];
        const bool new_stream = p == 0 || packets[p - 1].stream != pk.stream;
        if (new_stream) { run = 0; D.plan.s_base[pk.stream] = p; }
        const PacketInfo &pi = D.packet_info[pk.flags & 7];
        const Prev pv = prev_of(D, packets, p);
        const FrameGeom g = frame_geometry(D, pi, pv, pi.right_start);  // (sweep A let a mismatch pass in a stream's last packet only)
        if (P.compact) {
            uint8_t cf = (uint8_t)(pk.flags & 7);
            if (pk.flags & VPZ_PKT_NO_FLOOR) cf |= kCfNoFloor;
            if ((pk.flags & VPZ_PKT_INTERLEAVED) && group_bits) cf |= kCfInterleaved;
            if (g.mismatch) cf |= kCfSkip;  // window mismatch: a frame that does nothing
            P.cflags[p] = cf;
            P.cmap[p] = pk.mapping;
            D.plan.out_off_scratch[(size_t)p] = run;
        } else {
            P.frames[p] = frame_desc(D, pk, p, pi, pv, g, run);
        }
        run += g.out_count;
        if (P.rec_floor) fill_rec_floor(D, pk, P.rec_floor + (size_t)(p * C));
        if (is_last_of_stream(P, p)) {
            D.plan.out_count[pk.stream] = run;
            D.plan.s_cnt[pk.stream] = p + 1;  // END of the stream's packets; becomes a count below (the stream's first
                                              // packet may belong to another chunk: no read of s_base here)
        }
    }
}

// once per stream: its state after the batch (ReadNextPacket :640-694 for the last packet), the position
// (:459-463, :493) and the EOS trim (:658-666)
void finish_stream(SynthPlan &P, int s)
{
    Decoder &D = P.D;
    PlanScratch &W = D.plan;
    const vpz_packet *packets = P.packets;
    int32_t *psamples = D.packet_samples.data();
    const int64_t L = W.s_cnt[s] - 1;
    W.s_cnt[s] -= W.s_base[s];
    const vpz_packet &pk = packets[L];
    StreamState &S = P.st[s];
    const PacketInfo &pi = D.packet_info[pk.flags & 7];
    if (pk.flags & VPZ_PKT_EOS) S.eos_found = true;
    const Prev pv = prev_of(D, packets, L);
    auto out_off_of = [&](int64_t q) { return P.compact ? W.out_off_scratch[(size_t)q] : P.frames[q].out_off; };
    // position in front of the stream's first packet: its own, or re-based where a granule was picked up
    int64_t pos_base = S.current_position;
    bool has_pos = S.has_position;
    const int64_t anchor = W.anchor_pkt[s];
    if (anchor != kNone && anchor < L && !has_pos) {
        pick_up_position(packets[anchor], psamples[anchor], has_pos, pos_base);
        pos_base -= out_off_of(anchor);
    }
    const int right_start = trimmed_right_start(pi, pk, pv, pos_base + out_off_of(L));
    const FrameGeom g = frame_geometry(D, pi, pv, right_start);
    if (g.mismatch) {
        D.mismatch_packets.push_back(L);
        // the state is the one the packet before it left
        if (W.s_cnt[s] > 1) leave_state(S, pv.prev_long, pv.prev_end, pv.prev_stop);
    } else {
        if (right_start != pi.right_start) {  // trimmed: the last frame, the stream's total
            W.out_count[s] += g.out_count - psamples[L];
            psamples[L] = g.out_count;
            W.trim_out_count[s] = g.out_count;
            W.trim_left_start[s] = g.left_start;
            if (!P.compact) {
                P.frames[L].out_count = (uint16_t)g.out_count;
                P.frames[L].left_start = (uint16_t)g.left_start;
            }
        }
        if (!has_pos) {  // :459-463 at the last packet itself
            pick_up_position(pk, right_start - g.left_start, has_pos, pos_base);
            if (has_pos) pos_base -= out_off_of(L);
        }
        leave_state(S, pk.flags & VPZ_PKT_BLOCK_FLAG, right_start, pi.right_end);
    }
    S.has_position = has_pos;
    S.current_position = pos_base + W.out_count[s];
}

// Pass 1 for large batches, split over the host cores.  It takes the batches real hosts produce: packets sorted by
// stream, all decoded, no resync, and the only packet of a stream that may carry an EOS flag or fail the window
// check (StreamDecoder.cs:777-778) is the stream's LAST one in the batch.  Then a packet's frame depends only on
// its own flags and on the packet before it (its window geometry); output offsets are a prefix sum -- chunk-local
// sums first, the chunks' bases serially, the descriptors in a second sweep -- and everything that needs the
// stream position (granule pick-up :459-463, EOS trim :658-666) is settled once per stream afterwards.  Any other
// batch returns 0 and the serial state machine below runs instead, so the rare paths of ReadNextPacket live in one
// place.  Returns 1: done, 0: not applicable, < 0: error.
int run_state_machine_parallel(SynthPlan &P, int64_t *samples_written)
{
    Decoder &D = P.D;
    PlanScratch &W = D.plan;
    const int64_t n_packets = P.n_packets;
    if (n_packets < D.par_min_packets || P.parties < 2 || !P.pool) return 0;
    const int parties = P.parties;
    std::vector<Chunk> chunks((size_t)parties);
    const int64_t per = (n_packets + parties - 1) / parties;
    for (int c = 0; c < parties; ++c) {
        chunks[c].lo = std::min<int64_t>(n_packets, per * c);
        chunks[c].hi = std::min<int64_t>(n_packets, per * (c + 1));
    }
    begin_pass(P);
    W.anchor_pkt.assign((size_t)D.n_streams, kNone);  // per stream: first packet that carries a granule position
    if (!P.pool->run([&](int c) { sweep_a(P, chunks[c]); }))
        return set_error(D.ctx, VPZ_E_NOMEM, "vpz_decoder_synth: host pass failed (allocation)");
    bool all_dense = true;
    for (const Chunk &K : chunks) {
        if (!K.ok) {  // the serial pass expects the per-packet counts zeroed
            std::fill(D.packet_samples.begin(), D.packet_samples.end(), 0);
            return 0;
        }
        all_dense &= K.dense;
        P.facts.merge(K.facts);
    }
    // Compact runs (two bytes per frame, descriptors built on the device) need consecutive packets with back to
    // back residues and a batch the fused kernel takes as it is (no planar temp, no type-0 floor pass)
    P.compact = all_dense && !D.generic && !D.big && (!P.facts.any_floor0 || (D.f0_fused && P.dual_usable())) && !D.no_compact &&
                (!P.facts.need_coupling || P.group_usable() || P.dual_usable());
    if (P.compact) {
        P.cflags = arena_alloc<uint8_t>(*P.A, (size_t)n_packets);
        P.cmap = arena_alloc<uint8_t>(*P.A, (size_t)n_packets);
        W.out_off_scratch.resize((size_t)n_packets);
    } else {
        P.frames = arena_alloc<FrameDesc>(*P.A, (size_t)n_packets);
    }
    P.rec_floor = P.have_posts ? arena_alloc<uint8_t>(*P.A, (size_t)(n_packets * D.channels)) : nullptr;
    W.trim_out_count.assign((size_t)D.n_streams, -1);
    W.trim_left_start.assign((size_t)D.n_streams, 0);
    // bases of the chunks' leading segments; a leading segment's first granule packet belongs to the stream
    // unless an earlier chunk already found one
    int32_t cur_stream = -1;
    int64_t cur_sum = 0;
    for (Chunk &K : chunks) {
        if (K.lo >= K.hi) continue;
        const int32_t first = P.packets[K.lo].stream, last = P.packets[K.hi - 1].stream;
        K.base = first == cur_stream ? cur_sum : 0;
        if (K.lead_anchor != kNone && W.anchor_pkt[first] > K.lead_anchor) W.anchor_pkt[first] = K.lead_anchor;
        if (K.lead_end == K.hi) cur_sum = K.base + K.lead_sum;  // one stream all through
        else cur_sum = K.tail_sum;
        cur_stream = last;
    }
    if (!P.pool->run([&](int c) { sweep_b(P, chunks[c]); }))
        return set_error(D.ctx, VPZ_E_NOMEM, "vpz_decoder_synth: host pass failed (allocation)");
    for (int s = 0; s < D.n_streams; ++s)
        if (W.s_cnt[s] != 0) finish_stream(P, s);
    P.n_frames = (size_t)n_packets;
    const int rc = end_pass(P, samples_written);
    return rc == VPZ_OK ? 1 : rc;
}

// Pass 1: StreamDecoder.Read / ReadNextPacket per stream (StreamDecoder.cs:418-498, 640-694) -> one
// FrameDesc per packet that produces or carries samples, written in place, stream-major.
int run_state_machine(SynthPlan &P, int64_t *samples_written)
{
    Decoder &D = P.D;
    const int64_t n_packets = P.n_packets;
    const vpz_packet *packets = P.packets;
    const int C = D.channels;
    begin_pass(P);
    std::vector<int64_t> &s_base = D.plan.s_base, &s_cnt = D.plan.s_cnt, &out_count = D.plan.out_count;
    if (D.n_streams > 1) {
        for (int64_t p = 0; p < n_packets; ++p) {
            const int32_t s = packets[p].stream;
            if (s < 0 || s >= D.n_streams)
                return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: packet stream index out of range");
            ++s_base[(size_t)s + 1];
        }
        for (int s = 0; s < D.n_streams; ++s) s_base[(size_t)s + 1] += s_base[(size_t)s];
    }
    FrameDesc *frames = P.frames = arena_alloc<FrameDesc>(*P.A, (size_t)n_packets);
    P.rec_floor = P.have_posts ? arena_alloc<uint8_t>(*P.A, (size_t)(n_packets * C)) : nullptr;
    if (P.rec_floor) memset(P.rec_floor, 0, (size_t)(n_packets * C));

    for (int64_t p = 0; p < n_packets; ++p) {
        const vpz_packet &pk = packets[p];
        if (pk.stream < 0 || pk.stream >= D.n_streams)
            return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: packet stream index out of range");
        StreamState &S = P.st[pk.stream];
        // Read(): once EOS was seen and the previous packet is drained nothing more is read (:441-447)
        if (S.eos_found && S.prev_start == S.prev_end) continue;
        // DecodeNextPacket :718-722, before the packet's first bit is looked at
        if (pk.flags & VPZ_PKT_RESYNC) S.has_position = false;
        const bool eos = pk.flags & VPZ_PKT_EOS;
        if (eos) S.eos_found = true;  // _eosFound |= isEndOfStream (:647), before the null check
        if (pk.flags & VPZ_PKT_NOT_DECODED) {
            if (eos && S.has_prev && S.prev_stop > S.prev_end) {  // :451-455 drain, un-windowed
                FrameDesc fd{};
                fd.flags = kFrameDrain;
                fd.prev_end = (uint16_t)S.prev_end;
                fd.out_count = (uint16_t)(S.prev_stop - S.prev_end);
                fd.out_off = out_count[pk.stream];
                out_count[pk.stream] += fd.out_count;
                D.packet_samples[(size_t)p] = fd.out_count;
                S.current_position += fd.out_count;
                S.prev_end = S.prev_stop;
                S.prev_start = S.prev_stop;
                frames[s_base[pk.stream] + s_cnt[pk.stream]++] = fd;
            }
            continue;
        }
        if (!(pk.flags & VPZ_PKT_NO_FLOOR)) {
            if (pk.mapping >= D.mappings.size())
                return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: packet mapping index out of range");
            if (!P.have_posts)
                return set_error(D.ctx, VPZ_E_INVALID_ARG,
                                 "vpz_decoder_synth: posts and a floor table are required unless VPZ_PKT_NO_FLOOR");
        }
        if (pk.residue_offset < 0)
            return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: negative residue offset");

        const PacketInfo &pi = D.packet_info[pk.flags & 7];  // Mode.GetPacketInfo, tabulated at create
        const Prev pv = prev_of_state(S);
        const int right_start = trimmed_right_start(pi, pk, pv, S.current_position);
        const FrameGeom g = frame_geometry(D, pi, pv, right_start);
        if (g.mismatch) {
            D.mismatch_packets.push_back(p);
            continue;
        }
        leave_state(S, pk.flags & VPZ_PKT_BLOCK_FLAG, right_start, pi.right_end);
        pick_up_position(pk, right_start - g.left_start, S.has_position, S.current_position);  // (idx == 0 here)
        frames[s_base[pk.stream] + s_cnt[pk.stream]++] = frame_desc(D, pk, p, pi, pv, g, out_count[pk.stream]);
        out_count[pk.stream] += g.out_count;
        D.packet_samples[(size_t)p] = g.out_count;
        S.current_position += g.out_count;
        P.facts.note(D, pk);
        if (P.rec_floor) fill_rec_floor(D, pk, P.rec_floor + (size_t)(p * C));
    }
    // close the gaps skipped packets left between the streams' frame ranges
    for (int s = 0; s < D.n_streams; ++s) {
        if (s_cnt[s] && (size_t)s_base[s] != P.n_frames)
            memmove(frames + P.n_frames, frames + s_base[s], sizeof(FrameDesc) * (size_t)s_cnt[s]);
        s_base[s] = (int64_t)P.n_frames;
        P.n_frames += (size_t)s_cnt[s];
    }
    return end_pass(P, samples_written);
}

// ---- pass 2: the frames cut into runs ----------------------------------------------------------------------------------------

using CutSeg = PlanScratch::CutSeg;

// What one cut is made with; every step below reads the values of the steps before it and fills in its own
struct Cut {
    int r_max = 0;
    bool batches = false;   // short blocks ride in batches: the runs are cut to equal COST
    int parties = 1;        // threads that walk the segments
    int w_short = 8, w_member = 8;  // cost of a short block alone / riding along, in eighths of a pass
    bool reuse = false;     // R and the cost target of the decoder's last call are taken over
    int64_t total_units = 0;
    int R = 0;
    int64_t run_slots = 0;  // runs that fit the rounds R was chosen for
    bool single_round = false;  // every run has a resident wave slot of its own from the start of the launch
    int min_run_frames = 1;
    int64_t target_units = 0;
    int64_t heavy_work = -1;
    bool skew_frames = false;
    int64_t heavy_frames = 0;
};

inline void seg_range(const SynthPlan &P, const Cut &c, int party, int &lo, int &hi)
{
    const int64_t n_segs = (int64_t)P.D.plan.cut_segs.size();
    lo = (int)(n_segs * party / c.parties);
    hi = (int)(n_segs * (party + 1) / c.parties);
}
// fn(party) on the pool, or on this thread
template <typename F>
void on_parties(SynthPlan &P, const Cut &c, const F &fn)
{
    if (c.parties > 1) P.host_failed |= !P.pool->run(fn);
    else fn(0);
}
// ... and the sum of fn(segment) over all segments, every party its share of them
template <typename F>
int64_t sum_over_segments(SynthPlan &P, const Cut &c, const F &fn)
{
    std::vector<int64_t> part(c.parties, 0);
    on_parties(P, c, [&](int party) {
        int lo, hi;
        seg_range(P, c, party, lo, hi);
        int64_t mine = 0;
        for (int g = lo; g < hi; ++g) mine += fn(g);
        part[party] = mine;
    });
    int64_t total = 0;
    for (int64_t v : part) total += v;
    return total;
}

// what a thread cuts is a SEGMENT: a stream, or -- few streams, many packets -- a piece of one (runs do not cross
// segments; the first run of a piece inside a stream recomputes its predecessor like any run that is not a stream's first)
void cut_segments(SynthPlan &P, Cut &c)
{
    Decoder &D = P.D;
    const int64_t total_frames = (int64_t)P.n_frames;
    c.r_max = P.use_dual ? kMaxRunLengthDual : D.big ? kMaxRunLengthBig : (P.needs_general ? kMaxRunLengthGeneral : kMaxRunLength);
    // Group mode synthesises up to eight consecutive SHORT blocks of a run in one pass (synth_kernel's run builder):
    // a block that rides along costs a fraction of a pass.  Runs are cut to equal COST, in eighths of a pass -- a
    // run rich in short blocks holds more frames --, so that every wavefront of the launch has the same amount to do.
    // (cutting by cost walks every packet a few times: with enough streams it is split over the host pool, streams
    // being independent; a small batch is walked on this thread; a large batch of few streams keeps runs of equal
    // length -- the kernel still batches what it finds in them -- rather than spend a millisecond of host time)
    HostPool *pool = P.pool;
    const bool wide = pool && D.n_streams >= 2 * pool->parties();
    // (... or, with short blocks to batch, is walked in pieces: 65 536 frames of ONE stream cut by cost are a millisecond on one
    // thread and 40 us on sixteen once the cut hint applies -- and worth 12 % of the kernel's time, configs[2])
    const bool split = pool && !wide && pool->parties() > 1 && total_frames > 4096;
    c.batches = P.compact && !P.facts.any_floor0 && (P.use_dual || (P.use_group && P.facts.any_floor)) && P.facts.any_short &&
                !P.needs_general && D.size0 == 256 && D.size1 != 256 && !D.generic &&
                (wide || total_frames <= 4096 || split) && !(D.ablate & 128);
    c.parties = (c.batches && (wide || split)) ? pool->parties() : 1;
    // cost of a pass in eighths of a long block's (group mode, measured: a short block alone 0.74, eight
    // in one batch 3.2 together; the stereo fast path, fitted to the waves' durations on real streams -- -DVPZ_WAVE_TIMES,
    // HISTORY.md: a short block alone or at the head of a batch costs a whole pass, 8.6 / 7.7 eighths, every block
    // riding along 2.0)
    c.w_short = P.use_dual ? 8 : 6;
    c.w_member = P.use_dual ? 2 : 3;
    std::vector<CutSeg> &segs = D.plan.cut_segs;
    segs.clear();
    for (int st_i = 0; st_i < D.n_streams; ++st_i) {
        const int64_t cnt = D.plan.s_cnt[st_i];
        int pieces = 1;
        if (c.batches && split) pieces = (int)std::max<int64_t>(1, std::min<int64_t>(cnt / 1024, (cnt * 4 * c.parties + total_frames - 1) / total_frames));
        for (int k = 0; k < pieces; ++k) {
            const int64_t a = cnt * k / pieces, b = cnt * (k + 1) / pieces;
            segs.push_back(CutSeg{st_i, (int32_t)a, (int32_t)(b - a)});
        }
    }
}

// The cost code of a segment's packets: what the later walks need to know about a packet, one byte each (bit 0: short block,
// bit 1: may ride in a batch, bit 2: same mapping as its predecessor) -- they then touch no packet.  Returns the segment's cost
// where the caller wants it counted (kCount).  (Only batches are coded.)
template <bool kCount>
inline int64_t code_segment(const SynthPlan &P, const Cut &c, const CutSeg &seg)
{
    const vpz_packet *packets = P.packets;
    uint8_t *code = P.D.plan.cut_code.data();
    const bool use_dual = P.use_dual;
    const int w_short = c.w_short, w_member = c.w_member;
    int pos = -1;
    bool prev_ok = false;
    int64_t units = 0;
    for (int64_t p = P.D.plan.s_base[seg.stream] + seg.off, e = p + seg.cnt; p < e; ++p) {
        // does packet p ride with its predecessor?
        bool ok = false, link = false;
        const vpz_packet &pk = packets[p];
        if (p > 0 && packets[p - 1].stream == pk.stream) {
            const vpz_packet &pp = packets[p - 1];
            // (the stereo fast path batches planar and already-floored packets too; a batch holds one kind)
            ok = !(pk.flags & VPZ_PKT_BLOCK_FLAG) && !(pk.flags & VPZ_PKT_NOT_DECODED) && !(pp.flags & VPZ_PKT_NOT_DECODED) &&
                 (use_dual || ((pk.flags & VPZ_PKT_INTERLEAVED) && !(pk.flags & VPZ_PKT_NO_FLOOR)));
            // (after a long block it can head a batch; it rides with a short predecessor of its mapping)
            link = kCount && ok && prev_ok && !(pp.flags & VPZ_PKT_BLOCK_FLAG) && pk.mapping == pp.mapping &&
                   ((pk.flags ^ pp.flags) & VPZ_PKT_NO_FLOOR) == 0;
        }
        code[(size_t)p] = (uint8_t)(((pk.flags & VPZ_PKT_BLOCK_FLAG) ? 0 : 1) | (ok ? 2 : 0) |
                                    ((ok && pk.mapping == packets[p - 1].mapping && !(packets[p - 1].flags & VPZ_PKT_BLOCK_FLAG)) ? 4 : 0));
        if (kCount) {
            pos = ok ? (link ? pos + 1 : 0) : -1;
            units += (ok && (pos & 7) != 0) ? w_member : ((pk.flags & VPZ_PKT_BLOCK_FLAG) ? 8 : w_short);
        }
        prev_ok = ok;
    }
    return units;
}

// the cost of every segment (D.plan.s_units) and of the batch, the packets' codes on the way
int64_t count_units(SynthPlan &P, const Cut &c)
{
    PlanScratch &W = P.D.plan;
    return sum_over_segments(P, c, [&](int g) { return W.s_units[(size_t)g] = code_segment<true>(P, c, W.cut_segs[(size_t)g]); });
}

// R (<= r_max) is the value for which the run count fills k whole rounds of the resident waves with the least total work
// k * (R + 1); short batches fall back to R = 4.
void choose_run_length(const SynthPlan &P, Cut &c)
{
    const Decoder &D = P.D;
    const int C = D.channels;
    const int64_t slots = std::max<int64_t>(1, P.resident_slots(P));
    c.run_slots = 0;
    const int64_t work = (c.total_units + 7) / 8 * C;
    c.R = 4;
    int64_t best = -1;
    // The stereo fast path chains the runs of a workgroup (chain_runs: three of four recompute nothing), and the memory
    // system delivers more the shorter the runs are -- the launch's waves then sweep the batch round by round instead of
    // streaming through all of it at once (tools/io_shapes.hip, profiles/r5_io_shapes.txt: 5.05 / 5.5 / 5.7 TB/s for runs of
    // 32 / 16 / 8 frames with the arithmetic removed): the rounds whose runs come closest to kDualChainRun frames.
    const int chain_run = D.dual_run;
    // (batches cut by COST -- streams with short blocks -- keep their long runs: measured, shorter ones lose there, configs[2]
    // 0.205 -> 0.226 ms and configs[4]'s share 0.258 -> 0.302 at 8 frames, profiles/r5_ab_chain_batches.txt; their runs are
    // chained all the same)
    const bool chained = P.use_dual && P.compact && D.size1 == 2048 && !D.no_chain && !c.batches;
    // (chained runs are cut by length: the grid is known exactly -- four runs to a workgroup, one workgroup per channel pair
    // of a chunk on the pair route -- and a run length whose grid is ONE workgroup over k rounds costs a round: 8 192 frames
    // of 10 channels in runs of 10 are 1 025 workgroups on 1 024 places)
    const int64_t resident_wgs = std::max<int64_t>(1, slots / (2 * P.dual_waves));
    auto grid_of = [&](int64_t r) -> int64_t {
        int64_t n = 0;
        for (int st_i = 0; st_i < D.n_streams; ++st_i) n += (D.plan.s_cnt[st_i] + r - 1) / r;
        return (n + P.dual_waves - 1) / P.dual_waves * (D.pairs ? C / 2 : 1);
    };
    for (int k = 1; k <= 64; ++k) {
        int64_t r = (work + k * slots - 1) / (k * slots);
        if (chained)
            while (r <= c.r_max && grid_of(r) > k * resident_wgs) ++r;
        if (r > c.r_max) continue;
        if (r < 4) break;
        // (chained: four runs share one recomputed block, and a run length below the preferred one only adds prologues)
        const int64_t cost = chained ? (r >= chain_run ? 4 * r + 1 : 1000 + (chain_run - r)) : (int64_t)k * (r + 1);
        if (best < 0 || cost < best) { best = cost; c.R = (int)r; c.run_slots = k * slots / C; c.single_round = k == 1; }
    }
}

// one run of a frame: as many frames from f0 on as the cost target (and the descriptor area) allow
inline int run_length(const Cut &c, const uint8_t *code, int f0, int cnt, int64_t target, int64_t &units)
{
    int len = 0;
    units = 0;
    int pos = -1;
    bool prev_ok = false;
    const uint8_t *cd = code + f0;
    while (f0 + len < cnt && len < c.r_max) {
        const uint8_t c8 = cd[len];
        const bool ok = c8 & 2;
        const bool link = ok && prev_ok && (c8 & 4);
        pos = ok ? (link ? pos + 1 : 0) : -1;
        const int u = (ok && (pos & 7) != 0) ? c.w_member : ((c8 & 1) ? c.w_short : 8);
        if (len > 0 && units + u > target) break;
        units += u;
        prev_ok = ok;
        ++len;
    }
    return len;
}
// the target of the run of segment `g` that starts `before` cost units into its segment
inline int64_t target_at(const SynthPlan &P, const Cut &c, int g, int64_t before, int64_t target)
{
    if (c.heavy_work < 0) return target;
    const int64_t sk = target * kCutSkewPermille / 1000;
    return P.D.plan.cut_prefix[(size_t)g] + before < c.heavy_work ? target + sk : target - sk;
}

// runs of equal cost do not pack as evenly as runs of equal length (and every stream ends with a partial
// one): a few more runs than the rounds hold would put a nearly empty round behind them -- count, and give
// every run a little more until they fit
int64_t runs_with(SynthPlan &P, const Cut &c, int64_t target)
{
    const PlanScratch &W = P.D.plan;
    const int64_t n_total = sum_over_segments(P, c, [&](int g) {
        int64_t n = 0, before = 0, u = 0;
        const uint8_t *code = W.cut_code.data() + W.s_base[W.cut_segs[g].stream] + W.cut_segs[g].off;
        for (int f0 = 0, cnt = W.cut_segs[g].cnt; f0 < cnt; ++n, before += u)
            f0 += run_length(c, code, f0, cnt, target_at(P, c, g, before, target), u);
        return n;
    });
    if (getenv("VPZ_HOST_PROFILE"))
        fprintf(stderr, "[vpz host] run cutting: R %d, target %lld eighths, %lld runs for %lld slots\n", c.R,
                (long long)target, (long long)n_total, (long long)c.run_slots);
    return n_total;
}

// The cost target of a run, and which runs are cut heavier than the others
void fit_target(SynthPlan &P, Cut &c)
{
    PlanScratch &W = P.D.plan;
    const int n_segs = (int)W.cut_segs.size();
    const int64_t total_frames = (int64_t)P.n_frames;
    c.target_units = c.reuse ? W.cut_hint_target : 8 * (int64_t)c.R;
    // THE SKEW.  With one round of runs, the first half of the grid's workgroups are the first to arrive on their CUs and
    // the second half join them as each CU's second workgroup -- and the waves of the second arrivals run slower for the
    // whole launch (measured per wave, -DVPZ_WAVE_TIMES: identical runs take 600 k cycles in wave slot 0 of their SIMD,
    // 647 k in slot 1; priorities set with s_setprio do not change it), so with equal work the early half idles at the end
    // while the late half finishes at half occupancy.  Runs that start in the first half of the batch's WORK -- they are
    // the first half of the grid -- are therefore cut 2 % heavier, the others as much lighter (HISTORY.md:
    // configs[4] 0.283 -> 0.278 ms at 20 per mille, worse again from 40 on).
    c.heavy_work = c.reuse ? W.cut_hint_heavy : -1;
    if (c.batches && !c.reuse && c.single_round && P.use_dual && c.R >= 16) {  // (short runs: nothing to skew by)
        c.heavy_work = c.total_units * (1000 + kCutSkewPermille) / 2000;
        W.cut_prefix.resize((size_t)n_segs);
        int64_t acc = 0;
        for (int st_i = 0; st_i < n_segs; ++st_i) {
            W.cut_prefix[(size_t)st_i] = acc;
            acc += W.s_units[(size_t)st_i];
        }
    }
    if (c.heavy_work >= 0 && W.cut_prefix.size() != (size_t)n_segs) c.heavy_work = -1;
    // (all-long batches only: with short blocks in runs of equal length a frame more is not 3 % more -- configs[2] lost 2 %)
    // (group mode -- 6 channels, two workgroups of 8 waves per CU -- does not respond to it: configs[3] 0.323 either way)
    c.skew_frames = !c.batches && !P.facts.any_short && c.single_round && P.use_dual && c.R >= 24 && c.R + 1 <= c.r_max;
    c.heavy_frames = total_frames * (c.R + 1) / (2 * (int64_t)c.R);  // the first half of the frames' work at R + 1 each
    if (!(c.batches && c.run_slots > 0 && !c.reuse)) return;
    // in steps of half a pass until the runs fit, then back in eighths: the lightest runs that still fit (a launch
    // takes as long as its heaviest run; half a pass is 2 % of one)
    bool fits = false;
    for (int tries = 0; tries < 6 && c.target_units / 8 < c.r_max; ++tries) {
        if ((fits = runs_with(P, c, c.target_units) <= c.run_slots)) break;
        c.target_units += 4;
    }
    if (fits && c.target_units > 8 * (int64_t)c.R) {
        for (int64_t t = c.target_units - 3; t < c.target_units; ++t)
            if (runs_with(P, c, t) <= c.run_slots) { c.target_units = t; break; }
    }
    W.cut_hint_R = c.R;
    W.cut_hint_slots = c.run_slots;
    W.cut_hint_target = c.target_units;
    W.cut_hint_heavy = c.heavy_work;
    W.cut_hint_frames = total_frames;
    W.cut_hint_streams = P.D.n_streams;
}

// a compact run whose first staged frame is packet q: where its records and residue start, the window in front of it
__attribute__((always_inline)) inline void stage_from(const SynthPlan &P, RunDesc &r, int64_t q)
{
    r.rec_base = (int32_t)(q * P.D.channels);
    r.spec_base = P.packets[q].residue_offset;
    const Prev pv = prev_of(P.D, P.packets, q);
    r.has_prev0 = pv.has_prev ? 1 : 0;
    r.prev_end0 = (uint16_t)pv.prev_end;
    r.prev_stop0 = (uint16_t)pv.prev_stop;
}

// the run of segment `seg` that starts f0 frames into the segment and holds len frames
inline RunDesc make_run(const SynthPlan &P, const CutSeg &seg, int f0, int len)
{
    const Decoder &D = P.D;
    const int s = seg.stream;
    RunDesc r{};
    r.first = (int)D.plan.s_base[s] + seg.off + f0;
    r.count = len;
    r.stream = s;
    if (seg.off + f0 == 0) {
        r.pre_kind = P.started_with_prev[s] ? kPreState : kPreNone;
        r.prev_long = P.started_prev_long[s];
    } else {
        r.pre_kind = kPreRecompute;
    }
    const bool last = seg.off + f0 + len >= (int)D.plan.s_cnt[s];
    if (last) r.flags |= kRunSaveState;
    r.clip_epoch = D.states[s].clip_epoch;
    r.state_slot = D.states[s].state_slot;
    if (P.compact) {
        r.flags |= kRunCompact;
        stage_from(P, r, (int64_t)r.first + (r.pre_kind == kPreRecompute ? -1 : 0));  // first staged frame
        r.out_base = D.plan.out_off_scratch[(size_t)r.first];
        if (last && D.plan.trim_out_count[s] >= 0) {  // the stream's last frame was cut by the EOS trim
            r.flags |= kRunLastTrimmed;
            r.last_out_count = (uint16_t)D.plan.trim_out_count[s];
            r.last_left_start = (uint16_t)D.plan.trim_left_start[s];
        }
    }
    return r;
}

// Runs of equal LENGTH: the k-th run of a segment is its frames [k R, (k + 1) R) -- every run's place is known in advance,
// so a large batch is filled in by the host pool, every thread its share of the run indices (thousands of runs of 8 frames
// were 85 us on one thread: as long as the kernel takes for a third of them)
void write_runs_by_length_wide(SynthPlan &P, const Cut &c)
{
    const std::vector<CutSeg> &segs = P.D.plan.cut_segs;
    const int n_segs = (int)segs.size(), R = c.R;
    std::vector<int64_t> &seg_first = P.D.plan.cut_prefix;
    seg_first.assign((size_t)n_segs + 1, 0);
    for (int g = 0; g < n_segs; ++g) seg_first[(size_t)g + 1] = seg_first[(size_t)g] + (segs[g].cnt + R - 1) / R;
    const int64_t total_runs = seg_first[(size_t)n_segs];
    if ((size_t)total_runs > P.runs_cap) { P.host_failed = true; return; }
    const int n_threads = P.fill_threads = P.pool->parties();
    P.host_failed |= !P.pool->run([&](int party) {
        const int64_t lo = total_runs * party / n_threads, hi = total_runs * (party + 1) / n_threads;
        int g = (int)(std::upper_bound(seg_first.begin(), seg_first.end(), lo) - seg_first.begin()) - 1;
        for (int64_t i = lo; i < hi; ++i) {
            while (i >= seg_first[(size_t)g + 1]) ++g;
            const int f0 = (int)(i - seg_first[(size_t)g]) * R;
            P.runs[i] = make_run(P, segs[g], f0, std::min(R, segs[g].cnt - f0));
        }
    });
    P.n_runs = (size_t)total_runs;
}

// ... or segment by segment, by cost or by length: every thread its share of the segments
void write_runs_per_segment(SynthPlan &P, const Cut &c)
{
    const PlanScratch &W = P.D.plan;
    const std::vector<CutSeg> &segs = W.cut_segs;
    P.fill_threads = c.parties;
    std::vector<std::vector<RunDesc>> cut(c.parties);
    on_parties(P, c, [&](int party) {
        int s_lo, s_hi;
        seg_range(P, c, party, s_lo, s_hi);
        std::vector<RunDesc> &mine = cut[party];
        if (c.parties > 1) {
            // (a stream without packets in this call keeps s_base = s_cnt = 0: count the range's packets, never
            // subtract bases)
            int64_t pk_in_range = 0;
            for (int g = s_lo; g < s_hi; ++g) pk_in_range += segs[g].cnt;
            mine.reserve((size_t)(pk_in_range / c.min_run_frames) + (size_t)(s_hi - s_lo) + 1);
        }
        for (int g = s_lo; g < s_hi; ++g) {
            const int cnt = segs[g].cnt, base = (int)W.s_base[segs[g].stream] + segs[g].off;  // (f0 below counts from the segment's start)
            if (c.reuse) (void)code_segment<false>(P, c, segs[g]);  // (the codes of this segment's packets, skipped with the counting pass)
            int64_t before = 0, run_units = 0;
            for (int f0 = 0; f0 < cnt; before += run_units) {
                // (runs of equal LENGTH: the skew is a frame more in the first half of the frames, a frame less in the second)
                const int len = c.batches ? run_length(c, W.cut_code.data() + base, f0, cnt, target_at(P, c, g, before, c.target_units), run_units)
                                          : std::min(c.R + (c.skew_frames ? ((int64_t)base + f0 < c.heavy_frames ? 1 : -1) : 0), cnt - f0);
                const RunDesc r = make_run(P, segs[g], f0, len);
                if (c.parties > 1) mine.push_back(r);
                else if (P.n_runs < P.runs_cap) P.runs[P.n_runs++] = r;
                else { P.host_failed = true; return; }
                f0 += len;
            }
        }
    });
    if (c.parties == 1 || P.host_failed) return;
    for (const std::vector<RunDesc> &v : cut) {
        if (P.n_runs + v.size() > P.runs_cap) { P.host_failed = true; return; }  // (never silently into what follows)
        memcpy(P.runs + P.n_runs, v.data(), v.size() * sizeof(RunDesc));
        P.n_runs += v.size();
    }
}

// The stereo fast path: runs r - 1 and r of one stream that land in ONE workgroup (the kernel takes run i in wave i mod
// kDualWaves of workgroup i / kDualWaves) and meet in the steady state -- a 2048 block after a 2048 block, long windows on
// both sides -- are CHAINED: the later one recomputes nothing, it overlaps its first frame with the tail the earlier one
// leaves in LDS (kPreNeighbour, synth_desc.hpp).  With three runs of four chained, short runs cost a quarter of what their
// recomputed blocks did, and short runs are what the memory system likes (tools/io_shapes.hip: the waves of a launch then
// sweep a quarter or an eighth of the batch at a time instead of all of it).
void chain_runs(SynthPlan &P)
{
    const Decoder &D = P.D;
    const vpz_packet *packets = P.packets;
    RunDesc *runs = P.runs;
    const size_t n_runs = P.n_runs;
    P.n_chained = 0;
    if (!P.use_dual || !P.compact || D.size1 != 2048 || D.no_chain) return;
    const size_t waves = (size_t)P.dual_waves;
    // (a run looks at its predecessor's place and length only -- what the chaining never changes: any split of the runs works)
    auto chain_range = [&](size_t lo, size_t hi) -> int64_t {
        int64_t n = 0;
        for (size_t i = std::max<size_t>(lo, 1); i < hi; ++i) {
            RunDesc &r = runs[i];
            const RunDesc &pr = runs[i - 1];
            if (i % waves == 0 || r.pre_kind != kPreRecompute || r.stream != pr.stream || pr.count <= 0 ||
                r.first != pr.first + pr.count || !(r.flags & kRunCompact) || r.count <= 0)
                continue;
            const int64_t q = r.first;
            if (q <= 0 || packets[q - 1].stream != r.stream) continue;
            const uint8_t cf = P.cflags[q], pcf = P.cflags[q - 1];
            // frame q: long, long windows on both sides, taken; frame q - 1: long with a long window towards q, taken
            if ((cf & (7u | kCfSkip)) != 7u || (pcf & (1u | 4u | kCfSkip)) != 5u) continue;
            if (r.count == 1 && (r.flags & kRunLastTrimmed)) continue;  // (its only frame is the stream's EOS-trimmed last one)
            r.pre_kind = kPreNeighbour;
            stage_from(P, r, q);  // (in front of it: packet q - 1, checked above)
            ++n;
        }
        return n;
    };
    // the runs' flag bytes inline (SynthArgs.run_inline): one trip to the pinned arena per run instead of two
    // (only where runs are short enough to use them: the kernel takes the bytes of a run of up to 16 staged frames inline)
    const bool want_inline = P.cut_R > 0 && P.cut_R + 1 <= 16;
    P.run_inline = want_inline ? arena_alloc<uint8_t>(*P.A, 32 * n_runs + 32) : nullptr;
    auto inline_range = [&](size_t lo, size_t hi) {
        for (size_t i = lo; want_inline && i < hi; ++i) {
            const RunDesc &r = runs[i];
            uint8_t *dst = P.run_inline + 32 * i;
            memset(dst, 0, 32);
            if (!(r.flags & kRunCompact)) continue;
            const int64_t q = (int64_t)r.first + (r.pre_kind == kPreRecompute ? -1 : 0);
            const int n = std::min(16, r.count + (r.pre_kind == kPreRecompute ? 1 : 0));
            for (int j = 0; j < n; ++j) {
                dst[j] = P.cflags[q + j];
                dst[16 + j] = P.cmap[q + j];
            }
        }
    };
    // (one sweep does both: a run's bytes depend on its own record only, its chaining on its predecessor's place and length)
    P.chain_threads = 1;
    if (P.pool && P.pool->parties() > 1 && n_runs >= 1024) {  // (the pool's workers are still spinning from the cut's fork-join)
        const int n_threads = P.chain_threads = P.pool->parties();
        std::vector<int64_t> part((size_t)n_threads, 0);
        P.host_failed |= !P.pool->run([&](int party) {
            const size_t lo = n_runs * (size_t)party / n_threads, hi = n_runs * (size_t)(party + 1) / n_threads;
            part[(size_t)party] = chain_range(lo, hi);
            inline_range(lo, hi);
        });
        for (int64_t v : part) P.n_chained += v;
    } else {
        P.n_chained = chain_range(0, n_runs);
        inline_range(0, n_runs);
    }
}

// One more fact of the batch, beside the ones pass 1 gathers: every frame is the steady state of its stream, or its stream's
// first block after a reset -- what steady_stereo_kernel walks without descriptors (steady_stereo.hip).  The packets' flags are
// a fact of pass 1 (every packet long, long windows on both sides, already floored, planar); what is left is per stream: the
// block in front of the call's first packet, if there is one, is a long one with a long window towards it, no window check
// failed and no EOS trim cut the last packet.  The runs are the ones any batch of the stereo route gets.
bool all_steady(const SynthPlan &P, const Cut &c)
{
    const Decoder &D = P.D;
    if (!P.use_dual || D.pairs || !P.compact || c.batches || D.no_steady || D.channels != 2 || D.size0 != 256 || D.size1 != 2048) return false;
    if (!P.facts.all_steady_flags || P.facts.any_floor || P.facts.any_short || P.facts.ilv_seen || !D.mismatch_packets.empty()) return false;
    for (int s = 0; s < D.n_streams; ++s) {
        if (D.plan.s_cnt[s] <= 0) continue;
        const StreamState &S = D.states[s];  // (the state in front of the call: P.st is the one after it)
        if (S.has_prev && !(S.prev_long && S.prev_end == 1024 && S.prev_stop == 2048)) return false;
        if (D.plan.trim_out_count[s] >= 0) return false;
    }
    return true;
}

}  // namespace

// The stereo fast path takes a batch whose packets all have ONE input layout (its loads are unconditional: the
// layout is a template parameter) and start where its loads are aligned: 16 bytes for the Residue2 vector, 8 for planar.
bool SynthPlan::dual_usable() const
{
    if (!D.dual_ok || (facts.any_floor0 && !D.f0_fused) || (facts.ilv_seen && facts.planar_seen)) return false;
    // (int16 values are widened into the decoder's own, aligned staging buffer whatever the memory space)
    // (the pair route reads 8 bytes -- two adjacent channels of a bin, or two bins of a channel -- whatever the layout)
    const bool wide = facts.ilv_seen && !D.pairs;
    const bool dev_ok = mem_space == VPZ_MEM_HOST || D.residue_format == VPZ_RESIDUE_I16 || (residue_addr & (wide ? 15 : 7)) == 0;
    if (!(dev_ok && (wide ? facts.group_align_ok : facts.align2_ok))) return false;
    // Pairs or group mode, where both can take the call (measured on BASELINE configs[3], 6 channels, profiles/r5_ab_pairs.txt):
    // planar packets to planar PCM the pairs are 8 % faster; the Residue2 vector read by columns (a third of every line per
    // workgroup) ties with group mode's staging; interleaved PCM written by columns loses 20 % against the packet's waves writing
    // whole rows together.  VPZ_PAIRS=1 (tests, A/B): the pairs wherever they can.
    // Beyond eight channels (no group mode) the columns of the Residue2 vector cost what the separate coupling pass costs
    // (10 channels: 0.390 against 0.375 ms): the pairs take planar packets to planar PCM there too.
    if (D.pairs && !D.pairs_always && (facts.ilv_seen || out_interleaved)) return false;
    return true;
}
bool SynthPlan::group_usable() const
{
    return D.group_ok && facts.group_align_ok &&
           (mem_space == VPZ_MEM_HOST || D.residue_format == VPZ_RESIDUE_I16 || (residue_addr & 15) == 0);
}

int plan_frames(SynthPlan &P, int64_t *samples_written)
{
    int rc = run_state_machine_parallel(P, samples_written);
    if (rc < 0) return rc;
    P.was_parallel = rc == 1;
    if (rc == 0 && (rc = run_state_machine(P, samples_written)) != VPZ_OK) return rc;
    // group mode of the fused kernel (de-interleave and inverse coupling in LDS) when the batch needs either and
    // its packets can be read in 16-byte pieces; otherwise the separate pass through a planar temp
    // ... and for interleaved output of more than two channels, which only a packet's waves together can write densely
    const bool wants_group = P.facts.need_coupling || (P.out_interleaved && P.D.channels > 2);
    P.use_dual = P.dual_usable();
    P.use_group = !P.use_dual && P.D.group_ok && wants_group && !P.facts.any_floor0 && P.facts.group_align_ok &&
                  (P.mem_space == VPZ_MEM_HOST || (P.residue_addr & 15) == 0);
    return VPZ_OK;
}

// Pass 2: cut each stream's frames into runs.  A wavefront synthesises R consecutive blocks of one channel
// (+1 recomputed block in front): segments -> cost codes and units -> R and the run slots -> the cost target -> the run
// records -> the hint check -> the chaining.
void plan_runs(SynthPlan &P)
{
    Decoder &D = P.D;
    PlanScratch &W = D.plan;
    const int64_t total_frames = (int64_t)P.n_frames;
    Cut c;
    cut_segments(P, c);
    P.cut_by_cost = c.batches;
    const int n_segs = (int)W.cut_segs.size();
    const size_t runs_arena_mark = P.A->used;
    for (int attempt = 0; attempt < 2; ++attempt) {
        // (a retry -- the reused cut hint did not fit, see the end of this loop -- takes the first attempt's place
        // in the arena instead of a second allocation)
        P.A->used = runs_arena_mark;
        P.n_runs = 0;
        // a decoder's next batch usually has the shape of its last one: R and the fitted cost target are taken over, the
        // packets are walked ONCE (codes and cut together, one fork-join), and only if the runs do not fit the rounds
        // after all is the whole procedure gone through
        c.reuse = c.batches && c.parties > 1 && W.cut_hint_frames == total_frames && W.cut_hint_streams == D.n_streams &&
                  W.cut_hint_R > 0;
        if (c.batches && W.cut_code.size() < (size_t)total_frames) W.cut_code.resize((size_t)total_frames);
        if (c.batches) W.s_units.assign((size_t)n_segs, 0);
        c.total_units = (c.batches && !c.reuse) ? count_units(P, c) : 8 * total_frames;
        c.R = W.cut_hint_R;
        c.run_slots = W.cut_hint_slots;
        c.single_round = false;
        if (!c.reuse) choose_run_length(P, c);
        // (a run cut by cost holds at least R - 1 frames unless its stream ends: every frame costs at most a whole pass)
        // (... and the lighter half of a skewed cut holds that much less: see THE SKEW)
        c.min_run_frames = std::max(1, c.R - 1 - (c.R >= 16 ? c.R * kCutSkewPermille / 1000 + 2 : 0));
        // (every segment -- a stream, or a piece of a long one -- ends with a partial run)
        P.runs_cap = (size_t)(total_frames / c.min_run_frames) + (size_t)std::max(n_segs, D.n_streams) + 1;
        P.runs = arena_alloc<RunDesc>(*P.A, P.runs_cap);  // (throws ArenaOverflow -> VPZ_E_NOMEM: open_arena's budget is R >= 4 runs)
        if (D.generic) return;
        fit_target(P, c);
        if (!c.batches && !c.skew_frames && P.pool && P.pool->parties() > 1 && total_frames / std::max(1, c.R) >= 1024)
            write_runs_by_length_wide(P, c);
        else
            write_runs_per_segment(P, c);
        if (P.host_failed) { P.n_runs = 0; return; }
        // this batch is not like the last one after all: more runs than the rounds hold, or -- a lighter mix of blocks, so
        // fewer and longer runs -- so few that part of the resident waves would idle through the launch
        if (!(c.reuse && ((int64_t)P.n_runs > c.run_slots || (int64_t)P.n_runs * 10 < W.cut_hint_runs * 9))) break;
        W.cut_hint_frames = -1;
    }
    if (c.batches && !c.reuse) W.cut_hint_runs = (int64_t)P.n_runs;
    P.cut_R = c.R;
    chain_runs(P);
    P.steady = all_steady(P, c);
    if (getenv("VPZ_HOST_PROFILE"))
        fprintf(stderr, "[vpz host] cut: %s, by %s, R %d, target %lld eighths, %zu runs for %lld slots, %d segments on %d threads, heavy below %lld, "
                        "hint (frames %lld, runs %lld), chained %lld, runs filled by %s on %d threads, chain sweep on %d threads\n",
                c.reuse ? "hint reused" : "fitted", c.batches ? "cost" : "length", c.R,
                (long long)c.target_units, P.n_runs, (long long)c.run_slots, n_segs, c.parties, (long long)c.heavy_work,
                (long long)W.cut_hint_frames, (long long)W.cut_hint_runs, (long long)P.n_chained,
                P.fill_threads > 1 ? "the pool" : "the calling thread", P.fill_threads, P.chain_threads);
}

}  // namespace vpz
