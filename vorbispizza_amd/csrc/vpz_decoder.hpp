// The decoder object behind vpz_decoder_*: its setup, the streams' states and its buffers.  Shared by the decoder's lifecycle,
// staging and launches (vpz_decoder.hip) and the host plan of a synth call (synth_plan.hip).
#pragma once

#include <vector>

#include "vpz_internal.hpp"

namespace vpz {

// StreamDecoder.cs:45-49 + position / EOS bookkeeping, per stream
struct StreamState {
    bool has_prev = false;      // _prevPacketBuf != null
    bool prev_long = false;     // block flag of the packet held in _prevPacketBuf
    int prev_start = 0, prev_end = 0, prev_stop = 0;
    int64_t current_position = 0;
    bool has_position = true;   // ProcessHeaderPackets: _currentPosition = 0; _hasPosition = true (:165-168)
    bool eos_found = false;
    bool has_clipped = false;
    int32_t clip_epoch = 1;     // resets so far + 1: clipped[stream] == clip_epoch <=> HasClipped
    int32_t state_slot = 0;     // which of the two device copies of the saved overlap state is current: a batch reads it in
                                // the stream's first run and writes the other copy in its last one -- two wavefronts of
                                // one launch with no order between them (the last run of a stream rich in short blocks can
                                // be done before the first one has read)
};

using DevBuf = Scratch;  // the decoder's buffers grow by the context's rule (vpz_internal.hpp), none of them with a drain

// Pinned host arena for the per-call descriptor uploads: copies out of it are truly asynchronous,
// and the next call waits (on an event) only for the previous call's uploads before reusing it.
struct PinnedArena {
    char *base = nullptr;
    char *mapped = nullptr;   // the same memory as the GPU addresses it (hipHostGetDevicePointer)
    size_t cap = 0, used = 0;
    hipEvent_t uploaded = nullptr;   // the arena is in its device mirror
    bool pending = false;
    DevBuf dev;  // device mirror, same layout: one hipMemcpyAsync per call
};

// Carves `count` objects out of the call's arena.  open_arena sizes the arena for everything a call can ask for; should a
// request not fit after all, ArenaOverflow is thrown -- vpz_decoder_synth turns it into VPZ_E_NOMEM -- instead of a write
// beyond the allocation.
struct ArenaOverflow {};
template <typename T>
static T *arena_alloc(PinnedArena &A, size_t count)
{
    A.used = (A.used + 63) & ~(size_t)63;
    if (A.used > A.cap || sizeof(T) * count > A.cap - A.used) throw ArenaOverflow();
    T *p = reinterpret_cast<T *>(A.base + A.used);
    A.used += sizeof(T) * count;
    return p;
}

// Mode.cs:30-66
struct PacketInfo {
    int length, left_use_size1, left_start, left_end, right_start, right_end;
};

// What only the host plan of a synth call uses (synth_plan.hip): its per-call scratch, kept between calls for its capacity,
// and what one call's run cut leaves for the next (the cut hint).  s_cnt / out_count are read by the staging afterwards.
struct PlanScratch {
    std::vector<int64_t> s_base, s_cnt, out_count, anchor_pkt;  // per-stream scratch of a synth call
    std::vector<int64_t> out_off_scratch;    // compact batches: output offset of every frame (host only)
    std::vector<int32_t> trim_out_count, trim_left_start;  // per stream: EOS-trimmed last frame of the batch, -1: none
    std::vector<uint8_t> cut_code;           // plan_runs: one byte per packet (block size, batch eligibility)
    int cut_hint_R = 0;                      // ... and the cost target the last call's runs were fitted with
    int64_t cut_hint_slots = 0, cut_hint_target = 0, cut_hint_frames = -1, cut_hint_runs = 0;
    int cut_hint_streams = -1;
    int64_t cut_hint_heavy = -1;             // runs that start below this cost position get the heavier target (plan_runs: THE SKEW)
    struct CutSeg { int32_t stream, off, cnt; };  // packets [s_base[stream] + off, + cnt): what one thread cuts into runs
    std::vector<CutSeg> cut_segs;            // the streams of a call, long ones of a batch of few streams in pieces (plan_runs)
    std::vector<int64_t> s_units;            // cost of each segment's packets in this call (plan_runs), then
    std::vector<int64_t> cut_prefix;         // ... the cost of all segments in front of each one
};

struct Decoder {
    Context *ctx = nullptr;
    PinnedArena arenas[2];
    int arena_idx = 0;
    PlanScratch plan;
    int channels = 0, size0 = 0, size1 = 0, clip = 0;
    int n_streams = 0;
    std::vector<int64_t> stream_caps;  // vpz_decoder_set_stream_capacities: empty, or one bound per stream
    std::vector<vpz_floor1_config> floors;
    std::vector<vpz_mapping_config> mappings;
    std::vector<StreamState> states;
    BlockTables *t0 = nullptr, *t1 = nullptr;
    FloorDev *d_floors = nullptr;
    float *d_state_h = nullptr;
    int32_t *d_clipped = nullptr;
    uint8_t *d_steps = nullptr;              // coupling steps of all mappings, pairs (mag, ang)
    uint8_t *d_steps_lvl = nullptr;          // the same with bit 7 of `mag` set where a level of disjoint steps starts
    uint32_t *d_map_bits = nullptr;          // per mapping: group-mode frame flag bits (stage / steps) of a floored frame
    std::vector<uint8_t> mapping_uses_floor0;
    bool no_compact = false;                 // VPZ_NO_COMPACT=1: always upload explicit frame descriptors (A/B tests)
    std::vector<int32_t> mapping_steps_off;  // per mapping: offset into d_steps (pairs*2), -1 none
    std::vector<uint8_t> mapping_skip[2];    // per mapping and block size: point groups (of 8) beyond the residue's support (ABI v4)
    DevBuf b_curve, b_temp, b_cposts, b_ccount;
    // group mode of synth_kernel (channels of a packet share a workgroup; de-interleave + coupling in LDS)
    bool group_ok = false;       // channel count, step tables and floor types allow it
    // stereo fast path (synth_dual.hip: one wavefront per stream synthesises both channels, coupling in registers)
    bool dual_ok = false;        // two channels, 256 / 2048 blocks, type-1 floors only (VPZ_NO_DUAL=1: off, for A/B tests)
    // ... and its kernel for channel PAIRS (synth_pairs.hip): 4, 6, 8, ... channels that the coupling steps of all mappings join two
    // by two -- every pair is a stereo stream to the arithmetic (VPZ_NO_PAIRS=1: off, for A/B and bit-equality tests)
    bool pairs = false;          // (implies dual_ok)
    // group mode and the stereo kernel find a frame's steps in the decoder-wide table (count and first pair in the frame's flags);
    // the pair route has a table of its own (d_pair_steps) and may run where the decoder-wide one is too long for those bits
    bool wide_steps = false;
    bool pairs_always = false;   // VPZ_PAIRS=1: the pair route wherever it can run, also where group mode is as fast or faster
    uint8_t *d_pair_ch = nullptr;         // [pair][2]: the pair's channels, coupled ones first ("channel 0" of its steps), in channel order
    uint32_t *d_pair_map_bits = nullptr;  // [pair][mapping]: SynthArgs.map_bits of the pair route
    uint8_t *d_pair_steps = nullptr;      // the pairs' step lists: (0 | 1: which of the pair's channels is the magnitude, unused)
    int n_pair_step_pairs = 0;
    int max_steps = 0, n_step_pairs = 0;
    int host_threads = 0;        // parties of the parallel state machine (VPZ_HOST_THREADS; 0: pick)
    int64_t par_min_packets = 16384;  // batches below this take the serial state machine (VPZ_PAR_MIN_PACKETS)
    DevBuf b_in_res, b_in_posts, b_in_counts, b_out;  // VPZ_MEM_HOST staging
    DevBuf b_in_res16;              // VPZ_RESIDUE_I16: the int16 values as they came over the link, widened into b_in_res
    int residue_format = VPZ_RESIDUE_F32;
    DevBuf b_ybuf;                                    // any-block-size path
    DevBuf b_bigtail;                                 // synth_big_kernel, 8192 decoders: the waves' tails (SynthArgs.big_tail)
    bool generic = false;  // a block size the fused kernels do not take (64, 128): three-pass path (synth_kernels.hip)
    bool big = false;      // the long block is 4096 or 8192 samples: synth_big_kernel (synth_big.hip; VPZ_NO_BIG=1: the three-pass path)
    // type-0 floors (Floor0.cs)
    std::vector<uint8_t> floor_types;
    std::vector<vpz_floor0_config> floors0;
    void *d_floors0 = nullptr;
    int32_t *d_bark_maps = nullptr;
    // type-0 floors inside the stereo fast path (floor0_curve_kernel + floor0_multiply): possible when every type-0 floor's
    // bark map has at most kFloor0MaxBark entries; f0_k = the largest of them (row length of the per-record curves)
    bool f0_fused = false;
    bool has_floor1 = false;  // some floor of the setup is of type 1
    int f0_k = 0;
    uint16_t *d_f0_bark = nullptr;   // [floor][short / long][1024]: bark index of every bin in lane order (SynthArgs.f0_bark)
    float *d_f0_w = nullptr;         // [floor][f0_k]: 2 cos(pi k / bark_map_size), Floor0's wMap (floor0_wtab_kernel)
    DevBuf b_f0curve;
    DevBuf b_in_amp, b_in_coeff;
    const float *f0_amp = nullptr, *f0_coeff = nullptr;
    int32_t f0_stride = 0;
    PacketInfo packet_info[8];  // Mode.GetPacketInfo by (block | prev << 1 | next << 2) == vpz_packet.flags & 7
    int dual_run = 8;  // preferred run length of the stereo fast path's chained runs (VPZ_DUAL_RUN)
    int64_t plan_slots = 0;  // VPZ_PLAN_SLOTS=n (tests): the resident slots the run cut plans for, on every route; 0: the kernels' own
    bool no_direct_i16 = false;
    bool no_chain = false;  // VPZ_NO_CHAIN=1 (A/B tests): no run of the stereo fast path takes its predecessor's tail over in LDS
    bool no_steady = false;  // VPZ_NO_STEADY=1 (A/B and bit-equality tests): all-steady batches take synth_dual_kernel too (steady_stereo.hip)
    int ablate = 0;  // VPZ_SYNTH_ABLATE, tuning experiments only
    bool no_early_upload = false;  // VPZ_NO_EARLY_UPLOAD=1 (A/B tests): a host-memory call's H2D copies stay behind its host pass
    std::vector<int32_t> packet_samples;  // per packet of the last synth call
    std::vector<int64_t> mismatch_packets;  // packets of the last synth call that failed the window check (skipped)
};

}  // namespace vpz
