// The host plan of one vpz_decoder_synth call: pass 1 (StreamDecoder.ReadNextPacket / Read restated with integers), the cut of
// the frames into runs and the chaining of the runs.  Pure host code on integers: no call into the HIP runtime is made here;
// what the plan needs from the kernels' units (resident slots, waves of a stereo workgroup) the caller hands in as numbers.
#pragma once

#include <algorithm>

#include "host_pool.hpp"
#include "vpz_decoder.hpp"

namespace vpz {

// The facts of a batch that decide its route, gathered packet by packet (every packet that becomes a frame is noted once)
struct BatchFacts {
    bool any_floor = false, any_floor0 = false, need_coupling = false;
    bool any_short = false;       // the batch holds short blocks (run cutting by cost only pays then)
    bool ilv_seen = false, planar_seen = false;  // layouts of the packets that become frames (the dual kernel wants one)
    bool group_align_ok = true;   // every interleaved packet starts on a 16-byte boundary (group mode loads 16 bytes)
    bool align2_ok = true;        // every packet starts on an 8-byte boundary (planar packets are read 8 bytes at a time)
    bool all_steady_flags = true; // every packet: a long block with long windows on both sides, already floored, planar
    int64_t res_extent = 0;
    void note(const Decoder &D, const vpz_packet &pk)
    {
        const bool bf = pk.flags & VPZ_PKT_BLOCK_FLAG;
        if (!bf) any_short = true;
        res_extent = std::max(res_extent, pk.residue_offset + (int64_t)D.channels * ((bf ? D.size1 : D.size0) / 2));
        if (!(pk.flags & VPZ_PKT_NO_FLOOR)) {
            any_floor = true;
            if (D.mappings[pk.mapping].coupling_steps > 0) need_coupling = true;
            if (D.mapping_uses_floor0[pk.mapping]) any_floor0 = true;
        }
        if (pk.flags & VPZ_PKT_INTERLEAVED) { need_coupling = true; ilv_seen = true; }
        else planar_seen = true;
        if (pk.residue_offset & 3) group_align_ok = false;  // group mode reads every packet in 16-byte pieces
        if (pk.residue_offset & 1) align2_ok = false;
        if ((pk.flags & (7u | VPZ_PKT_NO_FLOOR | VPZ_PKT_INTERLEAVED)) != (7u | VPZ_PKT_NO_FLOOR)) all_steady_flags = false;
    }
    void merge(const BatchFacts &o)
    {
        any_floor |= o.any_floor; any_floor0 |= o.any_floor0; need_coupling |= o.need_coupling; any_short |= o.any_short;
        ilv_seen |= o.ilv_seen; planar_seen |= o.planar_seen; group_align_ok &= o.group_align_ok; align2_ok &= o.align2_ok;
        all_steady_flags &= o.all_steady_flags;
        res_extent = std::max(res_extent, o.res_extent);
    }
};

struct SynthPlan {
    // ---- what the plan reads: the decoder (setup, A/B switches, the streams' states, D.plan), the call's packets, and
    Decoder &D;
    const int64_t n_packets;
    const vpz_packet *packets;
    const bool have_posts;
    const int mem_space;              // ... where the residue lies and how it is aligned (which kernels can read it in place),
    const uintptr_t residue_addr;
    const bool out_interleaved;
    const int64_t stream_out_capacity;
    PinnedArena *A = nullptr;         // ... the arena the descriptor tables are carved from, in this order: frames or flag bytes,
                                      // rec_floor, runs, run_inline
    HostPool *pool = nullptr;         // ... the context's pool if it is this decoder's (else nullptr: everything on the calling thread)
    int parties = 1;                  // ... the host threads the decoder's calls may use
    // ... and of the kernels' units: the waves of a stereo workgroup, whether the sizes need synth_kernel's general variant, and
    // the resident wave slots of the kernel this plan leads to -- asked for only when no cut hint is reused (the answer comes
    // from the HIP runtime: the caller's business, and not free)
    int dual_waves = 1;
    bool needs_general = false;
    int64_t (*resident_slots)(const SynthPlan &) = nullptr;
    // ---- what it produces
    std::vector<StreamState> st;  // the streams' states after the batch: committed when the batch is accepted
    std::vector<uint8_t> started_with_prev, started_prev_long;
    FrameDesc *frames = nullptr;
    size_t n_frames = 0;
    uint8_t *rec_floor = nullptr;  // per channel record: floor index | 0x40 type-0 | 0x80 long block
    BatchFacts facts;
    bool was_parallel = false;    // pass 1 ran on the pool
    bool use_group = false;       // decided after pass 1: synth_kernel's group mode instead of the coupling pass
    bool use_dual = false;        // ... or the stereo fast path (synth_dual.hip), which takes precedence
    bool cut_by_cost = false;     // plan_runs balanced the runs by cost (short blocks ride in batches): only then do the kernels
                                  // batch -- in runs of equal LENGTH the ones rich in short blocks would be done early and the
                                  // launch would wait for the others (configs[2]: 0.205 ms without batches, 0.211 with)
    bool compact = false;         // every run compact: two bytes per frame instead of a FrameDesc (parallel pass only)
    uint8_t *cflags = nullptr, *cmap = nullptr;
    uint8_t *run_inline = nullptr;  // [run][32]: the flag bytes of a run's first 16 staged frames (SynthArgs.run_inline)
    RunDesc *runs = nullptr;
    size_t n_runs = 0, runs_cap = 0;
    bool host_failed = false;  // a share of a fork-join threw (allocation): the call returns VPZ_E_NOMEM
    int64_t n_chained = 0;
    bool steady = false;       // one more batch fact, set with the runs: EVERY frame is the steady state of its stream (a 2048 block
                               // after a 2048 block, long windows on both sides, already floored, planar) or a stream's first block
                               // after a reset -- such a batch may take steady_stereo_kernel (the launch looks at the PCM's layout)
    int cut_R = 0;  // the run length (or cost target, in passes) plan_runs settled on
    int fill_threads = 1, chain_threads = 1;  // threads that wrote the run records / swept them for chaining (VPZ_HOST_PROFILE)

    int64_t capacity_of(int s) const  // (vpz_decoder_set_stream_capacities tightens the call's bound per stream)
    {
        return D.stream_caps.empty() ? stream_out_capacity : std::min(stream_out_capacity, D.stream_caps[(size_t)s]);
    }
    bool dual_usable() const;
    bool group_usable() const;
};

// Pass 1 and the choice of the route: frames (or compact flag bytes), rec_floor, the facts, per-stream counts and offsets
// (D.plan), the states after the batch, samples_written.  VPZ_OK or the error already set on the context.
int plan_frames(SynthPlan &P, int64_t *samples_written);
// Pass 2: runs, run_inline.  Failure: P.host_failed.
void plan_runs(SynthPlan &P);

}  // namespace vpz
