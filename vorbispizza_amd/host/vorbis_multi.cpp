// In-process multi-device dispatcher (include/vorbispizza_multi.h): one host process, several MI355X.
//
// The reference's host is ONE process in which a VorbisReader holds N independent StreamDecoders (VorbisReader.cs:56-85);
// SURVEY.md section 8e prescribes "one host thread + one HIP stream per device; per-device context and tables", streams
// partitioned contiguously, no collective.  This file is that: vpzm_decode_library shards a library of containers over the
// device groups (shard_range's rule), and every group runs, on its own threads, the pipeline
//
//   open (setup headers)  ->  entropy decode into page-locked batch arrays  ->  vpz_decoder_synth (host memory)  ->  PCM
//        host threads              host threads, one stream each                 `contexts_per_device` issuing threads
//
// with sub-batches of `streams_per_call` streams of one setup header per synth call, `slots_per_device` sub-batches in
// flight.  Nothing is shared between groups but the caller's arrays; the C ABI below them is used exactly as any other host
// would use it (one thread at a time per context / decoder).
//
// With vpzm_options.gpu_entropy a sub-batch of a setup the device can decode (vpzh_gpu_decode_supported) takes the same stages
// with other contents: the workers PLAN its streams (vpzh_plan_range: packet records, spans, the packets' bytes) into the slot,
// and its issuing thread uploads the bytes, entropy-decodes them on the lane's stream (vpz_entropy_decode) into arrays that
// never leave the device, synthesises from those and downloads every member's PCM.
//
// With vpzm_set_mixed_setups (include/vorbispizza_multi_mixed.h) on top of that, the streams of device-decodable setups that agree in
// channels, block sizes and residue type are cut into sub-batches together: such a sub-batch's setup is a MERGED one (Setup::parts),
// its records carry mapping indices of the merged setup, vpz_entropy_group_decode decodes it and a decoder of the merged setup
// synthesises it.
//
// vpzm_decode_ranges (include/vorbispizza_multi_ranges.h) is the same pipeline over a WINDOW of every stream (vpzh_window: the pre-roll
// packet through the packet of the window's last sample; a Job carries it, and for vpzm_decode_library it is the whole stream).  A
// ranges call's PCM is staged on both routes -- the lane's device array, or a page-locked array of the slot --
// and its download trims every member's window out of its area (device route: an asynchronous vpz_pcm_download per member, one
// synchronise for the sub-batch).
//
// vpzm_decode_ranges_batch (include/vorbispizza_multi_batch.h) is a ranges call whose PCM never comes down: both routes stage it in the
// lane's device array (the host route uploads its slot's decoded arrays and makes a device-memory synth call), and the `download` stage
// (deliver_batch) is one vpz_pcm_pack per sub-batch, which trims every member's window into its row of the caller's device tensor and zero-fills the rest.
//
// vpzm_decode_ranges_resampled (include/vorbispizza_multi_resample.h) is that call with vpz_pcm_resample as its last stage: open_one works out
// every entry's ratio, the synth calls write float32, and deliver_batch makes one launch per ratio among the sub-batch's members.
//
// vpzm_decode_ranges_logmel (include/vorbispizza_multi_logmel.h) is the mono resampled call with one more stage: the resample launches write
// into the lane's own temporary, and one vpz_pcm_logmel launch per sub-batch turns its rows into (log-)mel frames in the caller's tensor.
// vpzm_decode_ranges_melspec (include/vorbispizza_multi_melspec.h) is that call with vpz_pcm_melspec as the feature launch: transforms of
// 2048, 4096 and 8192 samples.
// vpzm_decode_ranges_stft (include/vorbispizza_multi_stft.h) keeps the channels and the spectrum: the resample launches write planar rows
// [members][C][frames] into the temporary, and vpz_pcm_stft takes every (member, channel) as a row of its own.
// vpzm_decode_ranges_cqt (include/vorbispizza_multi_cqt.h) is the STFT call with vpz_pcm_cqt as its feature stage: constant-Q spectrograms.
// vpzm_decode_ranges_fbank (include/vorbispizza_multi_fbank.h) is the same call with vpz_pcm_fbank as that stage: Kaldi filterbank frames.
// vpzm_decode_ranges_mfcc (include/vorbispizza_multi_mfcc.h) is the same call with vpz_pcm_mfcc as that stage: Kaldi MFCC frames.
// vpzm_decode_ranges_fbank_post / _mfcc_post (include/vorbispizza_multi_featpost.h) are those two with vpz_feat_post behind the feature
// launch: it writes a lane temporary [members][T][D], and the post launches deliver deltas and normalisation into the group's piece.
//
// vpzm_measure_loudness (include/vorbispizza_multi_loudness.h) is a batch call whose delivery measures instead of moving: one
// vpz_pcm_loudness launch per sample rate among a sub-batch's members, into a temporary of the lane's; the step sums and peaks come down
// in one small copy, and vpz_loudness_gate runs per member on the issuing thread.  Its "piece" is the group's part of the caller's records.
// vpzm_measure_r128 (include/vorbispizza_multi_r128.h) is that call with one vpz_pcm_true_peak launch per rate beside the loudness one --
// the true peaks ride in the same copy -- and vpz_loudness_range and vpz_loudness_maxima beside the gate.
//
// vpzm_decode_ranges_normalized (include/vorbispizza_multi_normalize.h) is the resampled call with vpz_pcm_normalize as its last stage: the
// resample launches write planar rows into the lane's temporary, as for an STFT call, and one launch set per sub-batch delivers them
// normalised into the group's piece in the caller's layout; its loudness mode measures a sub-batch's members first, as the loudness call does.
//
// In the file's order: Setup, Buffer (the one owner of a page-locked or device array; Slot and Lane hold lists of them), SetupCache,
// Switches (the VPZM_* environment of one call), GroupRun (a group's pipeline) and SubCall (a sub-batch's synth step, stage by stage).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/vorbispizza_multi.h"
#include "../../include/vorbispizza_multi_mixed.h"
#include "../../include/vorbispizza_multi_ranges.h"
#include "../../include/vorbispizza_multi_batch.h"
#include "../../include/vorbispizza_pcm.h"
#include "../../include/vorbispizza_pcm_pack.h"
#include "../../include/vorbispizza_pcm_resample.h"
#include "../../include/vorbispizza_multi_resample.h"
#include "../../include/vorbispizza_pcm_logmel.h"
#include "../../include/vorbispizza_multi_logmel.h"
#include "../../include/vorbispizza_pcm_melspec.h"
#include "../../include/vorbispizza_multi_melspec.h"
#include "../../include/vorbispizza_pcm_stft.h"
#include "../../include/vorbispizza_multi_stft.h"
#include "../../include/vorbispizza_pcm_cqt.h"
#include "../../include/vorbispizza_multi_cqt.h"
#include "../../include/vorbispizza_pcm_fbank.h"
#include "../../include/vorbispizza_multi_fbank.h"
#include "../../include/vorbispizza_pcm_mfcc.h"
#include "../../include/vorbispizza_multi_mfcc.h"
#include "../../include/vorbispizza_pcm_featpost.h"
#include "../../include/vorbispizza_multi_featpost.h"
#include "../../include/vorbispizza_pcm_loudness.h"
#include "../../include/vorbispizza_multi_loudness.h"
#include "../../include/vorbispizza_pcm_r128.h"
#include "../../include/vorbispizza_multi_r128.h"
#include "../../include/vorbispizza_pcm_normalize.h"
#include "../../include/vorbispizza_multi_normalize.h"
#include "../../include/vorbispizza_entropy_group.h"

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// what a vpz_decoder is created from: the setup-header products of a stream (StreamDecoder.cs:213-353)
struct Setup {
    vpzh_info info{};
    std::vector<vpz_floor1_config> floors;
    std::vector<vpz_floor0_config> floors0;
    std::vector<uint8_t> floor_types;
    std::vector<vpz_mapping_config> mappings;
    int f0_stride = 0;
    bool integral = false;  // every residue value is an integer of 16 bits: the residue travels as int16 (half the link bytes)
    std::vector<uint8_t> image;  // gpu_entropy, a setup the device can decode: its entropy setup image (else empty)
    // mixed_setups, a MERGED setup: the union of the Floor1 configurations of `parts` (equal ones shared) and their mappings back to
    // back with channel_floor remapped -- the C++ counterpart of sharding.merge_setups; part q's mapping i is mapping_base[q] + i.
    // It has no image of its own: the parts' images, in order, are its entropy group's
    std::vector<std::shared_ptr<Setup>> parts;
    std::vector<int> mapping_base;
    static constexpr size_t kMergedMost = 256;   // mappings (a record's index is a byte) and parts (a group's images) of a merged setup
    static constexpr size_t kMergedFloors = 64;  // ... and its floors: what vpz_decoder_create accepts

    bool load(vpzh_stream *h, bool gpu_entropy)
    {
        if (vpzh_get_info(h, &info) != VPZH_OK) return false;
        floors.assign((size_t)info.floor_count, vpz_floor1_config{});
        floors0.assign((size_t)info.floor_count, vpz_floor0_config{});
        floor_types.assign((size_t)info.floor_count, 1);
        mappings.assign((size_t)info.mapping_count, vpz_mapping_config{});
        for (int i = 0; i < info.floor_count; ++i) {
            const int t = vpzh_get_floor_type(h, i);
            floor_types[i] = (uint8_t)t;
            if ((t == 0 ? vpzh_get_floor0(h, i, &floors0[i]) : vpzh_get_floor1(h, i, &floors[i])) != VPZH_OK) return false;
        }
        for (int i = 0; i < info.mapping_count; ++i)
            if (vpzh_get_mapping(h, i, &mappings[i]) != VPZH_OK) return false;
        f0_stride = vpzh_max_floor0_order(h);
        integral = vpzh_residue_is_integral(h) != 0;
        uint64_t bytes = 0;
        if (gpu_entropy && vpzh_gpu_decode_supported(h) && vpzh_get_entropy_setup(h, nullptr, 0, &bytes) == VPZH_OK) {
            image.resize((size_t)bytes);
            if (vpzh_get_entropy_setup(h, image.data(), bytes, &bytes) != VPZH_OK) image.clear();
        }
        return true;
    }
    bool on_device() const { return !image.empty() || !parts.empty(); }
    // the merge class: two setups may share a merged setup (a decoder, an entropy group)
    bool same_class(const Setup &o) const
    {
        return info.channels == o.info.channels && info.block_size0 == o.info.block_size0 && info.block_size1 == o.info.block_size1 &&
               integral == o.integral && on_device() && o.on_device();
    }
    int part_of(const Setup &o) const
    {
        for (size_t q = 0; q < parts.size(); ++q)
            if (parts[q]->same(o)) return (int)q;
        return -1;
    }
    static bool same_floor1(const vpz_floor1_config &a, const vpz_floor1_config &b)
    {
        return a.x_count == b.x_count && a.multiplier == b.multiplier &&
               memcmp(a.x_list, b.x_list, sizeof(int32_t) * (size_t)std::max(0, a.x_count)) == 0;
    }
    // where floor f lies in the union: in `floors`, or behind them in `fresh` (those of the coming part that the union does not have yet;
    // floors.size() + fresh.size(): in neither)
    size_t floor_in_union(const vpz_floor1_config &f, const std::vector<vpz_floor1_config> &fresh) const
    {
        size_t at = 0;
        while (at < floors.size() && !same_floor1(floors[at], f)) ++at;
        if (at < floors.size()) return at;
        for (at = 0; at < fresh.size() && !same_floor1(fresh[at], f); ++at) {}
        return floors.size() + at;
    }
    // a merged setup can take one more part: with it, it holds at most `most_mappings` mappings (kMergedMost at the most), kMergedFloors
    // floors and kMergedMost parts -- an empty one takes any part (a single setup is what a decoder was created from before)
    bool fits(const Setup &o, size_t most_mappings) const
    {
        if (parts.empty()) return true;
        std::vector<vpz_floor1_config> fresh;
        for (const vpz_floor1_config &f : o.floors)
            if (floor_in_union(f, fresh) == floors.size() + fresh.size()) fresh.push_back(f);
        return mappings.size() + o.mappings.size() <= std::min(most_mappings, kMergedMost) && floors.size() + fresh.size() <= kMergedFloors &&
               parts.size() < kMergedMost;
    }
    // ... and takes it (the caller has asked `fits`)
    void add_part(const std::shared_ptr<Setup> &o)
    {
        std::vector<vpz_floor1_config> fresh;
        std::vector<uint8_t> remap(o->floors.size(), 0);
        for (size_t i = 0; i < o->floors.size(); ++i) {
            const size_t at = floor_in_union(o->floors[i], fresh);
            if (at == floors.size() + fresh.size()) fresh.push_back(o->floors[i]);
            remap[i] = (uint8_t)at;
        }
        if (parts.empty()) {
            info = o->info;
            integral = o->integral;
        }
        mapping_base.push_back((int)mappings.size());
        for (vpz_mapping_config mc : o->mappings) {
            for (int c = 0; c < info.channels; ++c) mc.channel_floor[c] = remap[mc.channel_floor[c]];
            mappings.push_back(mc);
        }
        floors.insert(floors.end(), fresh.begin(), fresh.end());
        floors0.assign(floors.size(), vpz_floor0_config{});
        floor_types.assign(floors.size(), 1);  // (the device decodes no type-0 floor: a merge class has none)
        info.floor_count = (int32_t)floors.size();
        info.mapping_count = (int32_t)mappings.size();
        parts.push_back(o);
    }
    // the same decoder serves two streams iff everything it was created from is the same
    bool same(const Setup &o) const
    {
        if (info.channels != o.info.channels || info.block_size0 != o.info.block_size0 || info.block_size1 != o.info.block_size1 ||
            floors.size() != o.floors.size() || mappings.size() != o.mappings.size() || floor_types != o.floor_types || integral != o.integral)
            return false;
        // (the synthesis does not know the codebooks, the device's entropy decode does: equal setup headers give equal images)
        if (image != o.image || parts.size() != o.parts.size()) return false;
        for (size_t q = 0; q < parts.size(); ++q)
            if (parts[q]->image != o.parts[q]->image) return false;
        for (size_t i = 0; i < floors.size(); ++i) {
            if (floor_types[i] == 0) {
                if (memcmp(&floors0[i], &o.floors0[i], sizeof floors0[i]) != 0) return false;
            } else if (!same_floor1(floors[i], o.floors[i])) {
                return false;
            }
        }
        for (size_t i = 0; i < mappings.size(); ++i)
            if (memcmp(&mappings[i], &o.mappings[i], sizeof mappings[i]) != 0) return false;
        return true;
    }
};

// The one owner of an array of a slot (page-locked host memory) or of a lane (device memory).  It only grows: a request for
// `need` elements of `elem` bytes gets room for a quarter more and 64, so that jobs of like size do not allocate again.  The
// old array may go at once: a slot is prepared when no sub-batch holds it, a lane's stream is idle between its sub-batches.
struct Buffer {
    bool device = false;
    void *p = nullptr;
    size_t bytes = 0;
    void release(vpz_context *ctx)
    {
        if (p && ctx) (void)(device ? vpz_device_free(ctx, p) : vpz_host_free(ctx, p));
        p = nullptr;
        bytes = 0;
    }
    bool grow(vpz_context *ctx, size_t need, size_t elem)
    {
        if (need * elem <= bytes) return true;
        release(ctx);
        const size_t want = (need + need / 4 + 64) * elem;
        if ((device ? vpz_device_alloc(ctx, (uint64_t)want, &p) : vpz_host_alloc(ctx, (uint64_t)want, &p)) != VPZ_OK) p = nullptr;
        bytes = p ? want : 0;
        return p != nullptr;
    }
};

// What a context keeps per setup header, looked up by Setup::same: a library of files from many encoders meets many setups, and
// a context keeps the decoders (and entropy setups: as many) of the last few, not of every one it has seen -- the oldest goes
template <class T>
struct SetupCache {
    static constexpr size_t kKept = 8;
    void (*destroy)(T *);
    std::vector<std::pair<std::shared_ptr<Setup>, T *>> kept;
    T *find(const Setup &st) const
    {
        for (const auto &e : kept)
            if (e.first->same(st)) return e.second;
        return nullptr;
    }
    void keep(const std::shared_ptr<Setup> &st, T *made)
    {
        if (kept.size() >= kKept) {
            destroy(kept.front().second);
            kept.erase(kept.begin());
        }
        kept.emplace_back(st, made);
    }
    void clear()
    {
        for (const auto &e : kept) destroy(e.second);
        kept.clear();
    }
};

struct Lane {  // one context (HIP stream) of a device group and the decoders that live on it
    vpz_context *ctx = nullptr;
    SetupCache<vpz_decoder> decoders{vpz_decoder_destroy, {}};
    // gpu_entropy: the entropy setups next to the decoders (a setup belongs to a context and serves one call at a time), and
    // what a device-decoded sub-batch keeps on the device: packet bytes in, residue / posts / counts between the two calls, PCM out
    SetupCache<vpz_entropy_setup> esetups{vpz_entropy_setup_destroy, {}};
    SetupCache<vpz_entropy_group> egroups{vpz_entropy_group_destroy, {}};  // mixed_setups: the groups of the merged setups, kept alike
    // (kF0Amp, kF0Coeff: a batch call's host route uploads a type-0 floor's data beside residue, posts and counts)
    // (kMono: a log-mel call's resampled mono rows [members][frames], between the resample launches and the vpz_pcm_logmel launch that
    // reads them -- an STFT call's are [members][channels][frames], every channel a row of the vpz_pcm_stft launch; the lane owns it, it only grows, and it goes with the lane when the dispatcher is destroyed)
    // (kLoud: a loudness call's step sums [members][max_steps] float64 and, behind them, peaks [members] float32, between the
    // vpz_pcm_loudness launches and the one copy that brings them down; an R 128 call's true peaks [members] float32 lie behind the peaks;
    // owned like kMono)
    // (kFeat: a posted fbank or MFCC call's feature frames [members][T][D] float32, between the feature launch and the vpz_feat_post
    // launches that read them; kPostScratch: those launches' chunk sums, float64 -- and a normalised call's, sized by its own stage's
    // rule: one array, whichever call grew it last; kNormResult: a normalised call's vpz_norm_result [members], between the launches and
    // the copy that brings them down; owned like kMono)
    enum { kPayload, kResidue, kPosts, kCounts, kPcm, kF0Amp, kF0Coeff, kMono, kLoud, kFeat, kPostScratch, kNormResult, kBuffers };
    Buffer buf[kBuffers] = {{true}, {true}, {true}, {true}, {true}, {true}, {true}, {true}, {true}, {true}, {true}, {true}};  // (device memory, every one)
    uint8_t *payload() const { return static_cast<uint8_t *>(buf[kPayload].p); }
    float *residue() const { return static_cast<float *>(buf[kResidue].p); }  // (float32 or int16 values; the ABI's parameter is float-typed)
    int16_t *posts() const { return static_cast<int16_t *>(buf[kPosts].p); }
    uint8_t *counts() const { return static_cast<uint8_t *>(buf[kCounts].p); }
    char *pcm() const { return static_cast<char *>(buf[kPcm].p); }
    float *f0_amp() const { return static_cast<float *>(buf[kF0Amp].p); }
    float *f0_coeff() const { return static_cast<float *>(buf[kF0Coeff].p); }
    float *mono() const { return static_cast<float *>(buf[kMono].p); }
    float *feat() const { return static_cast<float *>(buf[kFeat].p); }
};

struct Slot {  // page-locked batch arrays of one sub-batch in flight (a device-decoded one holds packets, spans and payload only)
    // (kStage: a ranges call's host route writes its members' PCM areas here, and `download` copies every window out of them)
    enum { kPackets, kResidue, kPosts, kCounts, kF0Amp, kF0Coeff, kSpans, kPayload, kStage, kBuffers };
    Buffer buf[kBuffers];
    vpz_packet *packets() const { return static_cast<vpz_packet *>(buf[kPackets].p); }
    float *residue_f32() const { return static_cast<float *>(buf[kResidue].p); }  // (one array: a sub-batch's residue travels as float32 ...
    int16_t *residue_i16() const { return static_cast<int16_t *>(buf[kResidue].p); }  // ... or as int16, see use_i16)
    int16_t *posts() const { return static_cast<int16_t *>(buf[kPosts].p); }
    uint8_t *counts() const { return static_cast<uint8_t *>(buf[kCounts].p); }
    float *f0_amp() const { return static_cast<float *>(buf[kF0Amp].p); }
    float *f0_coeff() const { return static_cast<float *>(buf[kF0Coeff].p); }
    vpz_entropy_span *spans() const { return static_cast<vpz_entropy_span *>(buf[kSpans].p); }
    uint8_t *payload() const { return static_cast<uint8_t *>(buf[kPayload].p); }
    char *stage() const { return static_cast<char *>(buf[kStage].p); }
    size_t bytes() const
    {
        size_t sum = 0;
        for (const Buffer &b : buf) sum += b.bytes;
        return sum;
    }
};

struct Group {
    int device = 0;
    std::vector<Lane> lanes;
    std::vector<Slot> slots;
};

constexpr int64_t kCallValues = (int64_t)64 << 20;  // residue values of one synth call (256 MiB as float32), see GroupRun::cut

// The VPZM_* test and diagnosis switches of the environment as one vpzm_decode_library / vpzm_decode_ranges call finds them (its GroupRuns carry a copy)
struct Switches {
    static int64_t number(const char *name) { return getenv(name) ? atoll(getenv(name)) : 0; }
    int64_t max_call_values = number("VPZM_MAX_CALL_VALUES") > 0 ? number("VPZM_MAX_CALL_VALUES") : kCallValues;  // (tests: small calls)
    int64_t max_merged_mappings = number("VPZM_MAX_MERGED_MAPPINGS") > 0 ? number("VPZM_MAX_MERGED_MAPPINGS") : (int64_t)Setup::kMergedMost;  // (tests: small merged setups)
    bool fail_gpu_entropy = number("VPZM_FAIL_GPU_ENTROPY") != 0;  // (tests: every device-decoded sub-batch is refused, so that the host path after all runs)
    bool fail_batch_calls = number("VPZM_FAIL_BATCH_CALLS") != 0;  // (tests: every sub-batch's call counts as failed, so that the member-by-member path runs)
    bool fail_delivery = number("VPZM_FAIL_DELIVERY") != 0;        // (tests: a batch call's delivery launch -- pack, resample, the feature launch of a log-mel, mel-spectrogram, STFT, CQT, fbank or MFCC call, a loudness call's or a normalised call's vpz_pcm_normalize -- is not made and counts as failed)
    bool profile = getenv("VPZM_PROFILE") != nullptr;              // a line per sub-batch on stderr
    bool no_synth = getenv("VPZM_NO_SYNTH") != nullptr;            // (diagnosis: the decode side of the pipeline alone)
};

}  // namespace

struct vpzm_dispatcher {
    std::vector<Group> groups;
    vpzm_options opt{};
    int device_streams_per_call = 0;  // gpu_entropy: streams of a device-decoded call (opt.streams_per_call: of a host-decoded one)
    int call_streams() const { return std::max(opt.streams_per_call, device_streams_per_call); }  // what a decoder is created for
    bool mixed_setups = false;        // vpzm_set_mixed_setups: device-decoded sub-batches may hold streams of several setups
    vpzm_call_counts counts{};        // of the last vpzm_decode_library call
    std::string error;
    std::mutex err_mu;
    std::mutex call_mu;  // vpzm_decode_library holds it: calls from several host threads take the dispatcher in turn
    void fail(const std::string &what)
    {
        std::lock_guard<std::mutex> g(err_mu);
        if (error.empty()) error = what;
    }
};

namespace {

constexpr int kNoDecoder = 1;  // (SubCall: no decoder for the sub-batch's setup; not a VPZ_* status, those are <= 0)

struct Job {  // one stream of the library inside its group
    int32_t k = 0;  // index in the caller's arrays
    vpzh_stream *h = nullptr;
    std::shared_ptr<Setup> own;  // its setup-header products, loaded when it is opened
    // its WINDOW (vpzh_window; vpzm_decode_library: the whole stream): `packets` packets from `first`, `residue_floats` values in them;
    // the decoder's stream starts at `position`, and the caller gets `wanted` samples of what they give after dropping `roll`
    int64_t first = 0, packets = 0, residue_floats = 0, roll = 0, wanted = 0, position = 0;
    int64_t total_samples = 0;
    int64_t payload_bytes = 0, plan_failures = 0;  // gpu_entropy: what its plan needs in the payload area; packets its plan gave up
    int part = 0;  // mixed_setups: which part of its class's merged setup its own setup is
    int32_t up = 1, down = 1;  // a resampled call: the batch's rate / the stream's, in lowest terms
    int32_t status = VPZM_OK;
    bool finished = false;  // its PCM has been written (or it has its own failure status): what an aborted run leaves alone
    bool row_packed = false;  // a batch call: a pack launch has defined its row (the others get their zeros when the run ends)
    void close()
    {
        if (h) vpzh_close(h);
        h = nullptr;
    }
};

// One kind of feature call, stated once: a resampled call with a feature stage behind the resample launches, fed from the lane's
// temporary.  The stage's step in a failure text, the entry point, the profile line's word, what GroupRun::zero_rows calls its rows of
// no samples; whether a descriptor stands for its entry's `channels` rows or for one (mono); the launch, vpz_pcm_* of the kind
struct Feature {
    const char *step, *call, *name, *empty;
    bool per_channel;
    int (*launch)(vpz_context *ctx, const void *src, int64_t src_elems, int64_t frames, const void *spec, int32_t n, const vpz_pack_row *rows, void *to, int64_t to_rows);
};
template <class Spec, int (*Fn)(vpz_context *, const void *, int64_t, int64_t, const Spec *, int32_t, const vpz_pack_row *, void *, int64_t)>  // (the spec cast back to the type its entry point took)
int launch_of(vpz_context *ctx, const void *src, int64_t src_elems, int64_t frames, const void *spec, int32_t n, const vpz_pack_row *rows, void *to, int64_t to_rows)
{
    return Fn(ctx, src, src_elems, frames, static_cast<const Spec *>(spec), n, rows, to, to_rows);
}
// `dst` is [rows][n_mels][T] (the mel spectrogram: with the transform sizes of vorbispizza_pcm_melspec.h), [rows][T][n_mels], [rows][T][n_ceps],
// and entry k's channel c in row (k - lo) * channels + c of [rows][channels][n_freq or n_bins][T], complex pairs included -- or transposed
const Feature kLogmel{"vpz_pcm_logmel", "vpzm_decode_ranges_logmel", "log-mel", "silence rows", false, launch_of<vpz_logmel_spec, vpz_pcm_logmel>};
const Feature kMelspec{"vpz_pcm_melspec", "vpzm_decode_ranges_melspec", "mel-spectrogram", "silence rows", false, launch_of<vpz_logmel_spec, vpz_pcm_melspec>};
const Feature kFbank{"vpz_pcm_fbank", "vpzm_decode_ranges_fbank", "fbank", "pad rows", false, launch_of<vpz_fbank_spec, vpz_pcm_fbank>};
const Feature kMfcc{"vpz_pcm_mfcc", "vpzm_decode_ranges_mfcc", "mfcc", "pad rows", false, launch_of<vpz_mfcc_spec, vpz_pcm_mfcc>};
const Feature kStft{"vpz_pcm_stft", "vpzm_decode_ranges_stft", "stft", "zero rows", true, launch_of<vpz_stft_spec, vpz_pcm_stft>};
const Feature kCqt{"vpz_pcm_cqt", "vpzm_decode_ranges_cqt", "cqt", "zero rows", true, launch_of<vpz_cqt_spec, vpz_pcm_cqt>};
// (a normalised call: the delivery stage has gains, scratch memory and a result array beside the rows -- Batch::norm_rows launches it)
const Feature kNormalized{"vpz_pcm_normalize", "vpzm_decode_ranges_normalized", "normalize", "zero rows", false, nullptr};

// vpzm_decode_ranges_batch: what the call delivers into instead of the caller's host array -- one group's piece of the batch (rows of
// `channels * frames` elements in `layout`, entry k of the group in row k - lo); dst == nullptr: not a batch call
struct Batch {
    // what delivers a window into its row: vpz_pcm_pack; vpz_pcm_resample, and behind it the launch of `feature` where there is one; or,
    // into its record, vpz_pcm_loudness and the gate; or those with vpz_pcm_true_peak, the range and the maxima
    enum Kind { kPack, kResampled, kLoudness, kR128 };
    Kind kind = kPack;
    int32_t channels = 0, layout = 0;
    int64_t frames = 0;
    int32_t rate = 0, downmix = 0;  // kResampled: every row at `rate`, mixed down to mono with `downmix`
    // a feature call: its kind and its spec, of the type the kind's launch casts it back to; channels, layout and frames are then those
    // of the resampled rows in the lane's temporary -- planar float32, mono where the kind is
    const Feature *feature = nullptr;
    const void *spec = nullptr;
    // a posted call (fbank, MFCC): vpz_feat_post of this spec behind the feature launch (`dst` is [rows][T][D_out] or transposed), the
    // feature spec's mel stage and the feature launch's columns D; null: none
    const vpz_feat_post_spec *post = nullptr;
    const vpz_fbank_spec *post_mel = nullptr;
    int32_t post_D = 0;
    // a normalised call (feature == &kNormalized): vpz_pcm_normalize of this spec delivers the lane's temporary into the group's piece in
    // `norm_layout`, one of the four; `norm_out`: the caller's records, entry k's at [k] (null: none wanted)
    const vpzm_norm_spec *norm = nullptr;
    int32_t norm_layout = 0;
    vpzm_norm_out *norm_out = nullptr;
    // kLoudness: no tensor and no row length (`frames` caps nothing, `channels` is every stream's own); `dst` is the group's part of the
    // caller's records, HOST memory -- vpzm_loudness[rows], filled with the empty record before the run.  kR128: the same with vpzm_r128
    void *dst = nullptr;  // (decode_call fills these two in)
    int64_t rows = 0;     // of the group's piece: its entries
    // (members are initialised by name: with a constructor of its own a Batch is no aggregate, and no initialiser can depend on their order)
    Batch(Kind kind = kPack, int32_t channels = 0, int32_t layout = 0, int64_t frames = 0, int32_t rate = 0, int32_t downmix = 0, const Feature *feature = nullptr, const void *spec = nullptr)
        : kind(kind), channels(channels), layout(layout), frames(frames), rate(rate), downmix(downmix), feature(feature), spec(spec) {}
    static Batch featured(const Feature &feature, const void *spec, int32_t rate, int32_t downmix, int32_t channels, int64_t frames) { return Batch(kResampled, channels, VPZ_OUT_PLANAR, frames, rate, downmix, &feature, spec); }
    bool resampled() const { return kind == kResampled; }
    bool measured() const { return kind == kLoudness || kind == kR128; }
    vpzm_loudness &record(int64_t row) const { return static_cast<vpzm_loudness *>(dst)[row]; }
    vpzm_r128 &record_r128(int64_t row) const { return static_cast<vpzm_r128 *>(dst)[row]; }
    // the feature launch of the call's kind: these windows of a mono float32 array into their rows of `to` (the group's piece, or a
    // posted call's temporary), which has `to_rows` rows.  A per-channel kind's array is planar -- a descriptor's `src` is the window in its
    // member's first channel, the next channel lies `frames` elements on (none is read where samples = 0) -- and a descriptor stands for
    // its entry's `channels` rows: one descriptor of the launch per channel
    int feature_rows(vpz_context *ctx, const void *src, int64_t src_elems, const std::vector<vpz_pack_row> &d, void *to, int64_t to_rows) const
    {
        if (!feature->per_channel) return feature->launch(ctx, src, src_elems, frames, spec, (int32_t)d.size(), d.data(), to, to_rows);
        std::vector<vpz_pack_row> each;
        each.reserve(d.size() * (size_t)channels);
        for (const vpz_pack_row &r : d)
            for (int32_t c = 0; c < channels; ++c) each.push_back(vpz_pack_row{r.samples > 0 ? r.src + c * frames : 0, r.samples, r.row * channels + c});
        return feature->launch(ctx, src, src_elems, frames, spec, (int32_t)each.size(), each.data(), to, to_rows * channels);
    }
    // a posted call: a row's frames T and its real frames T_L of J samples
    int64_t feat_T() const { return 1 + (frames - post_mel->win) / post_mel->hop; }
    int64_t real_frames(int64_t J) const { return J < post_mel->win ? 0 : 1 + (J - post_mel->win) / post_mel->hop; }
    // a posted call's vpz_feat_post launches on the lane's stream: rows of `src` ([src_rows][T][D], the lane's temporary) into their rows
    // of `dst`; the chunk sums live in the lane's scratch array, which grows here
    // `*own`: the text of a failure that is not the context's (its last error says nothing about it), else null.  Descriptors without
    // real frames (pad rows) need no chunk sums: no scratch memory is sized or grown for them
    int post_rows(Lane &L, const void *src, int64_t src_rows, const std::vector<vpz_feat_row> &d, const char **own) const
    {
        *own = nullptr;
        int64_t need = 0;
        bool any_real = false;
        for (const vpz_feat_row &r : d) any_real = any_real || r.real_frames > 0;
        if (any_real && vpz_feat_post_scratch(post, (int32_t)d.size(), feat_T(), post_D, &need) != VPZ_OK) {
            *own = "the scratch memory's size overflows";
            return VPZ_E_INVALID_ARG;
        }
        if (need > 0 && !L.buf[Lane::kPostScratch].grow(L.ctx, (size_t)need, sizeof(double))) {
            *own = "the chunk sums' device memory could not be allocated";
            return VPZ_E_NOMEM;
        }
        return vpz_feat_post(L.ctx, src, src_rows, feat_T(), post_D, post, (int32_t)d.size(), d.data(), dst, rows, need > 0 ? L.buf[Lane::kPostScratch].p : nullptr,
                             need);
    }

    bool by_loudness() const { return norm && norm->mode == VPZM_NORM_LOUDNESS; }
    // a normalised call's vpz_pcm_normalize launches on the lane's stream: windows of the planar array `src` into their rows of `dst`.
    // The loudness mode delivers through the descriptors' gains, the gain mode through the spec's one; the chunk sums live in the lane's
    // scratch array and the result records (`want_result`) in its result array, which grow here.  `*own` as in post_rows.  Descriptors
    // without samples (zero rows) need neither
    int norm_rows(Lane &L, const void *src, int64_t src_elems, std::vector<vpz_norm_row> &d, bool want_result, const char **own) const
    {
        *own = nullptr;
        vpz_norm_spec stage{};
        stage.mode = by_loudness() ? VPZ_NORM_GAIN : norm->mode;
        stage.channels = channels;
        stage.target = norm->target;
        stage.eps = norm->eps;
        stage.ceiling = norm->ceiling;
        bool any_real = false;
        for (vpz_norm_row &r : d) {
            any_real = any_real || r.samples > 0;
            if (!by_loudness()) r.gain = stage.mode == VPZ_NORM_GAIN ? norm->target : 1.0;
        }
        want_result = want_result && any_real;
        int64_t need = 0;
        if (any_real && (stage.mode != VPZ_NORM_GAIN || stage.ceiling > 0.0 || want_result) &&
            vpz_pcm_normalize_scratch((int32_t)d.size(), channels, frames, &need) != VPZ_OK) {
            *own = "the scratch memory's size overflows";
            return VPZ_E_INVALID_ARG;
        }
        if (need > 0 && !L.buf[Lane::kPostScratch].grow(L.ctx, (size_t)need, sizeof(double))) {
            *own = "the chunk sums' device memory could not be allocated";
            return VPZ_E_NOMEM;
        }
        if (want_result && !L.buf[Lane::kNormResult].grow(L.ctx, d.size(), sizeof(vpz_norm_result))) {
            *own = "the result records' device memory could not be allocated";
            return VPZ_E_NOMEM;
        }
        return vpz_pcm_normalize(L.ctx, src, src_elems, frames, &stage, (int32_t)d.size(), d.data(), dst, rows, norm_layout,
                                 need > 0 ? L.buf[Lane::kPostScratch].p : nullptr, need,
                                 want_result ? static_cast<vpz_norm_result *>(L.buf[Lane::kNormResult].p) : nullptr);
    }

    // These descriptors (samples = 0 each) get rows of no samples -- zeros, or the silence row of a log-mel call or the pad_value row of
    // an fbank or MFCC call (a posted one: the post spec's), which their own kernels write -- from a launch that reads nothing: the
    // destination stands in for a source of no elements
    int empty_rows(Lane &L, const std::vector<vpz_pack_row> &d) const
    {
        if (post) {
            std::vector<vpz_feat_row> none;
            for (const vpz_pack_row &r : d) none.push_back(vpz_feat_row{0, 0, r.row});
            const char *own;  // (no scratch memory is asked for: none can fail)
            return post_rows(L, dst, 0, none, &own);
        }
        if (norm) {
            std::vector<vpz_norm_row> none;
            for (const vpz_pack_row &r : d) none.push_back(vpz_norm_row{0, 0, r.row, 1.0});
            const char *own;  // (no memory is asked for: none can fail)
            return norm_rows(L, dst, 0, none, false, &own);
        }
        if (feature) return feature_rows(L.ctx, dst, 0, d, dst, rows);
        return vpz_pcm_pack(L.ctx, dst, 0, channels, (int32_t)d.size(), d.data(), dst, rows, frames, layout);
    }
    const char *empty_step() const { return post ? "vpz_feat_post" : feature ? feature->step : "vpz_pcm_pack"; }
    const char *empty_words() const { return post ? "pad rows" : feature ? feature->empty : "zero rows"; }  // what that launch's rows are called
};

// ceil(samples * up / down): the output samples of a resampled window (the definition's J)
int64_t resampled_length(int64_t samples, int32_t up, int32_t down) { return (samples * up + down - 1) / down; }
// the window rule: of the `written` samples its window's packets gave, a member delivers those behind the roll, never more than it asked for
int64_t delivered_length(int64_t wanted, int64_t written, int64_t roll) { return std::max<int64_t>(0, std::min(wanted, written - roll)); }

struct Sub {  // streams of one setup that ride in one vpz_decoder_synth call
    std::shared_ptr<Setup> st;           // (its own reference: `setups` grows under the group's mutex while sub-batches are worked on outside it)
    std::vector<int> members;            // indices into jobs
    std::vector<int64_t> pbase, rbase;   // where each member's packets / residue start in the slot's arrays
    std::vector<int64_t> ybase;          // ... and its packet bytes in the slot's payload area (a device-decoded sub-batch)
    std::vector<uint8_t> part;           // a MIXED sub-batch (`st` is a merged setup): each member's part of it; empty otherwise
    bool mixed() const { return !part.empty(); }
    int mapping_shift(size_t j) const { return mixed() ? st->mapping_base[part[j]] : 0; }  // what member j's records add to their mapping index
    int64_t n_packets = 0, res_floats = 0, payload_bytes = 0;
    bool on_device = false;              // planned on the host, entropy-decoded on the device
    int decoded = 0;                     // members whose entropy decode is complete (under the group's mutex)
    bool prepped = false, prepping = false, synth_done = false;
};

// One device group's share of a vpzm_decode_library call.  A streaming pipeline, every stage on the group's own threads and all
// of them overlapped:
//   open      a container is walked and its three headers parsed (setup cache: vorbis_front.cpp) -- `threads` workers, in
//             stream order;
//   plan      when a WAVE of consecutive streams (4 sub-batches' worth) is open, its streams are grouped by setup header and
//             cut into sub-batches (streams of one setup share a decoder and ride in the same synth calls);
//   decode    the workers entropy-decode a sub-batch's streams, one stream each, straight into the page-locked arrays of the
//             sub-batch's SLOT (slots_per_device of them: sub-batch b takes slot b mod slots once sub-batch b - slots has been
//             synthesised) -- a worker with no decode work opens the next container instead, so the first synth call is under
//             way a few milliseconds into the job;
//   synth     `contexts_per_device` issuing threads take the decoded sub-batches in order, one host-memory vpz_decoder_synth call
//             each: the upload of one overlaps the download of the other's (SubCall below).
struct GroupRun {
    vpzm_dispatcher *m;
    Group &G;
    int slot_index;
    int32_t lo, hi;  // the group's streams [lo, hi)
    const uint8_t *const *data;
    const uint64_t *size;
    const vpzm_range *ranges;  // vpzm_decode_ranges: every stream's window (nullptr: vpzm_decode_library, whole streams)
    int32_t out_layout;
    void *pcm_out;
    const int64_t *pcm_offset, *pcm_capacity;
    vpzm_stream_result *results;
    int threads;
    const Switches sw;
    const bool mixed;  // the dispatcher's mixed_setups as the call found it, with gpu_entropy
    Batch batch{};     // (decode_call fills it in for a batch call)
    bool batched() const { return batch.dst != nullptr; }
    int64_t capacity_of(int32_t k) const { return batched() ? batch.frames : pcm_capacity[k]; }  // samples entry k may deliver
    int lane_host_threads = std::max(1, std::min(8, threads / std::max(1, (int)G.lanes.size())));  // vpz_decoder_set_host_threads of every lane's decoders: the device's threads / its contexts
    double t_wall = 0, t_decode = 0, t_synth = 0;
    int64_t device_streams = 0, device_payload = 0;  // streams entropy-decoded on the device, their packet bytes
    Clock::time_point t_begin = Clock::now();
    int64_t samples_total = 0;

    std::vector<Job> jobs;
    std::vector<std::shared_ptr<Setup>> setups;
    // mixed: the merged setups of this call; setups[q] is part merged_at[q].second of merged[merged_at[q].first] (-1: not looked up yet).
    // A merged setup only grows, as a copy with one more part: sub-batches cut before keep the one they were cut with
    std::vector<std::shared_ptr<Setup>> merged;
    std::vector<std::pair<int, int>> merged_at;
    int64_t n_device_subs = 0, n_mixed_subs = 0, most_setups = 0;  // vpzm_call_counts, this group's share (under `mu`)
    std::atomic<int64_t> decoders_created{0};
    std::deque<Sub> subs;                    // (a deque: sub-batches are appended while others are in flight)
    std::vector<std::pair<int, int>> tasks;  // (sub, member) in the order they are decoded
    std::vector<int> wave_left;              // streams of each wave still to be opened
    int waves_planned = 0;
    std::mutex mu;
    std::condition_variable cv;
    size_t next_open = 0, next_task = 0, next_synth = 0;

    int wave_size() const { return std::max(4 * m->opt.streams_per_call, 2 * m->device_streams_per_call); }
    bool all_planned() const { return waves_planned == (int)wave_left.size(); }
    Slot &slot_of(size_t b) { return G.slots[b % G.slots.size()]; }

    // ---- open: the container walked (pages, CRC, lacing), the three headers parsed, the setup products read out
    void open_one(size_t i)
    {
        Job &J = jobs[i];
        J.k = lo + (int32_t)i;
        vpzm_stream_result &R = results[J.k];
        R = vpzm_stream_result{};
        R.device_slot = slot_index;
        try {
            if (vpzh_open_memory(data[J.k], size[J.k], &J.h) != VPZH_OK) {
                J.status = VPZM_E_OPEN;
                J.close();
                return;
            }
            vpzh_info info{};
            vpzh_get_info(J.h, &info);
            J.packets = info.audio_packets;
            J.residue_floats = info.residue_floats;
            J.total_samples = vpzh_total_samples(J.h);
            R.channels = info.channels;
            R.sample_rate = info.sample_rate;
            R.packets = info.audio_packets;
            J.wanted = J.total_samples;
            if (ranges) {  // (the window rule is the front end's; a window outside the stream costs its entry alone)
                int64_t values = 0;
                if (vpzh_window(J.h, ranges[J.k].start, ranges[J.k].count, &J.first, &J.packets, &J.roll, &J.position, &J.wanted, &values) != VPZH_OK) {
                    J.status = VPZM_E_RANGE;
                    R.packets = 0;
                    return;
                }
                J.residue_floats = values;
                R.packets = J.packets;
            }
            if (batch.resampled()) {  // (the ratio first: the row's capacity is in output samples)
                if (!batch.downmix && info.channels != batch.channels) { J.status = VPZM_E_CHANNELS; return; }
                int64_t a = info.sample_rate, b = batch.rate;
                while (b) { const int64_t t = a % b; a = b; b = t; }
                const int64_t up = a > 0 ? batch.rate / a : 0, down = a > 0 ? info.sample_rate / a : 0;
                if (up < 1 || down < 1 || up > VPZ_RESAMPLE_MAX_UP || down > VPZ_RESAMPLE_MAX_DOWN_PER_UP * up) { J.status = VPZM_E_RATE; return; }
                J.up = (int32_t)up;
                J.down = (int32_t)down;
                if (batch.by_loudness() && (info.sample_rate < VPZ_LOUDNESS_MIN_RATE || info.sample_rate > VPZ_LOUDNESS_MAX_RATE)) { J.status = VPZM_E_RATE; return; }
                if (J.wanted > INT64_MAX / 2048 || resampled_length(J.wanted, J.up, J.down) > batch.frames) { J.status = VPZM_E_CAPACITY; return; }
            } else {
                if (J.wanted > capacity_of(J.k)) { J.status = VPZM_E_CAPACITY; return; }
                if (batched() && !batch.measured() && info.channels != batch.channels) { J.status = VPZM_E_CHANNELS; return; }
                if (batch.measured() && (info.sample_rate < VPZ_LOUDNESS_MIN_RATE || info.sample_rate > VPZ_LOUDNESS_MAX_RATE)) { J.status = VPZM_E_RATE; return; }
            }
            if (J.packets > 0) {
                J.own = std::make_shared<Setup>();
                if (!J.own->load(J.h, m->opt.gpu_entropy != 0)) J.status = VPZM_E_SETUP;
                // (the plan's sizes first, without a payload: members' payload bases are known when the sub-batch is cut)
                if (J.status == VPZM_OK && J.own->on_device() &&
                    vpzh_plan_range(J.h, J.first, J.packets, 0, 0, nullptr, nullptr, nullptr, 0, &J.payload_bytes, nullptr) != VPZH_OK)
                    J.own->image.clear();
            }
        } catch (...) {
            J.status = VPZM_E_OPEN;
        }
    }

    // ---- plan (under `mu`): the streams of one wave grouped by setup header, every group cut into sub-batches
    void plan_wave(int w)
    {
        const size_t a = (size_t)w * (size_t)wave_size(), b = std::min(jobs.size(), a + (size_t)wave_size());
        std::vector<std::vector<int>> by_setup(setups.size());
        for (size_t i = a; i < b; ++i) {
            Job &J = jobs[i];
            if (J.status != VPZM_OK || !J.h || J.packets == 0 || !J.own) {  // (no audio packets: 0 samples, nothing to do)
                ++skipped_streams;
                continue;
            }
            int at = -1;
            for (size_t q = 0; q < setups.size(); ++q)
                if (setups[q]->same(*J.own)) { at = (int)q; break; }
            if (at < 0) {
                at = (int)setups.size();
                setups.push_back(J.own);
                by_setup.emplace_back();
            }
            J.own.reset();
            by_setup[(size_t)at].push_back((int)i);
        }
        std::vector<Sub> fresh;
        std::vector<std::vector<int>> pool;  // mixed: the wave's streams of every merged setup, in job order
        for (size_t q = 0; q < by_setup.size(); ++q) {
            if (by_setup[q].empty()) continue;
            if (!mixed || !setups[q]->on_device()) {
                for (Sub &sb : cut(setups[q], by_setup[q])) fresh.push_back(std::move(sb));
                continue;
            }
            const std::pair<int, int> at = merge(q);
            pool.resize(merged.size());
            for (int i : by_setup[q]) {
                jobs[(size_t)i].part = at.second;
                pool[(size_t)at.first].push_back(i);
            }
        }
        for (size_t g = 0; g < pool.size(); ++g) {
            std::sort(pool[g].begin(), pool[g].end());
            for (Sub &sb : cut(merged[g], pool[g])) fresh.push_back(std::move(sb));
        }
        for (const Sub &sb : fresh) {
            std::vector<uint8_t> seen = sb.part;
            std::sort(seen.begin(), seen.end());
            const int64_t n_setups = sb.mixed() ? std::unique(seen.begin(), seen.end()) - seen.begin() : 1;
            n_mixed_subs += n_setups > 1;
            most_setups = std::max(most_setups, n_setups);
        }
        std::sort(fresh.begin(), fresh.end(), [](const Sub &x, const Sub &y) { return x.members[0] < y.members[0]; });
        for (Sub &sb : fresh) {
            const int bi = (int)subs.size();
            for (size_t j = 0; j < sb.members.size(); ++j) tasks.emplace_back(bi, (int)j);
            subs.push_back(std::move(sb));
        }
        ++waves_planned;
    }

    // mixed: where setups[q] lies in the call's merged setups.  It joins the last merged setup of its class, which grows by it; when
    // that one is full (Setup::fits: mappings, floors, parts), or there is none, it starts another
    std::pair<int, int> merge(size_t q)
    {
        merged_at.resize(setups.size(), {-1, -1});
        if (merged_at[q].first >= 0) return merged_at[q];
        int last = -1;
        for (size_t g = 0; g < merged.size(); ++g)
            if (merged[g]->same_class(*setups[q])) last = (int)g;
        const bool grows = last >= 0 && merged[(size_t)last]->fits(*setups[q], (size_t)sw.max_merged_mappings);
        auto grown = grows ? std::make_shared<Setup>(*merged[(size_t)last]) : std::make_shared<Setup>();
        grown->add_part(setups[q]);
        if (grows) {
            merged[(size_t)last] = grown;
        } else {
            merged.push_back(grown);
            last = (int)merged.size() - 1;
        }
        return merged_at[q] = {last, (int)grown->parts.size() - 1};
    }

    // The cutting rule: the streams `v` of one setup (mixed: of one merged setup), in order, become sub-batches.  A synth call holds up to streams_per_call streams
    // and up to kCallValues residue values (a library of whole songs would otherwise ask for page-locked slots of gigabytes each):
    // a long stream rides with fewer others, or alone
    std::vector<Sub> cut(const std::shared_ptr<Setup> &st, const std::vector<int> &v) const
    {
        // (device-resident inputs are not bound by a page-locked slot's size, and one lane per packet wants many packets)
        const int limit = st->on_device() ? m->device_streams_per_call : m->opt.streams_per_call;
        std::vector<Sub> out;
        for (int i : v) {
            const Job &J = jobs[(size_t)i];
            if (out.empty() || (int)out.back().members.size() >= limit || out.back().res_floats + J.residue_floats > sw.max_call_values) {
                out.emplace_back();
                out.back().st = st;
                out.back().on_device = st->on_device();
            }
            Sub &sb = out.back();
            sb.members.push_back(i);
            sb.pbase.push_back(sb.n_packets);
            sb.rbase.push_back(sb.res_floats);
            sb.ybase.push_back(sb.payload_bytes);
            sb.n_packets += J.packets;
            sb.res_floats += J.residue_floats;
            sb.payload_bytes += (J.payload_bytes + 7) & ~(int64_t)7;
            if (!st->parts.empty()) sb.part.push_back((uint8_t)J.part);
        }
        // (a merged setup's sub-batch whose members all share one setup takes that setup's route: single image, vpz_entropy_decode)
        for (Sub &sb : out)
            if (sb.mixed() && std::count(sb.part.begin(), sb.part.end(), sb.part[0]) == (std::ptrdiff_t)sb.part.size()) {
                sb.st = st->parts[sb.part[0]];
                sb.part.clear();
            }
        return out;
    }

    // the residue of a sub-batch travels as int16 when its setup header guarantees integers (and the caller has not asked for floats)
    bool use_i16(const Setup &st) const { return st.integral && !m->opt.float_residue; }

    // (the functions below run with `mu` RELEASED: they get their sub-batch by reference -- a deque's elements stay where they are, but
    // indexing `subs` / `setups` while plan_wave appends to them is a race)
    bool prepare(size_t b, Sub &sb)  // (one thread prepares a given sub-batch, before any of its members is decoded)
    {
        Slot &sl = slot_of(b);
        const Setup &st = *sb.st;
        const size_t n = (size_t)sb.n_packets, rec = n * (size_t)st.info.channels;
        auto room = [&](int which, size_t need, size_t elem) { return sl.buf[which].grow(G.lanes[0].ctx, need, elem); };
        // (the residue array is counted in floats: int16 values take half the elements)
        const size_t res_elems = use_i16(st) ? ((size_t)sb.res_floats + 1) / 2 : (size_t)sb.res_floats;
        bool ok = room(Slot::kPackets, n, sizeof(vpz_packet));
        if (sb.on_device)  // (no residue, posts or counts on the host: those arrays are born on the device)
            ok = ok && room(Slot::kSpans, n, sizeof(vpz_entropy_span)) && room(Slot::kPayload, (size_t)sb.payload_bytes, 1);
        else
            ok = ok && room(Slot::kResidue, res_elems, sizeof(float)) && room(Slot::kPosts, rec * 64, sizeof(int16_t)) && room(Slot::kCounts, rec, 1);
        if (ok && !sb.on_device && st.f0_stride > 0)
            ok = room(Slot::kF0Amp, rec, sizeof(float)) && room(Slot::kF0Coeff, rec * (size_t)st.f0_stride, sizeof(float));
        if (!ok) fail_members(sb, VPZM_E_SYNTH, "vpzm_decode_library: page-locked batch arrays could not be allocated");
        return ok;
    }
    // a sub-batch that cannot go on: its members fail with `status` -- those that have a failure status of their own keep it
    void fail_members(const Sub &sb, int32_t status, const char *text)
    {
        for (int mi : sb.members)
            if (jobs[(size_t)mi].status == VPZM_OK) jobs[(size_t)mi].status = status;
        m->fail(text);
    }

    // A mixed sub-batch's records carry mapping indices of its merged setup: every record of member j, the not-decoded ones included (an
    // index valid in its own setup stays valid in the merged one), moves by the base of the member's part
    static void shift_mappings(vpz_packet *pk, int64_t n, int by)
    {
        if (by)
            for (int64_t p = 0; p < n; ++p) pk[p].mapping = (uint8_t)(pk[p].mapping + by);
    }

    // the plan of one member of a device-decoded sub-batch: packet records, spans and the packets' bytes into the slot
    int plan_member(Job &J, Slot &sl, const Sub &sb, int j)
    {
        const int64_t pb = sb.pbase[(size_t)j], yb = sb.ybase[(size_t)j];
        const int rc = vpzh_plan_range(J.h, J.first, J.packets, j, sb.rbase[(size_t)j], sl.packets() + pb, sl.spans() + pb, sl.payload() + yb,
                                       J.payload_bytes, nullptr, nullptr);
        if (rc != VPZH_OK) return rc;
        for (int64_t p = 0; p < J.packets; ++p) sl.spans()[pb + p].offset += yb;  // (spans count from the sub-batch's payload)
        shift_mappings(sl.packets() + pb, J.packets, sb.mapping_shift((size_t)j));
        J.plan_failures = vpzh_decode_failures(J.h, nullptr);
        return rc;
    }
    // ... and the entropy decode of one member of a host-decoded one: records, residue, posts, counts and Floor0 data into the slot
    int decode_member_on_host(Job &J, Slot &sl, const Sub &sb, int j)
    {
        const Setup &st = *sb.st;
        const size_t C = (size_t)st.info.channels;
        const int64_t pb = sb.pbase[(size_t)j], rb = sb.rbase[(size_t)j];
        float *amp_at = st.f0_stride ? sl.f0_amp() + (size_t)pb * C : nullptr;
        float *coeff_at = st.f0_stride ? sl.f0_coeff() + (size_t)pb * C * (size_t)st.f0_stride : nullptr;
        const int rc = use_i16(st) ? vpzh_decode_range_i16(J.h, J.first, J.packets, j, rb, sl.packets() + pb, sl.residue_i16() + rb, sl.posts() + (size_t)pb * 64 * C,
                                                           sl.counts() + (size_t)pb * C, nullptr, amp_at, coeff_at, st.f0_stride)
                                   : vpzh_decode_range_ex(J.h, J.first, J.packets, j, rb, sl.packets() + pb, sl.residue_f32() + rb, sl.posts() + (size_t)pb * 64 * C,
                                                          sl.counts() + (size_t)pb * C, nullptr, amp_at, coeff_at, st.f0_stride);
        if (rc == VPZH_OK) results[J.k].skipped_packets += vpzh_decode_failures(J.h, nullptr);
        if (rc == VPZH_OK) shift_mappings(sl.packets() + pb, J.packets, sb.mapping_shift((size_t)j));  // (the stream's own handle decoded it from its own setup)
        return rc;
    }
    // one member's decode task.  A container that does not decode costs its stream (VPZM_E_OPEN).  A planned member's container stays
    // open until the sub-batch has been issued (should the device refuse it, its members are decoded here after all); a decoded one's goes
    void decode_member(size_t b, Sub &sb, int j)
    {
        Job &J = jobs[(size_t)sb.members[(size_t)j]];
        if (J.status == VPZM_OK) {
            int rc = VPZH_E_ARG;
            try {
                rc = sb.on_device ? plan_member(J, slot_of(b), sb, j) : decode_member_on_host(J, slot_of(b), sb, j);
            } catch (...) {
                rc = VPZH_E_INVALID_DATA;
            }
            if (rc != VPZH_OK) J.status = VPZM_E_OPEN;
        }
        if (!sb.on_device) J.close();
    }

    // a whole sub-batch on the calling thread (a sub-batch the device did not take, the run without threads): the arrays, then every member
    void decode_sub(size_t b, Sub &sb)
    {
        if (!prepare(b, sb)) return;
        for (size_t j = 0; j < sb.members.size(); ++j) decode_member(b, sb, (int)j);
    }

    // ---- the workers: decode what can be decoded, else open the next container, else wait
    void worker()
    {
        const size_t B = G.slots.size();
        // containers open but not yet decoded hold their packets in memory: no more than a few waves ahead
        const size_t open_ahead = (size_t)wave_size() * 3;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            if (aborted) return;
            if (next_task < tasks.size()) {
                const size_t b = (size_t)tasks[next_task].first;
                Sub &sb = subs[b];
                if (sb.prepped) {
                    const int j = tasks[next_task++].second;
                    lk.unlock();
                    decode_member(b, sb, j);
                    lk.lock();
                    if (++sb.decoded == (int)sb.members.size()) {
                        if (sw.profile && sb.on_device)
                            fprintf(stderr, "[vpzm] group %d: sub-batch %zu planned at %.2f ms\n", slot_index, b, seconds_since(t_begin) * 1e3);
                        cv.notify_all();
                    }
                    continue;
                }
                if (!sb.prepping && (b < B || subs[b - B].synth_done)) {  // its slot is free: get the arrays ready
                    sb.prepping = true;
                    lk.unlock();
                    (void)prepare(b, sb);  // (without arrays its members have their status: decode_member passes them by)
                    lk.lock();
                    sb.prepped = true;
                    cv.notify_all();
                    continue;
                }
            }
            const size_t undecoded = next_open - std::min(next_open, done_decoding());
            if (next_open < jobs.size() && undecoded < open_ahead + (size_t)threads) {
                const size_t i = next_open++;
                lk.unlock();
                open_one(i);
                lk.lock();
                const int w = (int)(i / (size_t)wave_size());
                if (--wave_left[(size_t)w] == 0) {
                    plan_wave(w);
                    cv.notify_all();
                }
                continue;
            }
            if (all_planned() && next_task >= tasks.size()) {
                t_decode = std::max(t_decode, seconds_since(t_begin));
                return;
            }
            cv.wait(lk);
        }
    }
    // streams whose decode task has been handed out (under `mu`): what the open-ahead limit is measured against
    size_t done_decoding() const { return std::min(next_task + skipped_streams, jobs.size()); }
    size_t skipped_streams = 0;  // (streams that never become a decode task: failed to open, no packets, area too small)
    // An exception on one of the run's threads (std::bad_alloc out of a vector in plan_wave / synth_sub, ...) must neither leave
    // the thread (std::terminate inside a C ABI that promises statuses) nor leave the others waiting for a counter that will never
    // move: the run is ABORTED -- every loop looks at the flag --, and the streams without a result get VPZM_E_SYNTH
    bool aborted = false;  // (under `mu`)
    void abort_run(const char *what) noexcept
    {
        try {
            std::lock_guard<std::mutex> lk(mu);
            aborted = true;
        } catch (...) {
        }
        try {
            m->fail(what);
        } catch (...) {
        }
        cv.notify_all();
    }
    template <class F>
    void guarded(F &&body) noexcept
    {
        try {
            body();
        } catch (const std::bad_alloc &) {
            abort_run("vpzm_decode_library: out of host memory on a pipeline thread");
        } catch (...) {
            abort_run("vpzm_decode_library: a pipeline thread failed");
        }
    }

    vpz_decoder *decoder_for(Lane &L, const std::shared_ptr<Setup> &st)
    {
        if (vpz_decoder *dec = L.decoders.find(*st)) return dec;
        vpz_stream_config cfg{};
        cfg.channels = st->info.channels;
        cfg.block_size0 = st->info.block_size0;
        cfg.block_size1 = st->info.block_size1;
        cfg.floor_count = (int32_t)st->floors.size();
        cfg.floors = st->floors.data();
        cfg.mapping_count = (int32_t)st->mappings.size();
        cfg.mappings = st->mappings.data();
        cfg.clip_samples = m->opt.clip_samples;
        cfg.floor_types = st->floor_types.data();
        cfg.floors0 = st->floors0.data();
        vpz_decoder *dec = nullptr;
        ++decoders_created;
        if (vpz_decoder_create(L.ctx, &cfg, m->call_streams(), &dec) != VPZ_OK) {
            m->fail(std::string("vpz_decoder_create: ") + vpz_context_last_error(L.ctx));
            return nullptr;
        }
        // The integer half of a synth call may fork over a pool of the decoder's context (batches of whole songs do): every lane its
        // share of the device's host threads, not a pool for the whole machine each -- the decode workers need the CPUs
        (void)vpz_decoder_set_host_threads(dec, lane_host_threads);
        L.decoders.keep(st, dec);
        return dec;
    }

    // ---- synth: one issuing thread per context takes the decoded sub-batches in order
    void issuer(Lane &L)
    {
        for (;;) {
            size_t b;
            Sub *sp = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (aborted) return;
                    if (next_synth < subs.size()) break;
                    if (all_planned()) return;
                    cv.wait(lk);
                }
                b = next_synth++;
                cv.wait(lk, [&] { return aborted || subs[b].decoded == (int)subs[b].members.size(); });
                if (aborted) return;
                sp = &subs[b];
            }
            synth_sub(L, b, *sp);
        }
    }
    void synth_sub(Lane &L, size_t b, Sub &sb);  // (SubCall's stages, below)

    // A batch call, the run's threads joined: the rows no sub-batch's pack has defined become zeros in ONE launch of samples = 0
    // descriptors on the group's first lane -- entries that never reached a sub-batch (open failure, range, capacity, channel count, an
    // empty window) and whatever a failed pack or an aborted run left -- and the lanes' streams drain.  Without it (no memory for the
    // descriptors, a failed launch) the entries concerned say so: VPZM_E_SYNTH
    void zero_rows() noexcept
    {
        bool ok = true;
        try {
            std::vector<vpz_pack_row> rows;
            for (const Job &J : jobs)
                if (!J.row_packed) rows.push_back(vpz_pack_row{0, 0, (int64_t)(&J - jobs.data())});
            if (batch.measured()) rows.clear();  // (a loudness call's records are the caller's and hold the empty record already)
            if (!rows.empty()) ok = batch.empty_rows(G.lanes[0], rows) == VPZ_OK;
            if (!ok) m->fail(std::string(batch.empty_step()) + " (" + batch.empty_words() + "): " + vpz_context_last_error(G.lanes[0].ctx));
        } catch (...) {
            ok = false;
        }
        for (Lane &L : G.lanes) ok = vpz_context_synchronize(L.ctx) == VPZ_OK && ok;
        for (size_t i = 0; !ok && i < jobs.size(); ++i)
            if (!jobs[i].row_packed && jobs[i].status == VPZM_OK) {
                jobs[i].status = VPZM_E_SYNTH;
                results[lo + (int32_t)i].samples = 0;
            }
    }

    // run() for a thread of its own: whatever it throws before its pipeline stands (the job table's allocation) becomes the
    // statuses of the group's streams, never an exception out of the thread
    void run_guarded() noexcept
    {
        try {
            run();
        } catch (...) {
            for (int32_t k = lo; k < hi; ++k) {
                results[k] = vpzm_stream_result{};
                results[k].device_slot = slot_index;
                results[k].status = VPZM_E_SYNTH;
            }
            try {
                m->fail("vpzm_decode_library: a device group could not set its pipeline up (out of host memory)");
            } catch (...) {
            }
        }
    }

    void run()
    {
        t_begin = Clock::now();
        jobs.resize((size_t)(hi - lo));
        const size_t W = (size_t)wave_size();
        wave_left.assign((jobs.size() + W - 1) / W, 0);
        for (size_t w = 0; w < wave_left.size(); ++w) wave_left[w] = (int)(std::min(jobs.size(), (w + 1) * W) - w * W);
        std::vector<std::thread> pool;
        int workers = 0;
        try {
            for (int t = 0; t < threads; ++t) {
                pool.emplace_back([this] { guarded([this] { worker(); }); });
                ++workers;
            }
        } catch (...) {
        }
        if (workers == 0) {
            // no thread could be started: the stages in order on this one, a sub-batch at a time
            guarded([this] {
                for (size_t i = 0; i < jobs.size(); ++i) open_one(i);
                for (int w = 0; w < (int)wave_left.size(); ++w) plan_wave(w);
                for (size_t b = 0; b < subs.size(); ++b) {
                    decode_sub(b, subs[b]);
                    subs[b].decoded = (int)subs[b].members.size();
                    synth_sub(G.lanes[0], b, subs[b]);
                }
            });
            t_decode = seconds_since(t_begin);
        } else {
            try {
                for (size_t l = 1; l < G.lanes.size(); ++l) pool.emplace_back([this, l] { guarded([this, l] { issuer(G.lanes[l]); }); });
            } catch (...) {  // (fewer issuing threads: this thread's one drains every sub-batch)
            }
            guarded([this] { issuer(G.lanes[0]); });
        }
        for (std::thread &t : pool) t.join();
        if (batched()) zero_rows();
        for (Job &J : jobs) {
            J.close();
            if (aborted && J.status == VPZM_OK && !J.finished) {  // (an aborted run: no PCM, no count -- the stream has no result)
                J.status = VPZM_E_SYNTH;
                results[J.k].samples = 0;
            }
            results[J.k].status = J.status;
        }
        t_wall = seconds_since(t_begin);
    }
};

// One sub-batch's synth step on its issuing thread, stage by stage (GroupRun::synth_sub runs them; the model is SynthCall in
// vpz_decoder.hip).  Two routes: a host-decoded sub-batch's arrays lie in its slot and its PCM goes straight into the caller's array;
// a device-decoded one's packet bytes go up, vpz_entropy_decode writes the lane's device arrays, the synth call reads those and writes
// the lane's device PCM array, and every member's PCM comes down.  `sb.on_device` says which; decode_on_device may clear it.
// A ranges call (`ranged`) stages the PCM on both routes; `download` brings every member's window from there to the caller's area
// (copy_down) or into its row of the caller's device tensor (deliver_batch).
struct SubCall {
    GroupRun &R;
    Lane &L;
    const size_t b;
    Sub &sb;
    Slot &sl = R.slot_of(b);
    const Setup &st = *sb.st;
    const int C = st.info.channels, S = R.m->call_streams();  // channels; the streams a decoder is created for
    const size_t elem = R.out_layout == VPZ_OUT_INTERLEAVED_S16 ? sizeof(int16_t) : sizeof(float);  // bytes of a PCM sample
    const bool ranged = R.ranges != nullptr;  // a vpzm_decode_ranges call: staged PCM on both routes, windows trimmed in `download`
    const bool batched = R.batched();         // ... a vpzm_decode_ranges_batch call: staged in the lane's device array on both routes, packed in `download`
    const Batch &B = R.batch;                 // ... its kind, shape and destination
    bool inputs_on_device = false;            // the synth call reads the lane's device arrays (decode_on_device, upload_decoded) and is a VPZ_MEM_DEVICE call
    bool any = false;  // ---- repack: a member is left ...
    int64_t n_pk = 0;  // ... and the packets of those that are
    // ---- place_outputs: every member's area (offset and capacity in samples), where the areas start, the largest capacity, all the areas
    std::vector<int64_t> offs = std::vector<int64_t>((size_t)S), caps = offs;
    void *out_at = nullptr;
    int64_t cap = 0, pcm_elems = 0;
    // ---- the calls: samples of every member (of the calls that stand, of the last call), every member's own status
    vpz_decoder *dec = nullptr;
    std::vector<int64_t> written = offs, wr = offs;
    std::vector<int> member_rc = std::vector<int>(sb.members.size(), VPZ_OK);  // (a sub-batch is one synth call; after a failed one, a call per member)
    Clock::time_point t0 = Clock::now();
    double t_upload = 0, t_entropy = 0, t_call = 0, t_download = 0;
    int member_calls = 0;  // synth calls made for single members after the batch call failed (the profile line says how many)
    int resample_launches = 0;  // a resampled call: vpz_pcm_resample launches of this sub-batch, one per ratio among its members
    // a normalised call, per member: the loudness mode's measurement and the gain it gives; the stage's result records on their way down
    std::vector<double> norm_loud, norm_gain;
    std::vector<vpz_norm_result> norm_down;

    Job &job(size_t j) const { return R.jobs[(size_t)sb.members[j]]; }
    bool live(size_t j) const { return job(j).status == VPZM_OK; }
    bool has_call() const { return any && n_pk > 0; }

    // a member whose container did not decode leaves its packets out (rare): the arrays are re-packed stream by stream,
    // stream ids kept, so that vpz_decoder_synth sees only decoded packets; their residue stays where it is
    void repack()
    {
        bool all_ok = true;
        any = false;
        for (size_t j = 0; j < sb.members.size(); ++j) {
            if (live(j)) any = true;
            else all_ok = false;
        }
        n_pk = sb.n_packets;
        if (!any || all_ok) return;
        int64_t w = 0;
        for (size_t j = 0; j < sb.members.size(); ++j) {
            const Job &J = job(j);
            if (J.status != VPZM_OK) continue;
            const int64_t pb = sb.pbase[j];
            if (w != pb) {
                memmove(sl.packets() + w, sl.packets() + pb, sizeof(vpz_packet) * (size_t)J.packets);
                if (sb.on_device) {  // (the device arrays are written for the packets as they lie now)
                    memmove(sl.spans() + w, sl.spans() + pb, sizeof(vpz_entropy_span) * (size_t)J.packets);
                } else {
                    memmove(sl.posts() + (size_t)w * 64 * C, sl.posts() + (size_t)pb * 64 * C, sizeof(int16_t) * 64 * (size_t)C * (size_t)J.packets);
                    memmove(sl.counts() + (size_t)w * C, sl.counts() + (size_t)pb * C, (size_t)C * (size_t)J.packets);
                    if (st.f0_stride) {
                        memmove(sl.f0_amp() + (size_t)w * C, sl.f0_amp() + (size_t)pb * C, sizeof(float) * (size_t)C * (size_t)J.packets);
                        memmove(sl.f0_coeff() + (size_t)w * C * st.f0_stride, sl.f0_coeff() + (size_t)pb * C * st.f0_stride,
                                sizeof(float) * (size_t)C * st.f0_stride * (size_t)J.packets);
                    }
                }
            }
            w += J.packets;
        }
        n_pk = w;
    }

    // Every stream has its own area (files of one encoder setting share a setup header and differ in length).  Host route: a host-memory
    // call sees the sub-batch's part of the caller's PCM array (it mirrors its output extent on the device), so the offsets handed over
    // start at the sub-batch's lowest one, and a capacity is the caller's.  Device route: the areas lie back to back in the lane's device PCM
    // array; a stream produces at most block_size1 / 2 samples per packet, so an area need not be larger than that, plus one block of slack.
    // A ranges call stages its PCM on both routes, by the device route's rule: the areas back to back in the lane's device array or in
    // the slot's page-locked stage, `packets * block_size1 / 2` samples and a block of slack each -- a window's packets give up to a
    // packet of samples more than the caller wants, in front (Job::roll) and behind, so no area of the caller's could take them.
    void place_outputs()
    {
        const bool dev = sb.on_device || ranged;  // (the areas are the call's own, not the caller's)
        int64_t base = INT64_MAX, dev_at = 0;
        for (size_t j = 0; !dev && j < sb.members.size(); ++j) base = std::min(base, R.pcm_offset[job(j).k]);
        cap = 0;
        for (size_t j = 0; j < sb.members.size(); ++j) {
            const Job &J = job(j);
            offs[j] = dev ? dev_at : R.pcm_offset[J.k] - base;
            caps[j] = 0;
            if (J.status != VPZM_OK) continue;
            caps[j] = ranged ? J.packets * (st.info.block_size1 / 2)
                      : dev  ? std::min(R.pcm_capacity[J.k], J.packets * (st.info.block_size1 / 2))
                             : R.pcm_capacity[J.k];
            if (dev) dev_at += (caps[j] + st.info.block_size1) * C;
            cap = std::max(cap, caps[j]);
        }
        pcm_elems = dev_at;
        out_at = dev ? nullptr : static_cast<char *>(R.pcm_out) + elem * (size_t)base;  // (the lane's array: once decode_on_device has grown it)
        if (ranged && !batched && !sb.on_device && has_call()) {  // (host route of a ranges call: the slot's stage; without it the members fail like a slot without arrays)
            if (sl.buf[Slot::kStage].grow(R.G.lanes[0].ctx, (size_t)pcm_elems, elem)) out_at = sl.stage();
            else R.fail_members(sb, VPZM_E_SYNTH, "vpzm_decode_ranges: the page-locked PCM stage could not be allocated");
        }
    }

    // A device-decoded sub-batch's first two steps on the lane's stream: the packet bytes go up, vpz_entropy_decode writes residue,
    // posts and counts into the lane's device arrays (asynchronous: the synth call that follows on the same stream consumes them without
    // a synchronise).  false: the device path is not to be had for this sub-batch (no memory, an image the library refuses, a failed
    // call) -- nothing of the job has changed, the sub-batch takes the host path
    bool decode_on_device()
    {
        if (R.sw.fail_gpu_entropy) return false;
        const bool i16 = R.use_i16(st);
        const size_t rec = (size_t)n_pk * (size_t)C;
        auto room = [&](int which, size_t bytes) { return L.buf[which].grow(L.ctx, bytes, 1); };
        if (!room(Lane::kPayload, (size_t)sb.payload_bytes) || !room(Lane::kResidue, (size_t)sb.res_floats * (i16 ? sizeof(int16_t) : sizeof(float))) ||
            !room(Lane::kPosts, rec * 64 * sizeof(int16_t)) || !room(Lane::kCounts, rec) || !room(Lane::kPcm, (size_t)pcm_elems * elem))
            return false;
        vpz_entropy_setup *es = sb.mixed() ? nullptr : L.esetups.find(st);
        if (!sb.mixed() && !es) {
            if (vpz_entropy_setup_create(L.ctx, st.image.data(), (uint64_t)st.image.size(), &es) != VPZ_OK) return false;  // (refused: the host path)
            L.esetups.keep(sb.st, es);
        }
        vpz_entropy_group *eg = sb.mixed() ? L.egroups.find(st) : nullptr;
        if (sb.mixed() && !eg) {  // (the merged setup's parts in order: a member's part is its setup in the group)
            std::vector<const void *> images;
            std::vector<uint64_t> sizes;
            for (const auto &part : st.parts) {
                images.push_back(part->image.data());
                sizes.push_back((uint64_t)part->image.size());
            }
            if (vpz_entropy_group_create(L.ctx, images.data(), sizes.data(), (int32_t)images.size(), &eg) != VPZ_OK) return false;
            L.egroups.keep(sb.st, eg);
        }
        std::vector<uint8_t> bases;  // (a mixed sub-batch: the member index is the stream, its part the stream's setup)
        for (size_t j = 0; j < sb.part.size(); ++j) bases.push_back((uint8_t)sb.mapping_shift(j));
        const auto t_up = Clock::now();
        if (vpz_memcpy_h2d(L.ctx, L.payload(), sl.payload(), (uint64_t)sb.payload_bytes) != VPZ_OK) return false;
        t_upload = seconds_since(t_up);
        const auto t_en = Clock::now();
        const int32_t format = i16 ? VPZ_RESIDUE_I16 : VPZ_RESIDUE_F32;
        const int rc = sb.mixed() ? vpz_entropy_group_decode(eg, (int32_t)sb.part.size(), sb.part.data(), bases.data(), n_pk, sl.packets(), sl.spans(),
                                                             L.payload(), sb.payload_bytes, format, L.residue(), sb.res_floats, L.posts(),
                                                             L.counts(), (int64_t)rec, VPZ_MEM_DEVICE)
                                  : vpz_entropy_decode(es, n_pk, sl.packets(), sl.spans(), L.payload(), sb.payload_bytes, format, L.residue(),
                                                       sb.res_floats, L.posts(), L.counts(), (int64_t)rec, VPZ_MEM_DEVICE);
        if (rc != VPZ_OK) return false;
        if (R.sw.profile) (void)vpz_context_synchronize(L.ctx);  // (the timeline wants the stage's own time; otherwise nothing waits here)
        t_entropy = seconds_since(t_en);
        out_at = L.pcm();
        inputs_on_device = true;
        return true;
    }

    // A batch call's host route brings no PCM down, so its synth call is a device-memory one like the device route's: the slot's decoded
    // arrays -- residue, posts, counts, a type-0 floor's amp and coefficients -- go up into the lane's device arrays (vpz_memcpy_h2d: the
    // slot is free again when it returns) and the PCM areas lie in the lane's device PCM array.  Without the memory or a copy the members
    // fail like a slot without arrays
    void upload_decoded()
    {
        const bool i16 = R.use_i16(st);
        const size_t rec = (size_t)sb.n_packets * (size_t)C;  // (the slot's arrays as they lie: a re-packed sub-batch's calls index them by packet)
        const size_t res_bytes = (size_t)sb.res_floats * (i16 ? sizeof(int16_t) : sizeof(float)), f0 = (size_t)st.f0_stride;
        auto up = [&](int which, const void *from, size_t bytes) {
            return bytes == 0 || (L.buf[which].grow(L.ctx, bytes, 1) && vpz_memcpy_h2d(L.ctx, L.buf[which].p, from, (uint64_t)bytes) == VPZ_OK);
        };
        const auto t_up = Clock::now();
        bool ok = up(Lane::kResidue, sl.residue_f32(), res_bytes) && up(Lane::kPosts, sl.posts(), rec * 64 * sizeof(int16_t)) &&
                  up(Lane::kCounts, sl.counts(), rec) && L.buf[Lane::kPcm].grow(L.ctx, (size_t)pcm_elems, elem);
        if (ok && f0 > 0) ok = up(Lane::kF0Amp, sl.f0_amp(), rec * sizeof(float)) && up(Lane::kF0Coeff, sl.f0_coeff(), rec * f0 * sizeof(float));
        t_upload += seconds_since(t_up);
        if (!ok) {
            R.fail_members(sb, VPZM_E_SYNTH, "vpzm_decode_ranges_batch: the decoded arrays of a sub-batch could not be uploaded");
            return;
        }
        out_at = L.pcm();
        inputs_on_device = true;
    }

    // the host path after all: the slot gets the host arrays, this thread decodes the members (their containers are still open), and
    // the sub-batch is packed and placed again as the host-decoded one it now is
    void decode_on_host()
    {
        sb.on_device = false;
        R.decode_sub(b, sb);
        repack();
        place_outputs();
    }

    // one synth call over the slot's packets [p0, p0 + n): the records, the Floor0 data and the statuses move with p0, the
    // residue offsets are the slot's.  A device-decoded sub-batch's call reads the lane's device arrays, laid out the same way
    int call(int64_t p0, int64_t n)
    {
        const bool dev = inputs_on_device;
        const int16_t *posts = dev ? L.posts() : sl.posts();
        const uint8_t *counts = dev ? L.counts() : sl.counts();
        // the decoder is re-used for new streams: back to what a StreamDecoder is after ProcessHeaderPackets
        // (`_currentPosition = 0; _hasPosition = true`, StreamDecoder.cs:165-168) -- a bare reset would leave the position to be
        // picked up from the first granule the way a seek does (:459-463), which moves the EOS trim (:658-666)
        int r = vpz_decoder_reset(dec, -1);
        // -- every member's stream at the position its window starts from (Job::position: 0 for a whole stream)
        for (int sidx = 0; sidx < S && r == VPZ_OK; ++sidx)
            r = vpz_decoder_set_position(dec, sidx, (size_t)sidx < sb.members.size() ? job((size_t)sidx).position : 0);
        if (r == VPZ_OK && st.f0_stride > 0)
            r = vpz_decoder_set_floor0_data(dec, (dev ? L.f0_amp() : sl.f0_amp()) + (size_t)p0 * C,
                                            (dev ? L.f0_coeff() : sl.f0_coeff()) + (size_t)p0 * C * st.f0_stride, st.f0_stride);
        if (r == VPZ_OK) r = vpz_decoder_set_residue_format(dec, R.use_i16(st) ? VPZ_RESIDUE_I16 : VPZ_RESIDUE_F32);
        if (r == VPZ_OK) r = vpz_decoder_set_stream_capacities(dec, caps.data(), S);
        if (r == VPZ_OK)
            r = vpz_decoder_synth(dec, n, sl.packets() + p0, dev ? L.residue() : sl.residue_f32(), sb.res_floats, posts + (size_t)p0 * 64 * C,
                                  counts + (size_t)p0 * C, n * C, dev ? VPZ_MEM_DEVICE : VPZ_MEM_HOST, out_at, offs.data(), cap, R.out_layout, 0,
                                  wr.data());
        if (r != VPZ_OK) R.m->fail(std::string("vpz_decoder_synth: ") + vpz_context_last_error(L.ctx));
        int64_t not_ok = 0;
        if (r == VPZ_OK && vpz_decoder_last_packet_status(dec, nullptr, 0, &not_ok) == VPZ_OK && not_ok > 0) {
            std::vector<int32_t> status((size_t)n, 0);
            vpz_decoder_last_packet_status(dec, status.data(), n, nullptr);
            for (int64_t p = 0; p < n; ++p)
                if (status[(size_t)p] != VPZ_OK) {
                    const int32_t sid = sl.packets()[p0 + p].stream;
                    if (sid >= 0 && (size_t)sid < sb.members.size()) R.results[job((size_t)sid).k].skipped_packets += 1;
                }
        }
        return r;
    }

    // the sub-batch as ONE synth call
    void call_batch()
    {
        if (!has_call() || R.sw.no_synth || !out_at) return;  // (no out_at: a ranges call whose stage could not be had; its members have their status)
        dec = R.decoder_for(L, sb.st);
        const int rc = !dec ? kNoDecoder : R.sw.fail_batch_calls ? VPZ_E_CAPACITY : call(0, n_pk);
        if (rc == VPZ_OK) written = wr;
        else if (rc == kNoDecoder) std::fill(member_rc.begin(), member_rc.end(), kNoDecoder);  // (vpz_decoder_create's text is in vpzm_last_error)
        else call_members(rc);
    }

    // "a stream that fails costs only itself": whatever one member's packets did to the call, the others get a call
    // of their own (the packets lie member by member; a device-decoded sub-batch's arrays are not decoded again)
    void call_members(int batch_rc)
    {
        const vpz_packet *packets = sl.packets();
        for (int64_t p = 0; p < n_pk;) {
            const int32_t sid = packets[p].stream;
            int64_t q = p;
            while (q < n_pk && packets[q].stream == sid) ++q;
            if (sid >= 0 && (size_t)sid < sb.members.size()) {
                const bool again = q - p != n_pk || R.sw.fail_batch_calls;  // (a member that WAS the batch has had its call)
                member_rc[(size_t)sid] = again ? call(p, q - p) : batch_rc;
                member_calls += again;
                if (member_rc[(size_t)sid] == VPZ_OK) written[(size_t)sid] = wr[(size_t)sid];
            }
            p = q;
        }
    }

    // Every member's PCM from where the call left it to where the caller wants it: copy_down for a library or a ranges call,
    // deliver_batch for a batch call
    void download()
    {
        const bool dev = (sb.on_device || batched) && has_call();
        if (dev && R.sw.profile) (void)vpz_context_synchronize(L.ctx);  // (the timeline wants the call's own time)
        t_call = seconds_since(t0) - t_upload - t_entropy;
        if (!dev && !ranged) return;
        const auto t_down = Clock::now();
        if (batched) deliver_batch();
        else copy_down(dev);
        t_download = seconds_since(t_down);
    }

    // One copy per member that has samples.  A library call has something to copy on the device route only (the areas in the lane's
    // array have a block of slack between them, the caller's areas whatever the caller likes): what samples_written says and no more, a
    // synchronising vpz_memcpy_d2h each.  A ranges call copies on both routes, and member j gets its window (delivered_length) from `roll`
    // samples into its area; `written` becomes that count.  Its device route queues a vpz_pcm_download per member and synchronises
    // once; its host route is a memcpy per member from the slot's stage
    void copy_down(bool dev)
    {
        for (size_t j = 0; j < sb.members.size(); ++j) {
            if (!live(j) || member_rc[j] != VPZ_OK) continue;
            const Job &J = job(j);
            if (ranged) written[j] = delivered_length(J.wanted, written[j], J.roll);
            if (written[j] <= 0) continue;
            char *to = static_cast<char *>(R.pcm_out) + elem * (size_t)R.pcm_offset[J.k];
            const size_t from = elem * (size_t)(offs[j] + J.roll * C), bytes = elem * (size_t)(written[j] * C);  // (a whole stream rolls 0)
            if (!dev) {
                memcpy(to, static_cast<char *>(out_at) + from, bytes);
            } else if ((ranged ? vpz_pcm_download(L.ctx, to, L.pcm() + from, bytes) : vpz_memcpy_d2h(L.ctx, to, L.pcm() + from, bytes)) != VPZ_OK) {
                R.m->fail(std::string(ranged ? "vpz_pcm_download: " : "vpz_memcpy_d2h: ") + vpz_context_last_error(L.ctx));
                member_rc[j] = VPZ_E_HIP;
            }
        }
        // (the slot's packet records and the lane's arrays are free again once the stream has drained)
        if (dev && vpz_context_synchronize(L.ctx) != VPZ_OK)
            for (size_t j = 0; j < sb.members.size(); ++j)
                if (member_rc[j] == VPZ_OK) member_rc[j] = VPZ_E_HIP;
    }

    // A batch call copies nothing down: launches of its kind on the lane's stream, after whichever calls stand, move every member's
    // window from the lane's device array into its row of the group's piece and fill the rest of the row -- a member without samples
    // (failed, or nothing left after the roll) gets a samples = 0 descriptor, and so does every member when no call was made (`staged`:
    // the lane's array may not even exist).  One synchronise behind them; a failed launch costs the sub-batch's members VPZM_E_SYNTH
    // (GroupRun::zero_rows defines their rows)
    void deliver_batch()
    {
        const bool staged = has_call() && out_at == L.pcm() && out_at;
        std::vector<vpz_pack_row> rows;
        for (size_t j = 0; j < sb.members.size(); ++j) {
            const Job &J = job(j);
            const bool ok = live(j) && member_rc[j] == VPZ_OK && staged;
            written[j] = ok ? delivered_length(J.wanted, written[j], J.roll) : 0;
            rows.push_back(vpz_pack_row{written[j] > 0 ? offs[j] + J.roll * C : 0, written[j], (int64_t)(J.k - R.lo)});
        }
        int rc = VPZ_OK;
        if (B.measured()) {
            rc = measure_rows(rows, staged);
        } else if (!staged) {
            rc = launched(B.empty_step(), R.sw.fail_delivery ? VPZ_E_HIP : B.empty_rows(L, rows));
        } else if (B.kind == Batch::kPack) {
            rc = launched("vpz_pcm_pack", R.sw.fail_delivery ? VPZ_E_HIP
                                                             : vpz_pcm_pack(L.ctx, L.pcm(), pcm_elems, B.channels, (int32_t)rows.size(), rows.data(), B.dst,
                                                                            B.rows, B.frames, B.layout));
        } else {
            // (a log-mel, fbank or MFCC call: resampled into the lane's temporary, then ONE feature launch on the same stream -- stream-ordered:
            // no synchronise in between)
            if (B.feature) rc = mono_temporary(rows.size());
            if (rc == VPZ_OK && B.by_loudness()) rc = measure_gains(rows);  // (at the streams' own rates, before the resample)
            if (rc == VPZ_OK) rc = resample_by_ratio(rows);
            for (size_t j = 0; j < sb.members.size(); ++j) written[j] = resampled_length(written[j], job(j).up, job(j).down);
            if (rc != VPZ_OK) (void)vpz_context_synchronize(L.ctx);  // (the launches before the failed one have left the lane's array)
            else if (B.feature) rc = feature_rows(rows);
        }
        if (rc == VPZ_OK) rc = vpz_context_synchronize(L.ctx);  // (the lane's arrays are the next sub-batch's once the stream has drained)
        // (a normalised call: the result records came down with that synchronise; a member without samples has the empty record's values)
        // (the gain is reported in double where the row's float32 gain is its rounding: the loudness mode's, unless the ceiling bound)
        for (size_t j = 0; rc == VPZ_OK && j < norm_down.size(); ++j) {
            const bool own = !norm_gain.empty() && (double)(float)norm_gain[j] == norm_down[j].gain;
            B.norm_out[job(j).k] = vpzm_norm_out{own ? norm_gain[j] : norm_down[j].gain, norm_down[j].mean, norm_down[j].peak, norm_loud[j]};
        }
        for (size_t j = 0; j < sb.members.size(); ++j) {
            if (rc == VPZ_OK) job(j).row_packed = true;
            else if (member_rc[j] == VPZ_OK) member_rc[j] = VPZ_E_HIP;
        }
    }

    // a delivery launch's status; a failure goes into the dispatcher's error text under the step's name
    // (tests: with VPZM_FAIL_DELIVERY the callers do not make the launch and pass a failure)
    int launched(const char *step, int rc)
    {
        if (rc != VPZ_OK) R.m->fail(std::string(step) + ": " + vpz_context_last_error(L.ctx));
        return rc;
    }

    // A loudness call: the members that have samples grouped by sample rate (a sub-batch has one channel count), one vpz_pcm_loudness
    // launch per rate on the lane's stream into the lane's temporary -- member j in row j, `max_steps` the sub-batch's largest --, one
    // copy of the temporary down and one synchronise, then the gate per member on this thread.  A member without samples keeps the empty
    // record and needs no launch.  A record is written once everything has succeeded: a failed sub-batch's stay empty.
    // An R 128 call makes one vpz_pcm_true_peak launch per rate behind the loudness launches, over the same descriptors; the true peaks
    // [members] float32 lie behind the peaks in the temporary and come down in the same copy; range and maxima run beside the gate
    // `into` (a normalised call's loudness mode): member j's record goes to (*into)[j], not to the group's piece
    int measure_rows(std::vector<vpz_pack_row> &rows, bool staged, std::vector<vpzm_loudness> *into = nullptr)
    {
        const size_t M = rows.size();
        std::vector<int32_t> rate(M, 0), step(M, 1);
        int64_t max_steps = 1;
        bool any_samples = false;
        for (size_t j = 0; j < M; ++j) {
            rate[j] = R.results[job(j).k].sample_rate;
            step[j] = (rate[j] + 5) / 10;  // (the header's S)
            if (rows[j].samples <= 0) continue;
            any_samples = true;
            max_steps = std::max(max_steps, rows[j].samples / step[j]);
            rows[j].row = (int64_t)j;
        }
        if (R.sw.fail_delivery) return launched("vpz_pcm_loudness", VPZ_E_HIP);
        if (!staged || !any_samples) return VPZ_OK;
        const bool r128 = B.kind == Batch::kR128;
        const size_t sums_bytes = M * (size_t)max_steps * sizeof(double), bytes = sums_bytes + (r128 ? 2 : 1) * M * sizeof(float);
        if (!L.buf[Lane::kLoud].grow(L.ctx, bytes, 1)) {
            R.m->fail("vpzm_measure_loudness: the step sums' device temporary could not be allocated");
            return VPZ_E_NOMEM;
        }
        double *sums_dev = static_cast<double *>(L.buf[Lane::kLoud].p);
        float *peak_dev = reinterpret_cast<float *>(static_cast<char *>(L.buf[Lane::kLoud].p) + sums_bytes);
        float *true_peak_dev = peak_dev + M;  // (kR128)
        std::vector<double> w((size_t)C);
        (void)vpz_loudness_weights(C, w.data());
        if (R.sw.profile) (void)vpz_context_synchronize(L.ctx);  // (the timeline wants the launches' own time)
        const auto t_loud = Clock::now();
        int rc = VPZ_OK, launches = 0;
        std::vector<char> taken(M, 0);
        std::vector<vpz_pack_row> group;
        // the members of row i's rate that no launch of this round has taken
        auto same_rate = [&](size_t i) {
            group.clear();
            for (size_t j = i; j < M; ++j)
                if (!taken[j] && rows[j].samples > 0 && rate[j] == rate[i]) {
                    taken[j] = 1;
                    group.push_back(rows[j]);
                }
        };
        for (size_t i = 0; i < M && rc == VPZ_OK; ++i) {
            if (taken[i] || rows[i].samples <= 0) continue;
            same_rate(i);
            rc = launched("vpz_pcm_loudness", vpz_pcm_loudness(L.ctx, L.pcm(), pcm_elems, C, rate[i], w.data(), (int32_t)group.size(), group.data(), sums_dev,
                                                               peak_dev, (int64_t)M, max_steps));
            ++launches;
        }
        if (R.sw.profile && rc == VPZ_OK && vpz_context_synchronize(L.ctx) == VPZ_OK)
            fprintf(stderr, "[vpzm] group %d: sub-batch %zu loudness kernels %.3f ms (%d launches, %zu rows, %lld steps at most)\n", R.slot_index, b,
                    seconds_since(t_loud) * 1e3, launches, M, (long long)max_steps);
        if (r128) {
            const auto t_peak = Clock::now();
            taken.assign(M, 0);
            launches = 0;
            for (size_t i = 0; i < M && rc == VPZ_OK; ++i) {
                if (taken[i] || rows[i].samples <= 0) continue;
                same_rate(i);
                rc = launched("vpz_pcm_true_peak", vpz_pcm_true_peak(L.ctx, L.pcm(), pcm_elems, C, rate[i], (int32_t)group.size(), group.data(), true_peak_dev,
                                                                     nullptr, (int64_t)M));
                ++launches;
            }
            if (R.sw.profile && rc == VPZ_OK && vpz_context_synchronize(L.ctx) == VPZ_OK)
                fprintf(stderr, "[vpzm] group %d: sub-batch %zu true-peak kernels %.3f ms (%d launches, %zu rows)\n", R.slot_index, b, seconds_since(t_peak) * 1e3,
                        launches, M);
        }
        std::vector<char> down(bytes);
        if (rc == VPZ_OK) rc = launched("vpz_pcm_download", vpz_pcm_download(L.ctx, down.data(), L.buf[Lane::kLoud].p, (uint64_t)bytes));
        rc = vpz_context_synchronize(L.ctx) == VPZ_OK ? rc : rc == VPZ_OK ? VPZ_E_HIP : rc;  // (the copy has landed; the launches before a failed one have left the lane's array)
        if (rc != VPZ_OK) return rc;
        std::vector<std::pair<int64_t, vpzm_r128>> full_records;  // (kR128: written once every member's are there)
        for (size_t j = 0; j < M; ++j) {
            if (rows[j].samples <= 0) continue;
            const int64_t steps = rows[j].samples / step[j];
            float peak_j = 0.0f;
            vpzm_loudness rec{-HUGE_VAL, 0.0, steps, 0};
            std::vector<double> sums((size_t)steps);
            if (steps > 0) memcpy(sums.data(), down.data() + j * (size_t)max_steps * sizeof(double), (size_t)steps * sizeof(double));
            memcpy(&peak_j, down.data() + sums_bytes + j * sizeof(float), sizeof peak_j);
            rec.peak = (double)peak_j;
            (void)vpz_loudness_gate(sums.data(), steps, step[j], &rec.integrated, &rec.blocks_kept);
            if (r128) {
                float true_peak_j = 0.0f;
                memcpy(&true_peak_j, down.data() + sums_bytes + (M + j) * sizeof(float), sizeof true_peak_j);
                vpzm_r128 full{rec.integrated, 0.0, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, (double)true_peak_j, rec.peak, steps, rec.blocks_kept, 0};
                // (the range sorts in memory of its own: out of it, the sub-batch fails with no record written)
                if (vpz_loudness_range(sums.data(), steps, step[j], &full.range, &full.range_low, &full.range_high, &full.range_blocks) != VPZ_OK) {
                    R.m->fail("vpzm_measure_r128: vpz_loudness_range is out of host memory");
                    return VPZ_E_NOMEM;
                }
                (void)vpz_loudness_maxima(sums.data(), steps, step[j], &full.momentary_max, &full.short_term_max);
                full_records.emplace_back((int64_t)(job(j).k - R.lo), full);
                continue;
            }
            (into ? (*into)[j] : B.record((int64_t)(job(j).k - R.lo))) = rec;
        }
        for (const auto &fr : full_records) B.record_r128(fr.first) = fr.second;
        return VPZ_OK;
    }

    // A normalised call's loudness mode: the members' windows measured where the loudness call measures them -- the lane's interleaved
    // PCM at the streams' own rates --, by the same launches, copy and gate; member j's gain is 10^((target - L) / 20), 1 where nothing
    // was measured.  (With VPZM_FAIL_DELIVERY the measurement is not made either: the failed step is the delivery's)
    int measure_gains(const std::vector<vpz_pack_row> &rows)
    {
        norm_loud.assign(rows.size(), -HUGE_VAL);
        norm_gain.assign(rows.size(), 1.0);
        if (R.sw.fail_delivery) return VPZ_OK;
        std::vector<vpz_pack_row> mine(rows);  // (measure_rows renumbers its descriptors' rows)
        std::vector<vpzm_loudness> recs(rows.size(), vpzm_loudness{-HUGE_VAL, 0.0, 0, 0});
        const int rc = measure_rows(mine, true, &recs);
        for (size_t j = 0; rc == VPZ_OK && j < rows.size(); ++j) {
            norm_loud[j] = recs[j].integrated;
            if (norm_loud[j] != -HUGE_VAL) norm_gain[j] = pow(10.0, (B.norm->target - norm_loud[j]) / 20.0);
        }
        return rc;
    }

    // a normalised call: row j's first `written[j]` samples per channel of the temporary become row k - lo of the group's piece; the
    // result records start their way down, and deliver_batch's synchronise lands them
    int normalize_rows(const std::vector<vpz_pack_row> &rows)
    {
        std::vector<vpz_norm_row> d;
        for (size_t j = 0; j < rows.size(); ++j) d.push_back(vpz_norm_row{rows[j].src, rows[j].samples, rows[j].row, norm_gain.empty() ? 1.0 : norm_gain[j]});
        if (R.sw.fail_delivery) return launched(B.feature->step, VPZ_E_HIP);
        bool any_real = false;
        for (const vpz_norm_row &r : d) any_real = any_real || r.samples > 0;
        const bool want = B.norm_out != nullptr && any_real;
        const char *own = nullptr;
        int rc = B.norm_rows(L, L.mono(), (int64_t)rows.size() * B.channels * B.frames, d, want, &own);
        if (own) {
            R.m->fail(std::string(B.feature->step) + ": " + own);  // (a failure in front of the call: the context's last error is an older one)
            return rc;
        }
        rc = launched(B.feature->step, rc);
        if (rc == VPZ_OK && want) {
            if (norm_loud.empty()) norm_loud.assign(rows.size(), -HUGE_VAL);
            norm_down.assign(rows.size(), vpz_norm_result{0.0, 0.0, 0.0, 0.0, 1.0});
            rc = launched("vpz_pcm_download", vpz_pcm_download(L.ctx, norm_down.data(), L.buf[Lane::kNormResult].p, (uint64_t)(rows.size() * sizeof(vpz_norm_result))));
            if (rc != VPZ_OK) norm_down.clear();
        }
        return rc;
    }

    // a log-mel, fbank or MFCC call's resampled rows go to the lane's temporary: mono planar float32 [members][frames], member j in row j;
    // an STFT or CQT call's keep their channels: [members][channels][frames]
    int mono_temporary(size_t members)
    {
        if (L.buf[Lane::kMono].grow(L.ctx, members * (size_t)B.channels * (size_t)B.frames, sizeof(float))) return VPZ_OK;
        R.m->fail(std::string(B.feature->call) + ": the resampled rows' device temporary could not be allocated");
        return VPZ_E_NOMEM;
    }

    // A resampled call: the members grouped by ratio (a sub-batch has one channel count), one vpz_pcm_resample launch per group on the
    // lane's stream -- one launch where the members share a rate, more where streams of one setup differ in rate.  A member without
    // samples needs no ratio of its own: its zero row rides in the first group (alone, at 1:1, when no member has samples).  Into the
    // group's piece, or a feature call's temporary
    int resample_by_ratio(const std::vector<vpz_pack_row> &rows)
    {
        int rc = VPZ_OK;
        std::vector<char> taken(rows.size(), 0);
        std::vector<vpz_pack_row> group;
        for (size_t left = rows.size(); left > 0 && rc == VPZ_OK;) {
            size_t a = rows.size();
            for (size_t j = 0; j < rows.size() && a == rows.size(); ++j)
                if (!taken[j] && rows[j].samples > 0) a = j;
            const int32_t up = a < rows.size() ? job(a).up : 1, down = a < rows.size() ? job(a).down : 1;
            group.clear();
            for (size_t j = 0; j < rows.size(); ++j)
                if (!taken[j] && (rows[j].samples == 0 || (job(j).up == up && job(j).down == down))) {
                    taken[j] = 1;
                    group.push_back(rows[j]);
                    if (B.feature) group.back().row = (int64_t)j;
                }
            left -= group.size();
            rc = R.sw.fail_delivery && !B.feature ? VPZ_E_HIP
                                             : vpz_pcm_resample(L.ctx, L.pcm(), pcm_elems, C, up, down, B.downmix, (int32_t)group.size(), group.data(),
                                                                B.feature ? (void *)L.mono() : B.dst, B.feature ? (int64_t)rows.size() : B.rows, B.channels, B.frames,
                                                                B.layout);
            ++resample_launches;
        }
        return launched("vpz_pcm_resample", rc);
    }

    // a log-mel, fbank or MFCC call: row j's first `written[j]` samples of the temporary become row k - lo of the group's piece
    int feature_rows(std::vector<vpz_pack_row> &rows)
    {
        for (size_t j = 0; j < rows.size(); ++j) rows[j] = vpz_pack_row{(int64_t)j * B.channels * B.frames, written[j], rows[j].row};
        if (B.norm) return normalize_rows(rows);
        if (R.sw.profile) (void)vpz_context_synchronize(L.ctx);  // (the timeline wants the launch's own time)
        const auto t_mel = Clock::now();
        // (a posted call: the feature launch writes member j's frames into row j of the lane's second temporary, and vpz_feat_post's
        // launches, stream-ordered behind it, deliver them into the group's piece with the row's real frames T_L(J))
        std::vector<vpz_feat_row> posted;
        if (B.post) {
            if (!L.buf[Lane::kFeat].grow(L.ctx, rows.size() * (size_t)B.feat_T() * (size_t)B.post_D, sizeof(float))) {
                R.m->fail(std::string(B.feature->call) + ": the feature frames' device temporary could not be allocated");
                return VPZ_E_NOMEM;
            }
            for (size_t j = 0; j < rows.size(); ++j) {
                posted.push_back(vpz_feat_row{(int64_t)j, B.real_frames(written[j]), rows[j].row});
                rows[j].row = (int64_t)j;
            }
        }
        int rc = launched(B.feature->step, R.sw.fail_delivery ? VPZ_E_HIP
                                                                : B.feature_rows(L.ctx, L.mono(), (int64_t)rows.size() * B.channels * B.frames, rows, B.post ? (void *)L.feat() : B.dst,
                                                                                 B.post ? (int64_t)rows.size() : B.rows));
        if (B.post && rc == VPZ_OK) {
            const char *own = nullptr;
            rc = B.post_rows(L, L.feat(), (int64_t)rows.size(), posted, &own);
            if (own) R.m->fail(std::string("vpz_feat_post: ") + own);  // (a failure in front of the call: the context's last error is an older one)
            else rc = launched("vpz_feat_post", rc);
        }
        if (R.sw.profile && rc == VPZ_OK && vpz_context_synchronize(L.ctx) == VPZ_OK)
            fprintf(stderr, "[vpzm] group %d: sub-batch %zu %s kernel %.3f ms (%zu rows of %lld samples)\n", R.slot_index, b, B.feature->name,
                    seconds_since(t_mel) * 1e3, rows.size(), (long long)B.frames);
        return rc;
    }

    // the profile line, then under the group's mutex: the members' results, the group's sums, the slot handed back
    void account()
    {
        for (size_t j = 0; j < sb.members.size(); ++j) job(j).close();  // (a device-decoded sub-batch's containers were kept open for the host path after all)
        const double dt = seconds_since(t0), at_ms = seconds_since(R.t_begin) * 1e3;
        if (R.sw.profile && (sb.on_device || batched))  // (a batch call's host route has the device route's stages but the entropy decode: upload, synth, pack)
            fprintf(stderr, "[vpzm] group %d: sub-batch %zu %s done at %.2f ms (upload %.2f ms, entropy %.2f ms, synth %.2f ms, %s %.2f ms; %lld packets, %lld payload bytes, %d member calls)\n",
                    R.slot_index, b, sb.on_device ? "on the device" : "uploaded", at_ms, t_upload * 1e3, t_entropy * 1e3, t_call * 1e3, batched ? "pack" : "download",
                    t_download * 1e3, (long long)n_pk, (long long)sb.payload_bytes, member_calls);
        if (R.sw.profile && resample_launches > 0)
            fprintf(stderr, "[vpzm] group %d: sub-batch %zu resampled in %d launches (one per ratio among its %zu members)\n", R.slot_index, b, resample_launches,
                    sb.members.size());
        if (R.sw.profile && !(sb.on_device || batched))
            fprintf(stderr, "[vpzm] group %d: sub-batch %zu synthesised at %.2f ms (call %.2f ms, %lld packets, %d member calls)\n", R.slot_index, b, at_ms, dt * 1e3,
                    (long long)n_pk, member_calls);
        std::lock_guard<std::mutex> lk(R.mu);
        R.t_synth += dt;
        R.n_device_subs += sb.on_device && has_call();
        for (size_t j = 0; j < sb.members.size(); ++j) {
            Job &J = job(j);
            if (J.status != VPZM_OK) continue;
            J.finished = true;
            if (sb.on_device && has_call()) {  // (it was entropy-decoded on the device)
                ++R.device_streams;
                R.device_payload += J.payload_bytes;
                R.results[J.k].skipped_packets += J.plan_failures;  // (an unused mode number: the plan's "not decoded", counted as the host decode counts it)
            }
            if (member_rc[j] != VPZ_OK) {
                J.status = member_rc[j] == kNoDecoder ? VPZM_E_SETUP : member_rc[j] == VPZ_E_CAPACITY ? VPZM_E_CAPACITY : VPZM_E_SYNTH;
                continue;
            }
            R.results[J.k].samples = written[j];
            R.samples_total += written[j] * C;
        }
        sb.synth_done = true;
        R.cv.notify_all();
    }
};

void GroupRun::synth_sub(Lane &L, size_t b, Sub &sb)
{
    SubCall c{*this, L, b, sb};
    c.repack();
    c.t0 = Clock::now();
    c.place_outputs();
    if (sb.on_device && c.has_call() && !c.decode_on_device()) c.decode_on_host();
    if (c.batched && !sb.on_device && c.has_call()) c.upload_decoded();
    c.call_batch();
    c.download();
    c.account();
}

}  // namespace

extern "C" {

int vpzm_create(const int32_t *device_ids, int32_t n_devices, const vpzm_options *opt, vpzm_dispatcher **out)
{
    if (!device_ids || n_devices < 1 || n_devices > 64 || !out) return VPZM_E_ARG;
    *out = nullptr;
    std::unique_ptr<vpzm_dispatcher> m(new (std::nothrow) vpzm_dispatcher());
    if (!m) return VPZM_E_NOMEM;
    if (opt) m->opt = *opt;
    const bool threads_by_default = m->opt.host_threads <= 0;
    if (threads_by_default) m->opt.host_threads = vpzh_default_threads();
    // (gpu_entropy: one lane per packet, and a launch's time at small sizes is the latency of one packet's chain -- sixteen streams are
    // too few packets for the device.  Device-resident inputs are not bound by a page-locked slot's size, so a device-decoded call
    // takes more streams by default; a value the caller gives holds for both kinds of call)
    if (m->opt.gpu_entropy) m->device_streams_per_call = m->opt.streams_per_call > 0 ? m->opt.streams_per_call : 64;
    if (m->opt.streams_per_call <= 0) m->opt.streams_per_call = 16;
    // (one GPU, 16 CPUs, 1 024 streams, 16-bit PCM, slots = 4 * contexts + 4: 2 contexts 90 ms, 3: 84 ms, 4: 78 ms -- a host-memory
    // synth call is upload, kernels, download in a row, and only other contexts' calls fill the link's other direction and the
    // device meanwhile.  Every context is an issuing thread that waits in hipStreamSynchronize, so few host threads get few)
    if (m->opt.contexts_per_device <= 0) m->opt.contexts_per_device = m->opt.host_threads / n_devices >= 8 ? 4 : 2;
    if (m->opt.contexts_per_device > 8) m->opt.contexts_per_device = 8;
    // (one GPU, 16 CPUs, 1 024 streams, 16-bit PCM: 6 slots 114 ms, 12 slots 101 ms, 24 slots 104 ms -- with few slots the decode of
    // sub-batch b + slots waits for the synth call of sub-batch b)
    // (the default number of decode threads: the CPUs the process may use PLUS one per issuing thread -- an issuer spends its time waiting
    // for its stream, and on 16 CPUs 20 decode threads beat 16: 74-76 ms against 76-83 for the 1 024-stream job)
    if (threads_by_default) m->opt.host_threads += n_devices * m->opt.contexts_per_device;
    if (m->opt.slots_per_device <= 0) m->opt.slots_per_device = 4 * m->opt.contexts_per_device + 4;
    if (m->opt.slots_per_device < m->opt.contexts_per_device + 1) m->opt.slots_per_device = m->opt.contexts_per_device + 1;
    m->groups.resize((size_t)n_devices);
    int rc = VPZM_OK;
    for (int d = 0; d < n_devices && rc == VPZM_OK; ++d) {
        Group &G = m->groups[(size_t)d];
        G.device = device_ids[d];
        G.lanes.resize((size_t)m->opt.contexts_per_device);
        G.slots.resize((size_t)m->opt.slots_per_device);
        for (Lane &L : G.lanes)
            if (vpz_context_create(G.device, &L.ctx) != VPZ_OK) {
                rc = VPZM_E_DEVICE;
                break;
            }
    }
    if (rc != VPZM_OK) {
        vpzm_destroy(m.release());
        return rc;
    }
    *out = m.release();
    return VPZM_OK;
}

void vpzm_destroy(vpzm_dispatcher *m)
{
    if (!m) return;
    for (Group &G : m->groups) {
        for (Slot &s : G.slots)  // (page-locked memory is a context's: the slots' came from the group's first)
            for (Buffer &b : s.buf) b.release(G.lanes.empty() ? nullptr : G.lanes[0].ctx);
        for (Lane &L : G.lanes) {
            L.decoders.clear();
            L.esetups.clear();
            L.egroups.clear();
            for (Buffer &b : L.buf) b.release(L.ctx);
            if (L.ctx) vpz_context_destroy(L.ctx);
        }
    }
    delete m;
}

const char *vpzm_last_error(vpzm_dispatcher *m) { return m ? m->error.c_str() : "null dispatcher"; }
int vpzm_device_count(vpzm_dispatcher *m) { return m ? (int)m->groups.size() : 0; }

// the partition rule, its one statement: group g of D decodes entries [lo, hi) of n -- shard_range (vorbispizza_amd/sharding.py):
// contiguous, sizes differ by at most one
static void partition(int32_t n, int g, int D, int32_t *lo, int32_t *hi)
{
    *lo = (int32_t)((int64_t)n * g / D);
    *hi = (int32_t)((int64_t)n * (g + 1) / D);
}

// vpzm_decode_library (ranges == nullptr: whole streams), vpzm_decode_ranges and vpzm_decode_ranges_batch (batch != nullptr: its channels,
// frames and layout; group_dst: every group's piece, and no host array -- out_layout is then what the synth calls write, interleaved)
static int decode_call(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                       int32_t out_layout, void *pcm_out, const int64_t *pcm_offset, const int64_t *pcm_capacity,
                       vpzm_stream_result *results, vpzm_stats *stats, const Batch *batch = nullptr, void *const *group_dst = nullptr)
{
    if (!m) return VPZM_E_ARG;
    // (slots, contexts and decoder caches belong to one call at a time: a second caller waits here, it is not refused)
    std::lock_guard<std::mutex> one_call(m->call_mu);
    m->counts = vpzm_call_counts{};  // (of THIS call from here on, however it ends)
    if (n < 0 || !results || (n > 0 && (!data || !size))) return VPZM_E_ARG;
    if (!batch && n > 0 && (!pcm_out || !pcm_offset || !pcm_capacity)) return VPZM_E_ARG;
    if (out_layout != VPZ_OUT_INTERLEAVED && out_layout != VPZ_OUT_INTERLEAVED_S16) return VPZM_E_ARG;
    for (int32_t k = 0; k < n; ++k)
        if (!data[k] || (!batch && (pcm_offset[k] < 0 || pcm_capacity[k] < 0))) return VPZM_E_ARG;
    for (int d = 0; batch && d < (int)m->groups.size(); ++d) {  // (a group without rows needs no piece)
        int32_t lo, hi;
        partition(n, d, (int)m->groups.size(), &lo, &hi);
        if (hi > lo && !group_dst[d]) return VPZM_E_ARG;
    }
    // (the fields appended for gpu_entropy exist for a caller that sets the option; an older caller's struct ends before them)
    if (stats) memset(stats, 0, m->opt.gpu_entropy ? sizeof *stats : offsetof(vpzm_stats, device_gpu_entropy_streams));
    m->error.clear();
    const auto t0 = Clock::now();
    const int D = (int)m->groups.size();
    const int per_device = std::max(1, m->opt.host_threads / D);
    const Switches sw;
    std::vector<std::unique_ptr<GroupRun>> runs;
    std::vector<std::thread> threads;
    try {
        for (int d = 0; d < D; ++d) {
            int32_t lo, hi;
            partition(n, d, D, &lo, &hi);
            runs.emplace_back(new GroupRun{m, m->groups[(size_t)d], d, lo, hi, data, size, ranges, out_layout, pcm_out, pcm_offset,
                                           pcm_capacity, results, per_device, sw, m->mixed_setups && m->opt.gpu_entropy});
            if (batch && hi > lo) {
                runs.back()->batch = *batch;
                runs.back()->batch.dst = group_dst[d];
                runs.back()->batch.rows = hi - lo;
            }
        }
        for (int d = 1; d < D; ++d) threads.emplace_back([&runs, d] { runs[(size_t)d]->run_guarded(); });
        runs[0]->run_guarded();
    } catch (const std::bad_alloc &) {
        for (std::thread &t : threads) t.join();
        return VPZM_E_NOMEM;
    } catch (...) {
        for (std::thread &t : threads) t.join();
        m->fail("vpzm_decode_library: a device thread could not be started");
        return VPZM_E_NOMEM;
    }
    for (std::thread &t : threads) t.join();
    for (const auto &run : runs) {
        m->counts.sub_batches += (int64_t)run->subs.size();
        m->counts.device_decoded_sub_batches += run->n_device_subs;
        m->counts.mixed_sub_batches += run->n_mixed_subs;
        m->counts.max_setups_per_sub_batch = std::max(m->counts.max_setups_per_sub_batch, run->most_setups);
        m->counts.decoders_created += run->decoders_created;
    }
    if (stats) {
        stats->wall_s = seconds_since(t0);
        stats->threads_per_device = per_device;
        size_t pinned = 0;
        for (const Group &G : m->groups)
            for (const Slot &sl : G.slots) pinned += sl.bytes();
        stats->pinned_mib = (int32_t)std::min<size_t>(pinned >> 20, 0x7fffffff);
        for (int d = 0; d < D && d < 16; ++d) {
            stats->device_wall_s[d] = runs[(size_t)d]->t_wall;
            stats->device_decode_s[d] = runs[(size_t)d]->t_decode;
            stats->device_synth_s[d] = runs[(size_t)d]->t_synth;
            stats->device_streams[d] = runs[(size_t)d]->hi - runs[(size_t)d]->lo;
            stats->device_samples[d] = runs[(size_t)d]->samples_total;
            if (m->opt.gpu_entropy) {
                stats->device_gpu_entropy_streams[d] = runs[(size_t)d]->device_streams;
                stats->device_payload_bytes[d] = runs[(size_t)d]->device_payload;
            }
        }
    }
    return VPZM_OK;
}

int vpzm_decode_library(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, int32_t out_layout,
                        void *pcm_out, const int64_t *pcm_offset, const int64_t *pcm_capacity, vpzm_stream_result *results,
                        vpzm_stats *stats)
{
    return decode_call(m, n, data, size, nullptr, out_layout, pcm_out, pcm_offset, pcm_capacity, results, stats);
}

// a VPZ_OUT_* layout as (int16 elements, planar); false: none of the four
static bool layout_of(int32_t layout, bool *s16, bool *planar)
{
    *s16 = layout == VPZ_OUT_INTERLEAVED_S16 || layout == VPZ_OUT_PLANAR_S16;
    *planar = layout == VPZ_OUT_PLANAR || layout == VPZ_OUT_PLANAR_S16;
    return *s16 || *planar || layout == VPZ_OUT_INTERLEAVED;
}
// the rate of a batch is a whole number of Hz (that an int32_t holds)
static bool whole_hz(double rate) { return rate >= 1.0 && rate <= 2147483647.0 && (double)(int32_t)rate == rate; }
// what vpzm_decode_ranges_resampled refuses of a rate, a channel count and a downmix flag
static bool resampled_args_fit(int32_t sample_rate, int32_t channels, int32_t downmix)
{
    return channels >= 1 && channels <= VPZ_MAX_CHANNELS && sample_rate >= 1 && (downmix == 0 || downmix == 1) && (!downmix || channels == 1);
}

// What the ranges family shares.  A call without ranges is refused; one without entries is a ranges call all the same.  A batch call
// (`batch`: kind, channels, frames, layout and what its kind adds) has a piece per group, rows of at least one frame and one of the four
// layouts, and no host array; its synth calls write their areas interleaved -- in the batch's element type where the pack step gives the
// rows their layout, float32 where the resample step converts once, at the end
static int ranges_call(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges, int32_t out_layout,
                       void *pcm_out, const int64_t *pcm_offset, const int64_t *pcm_capacity, vpzm_stream_result *results, vpzm_stats *stats,
                       const Batch *batch = nullptr, void *const *group_dst = nullptr)
{
    if (n > 0 && !ranges) return VPZM_E_ARG;
    static const vpzm_range none{0, 0};
    if (batch) {
        bool s16, planar;
        if (!group_dst || batch->frames < 1 || !layout_of(batch->layout, &s16, &planar)) return VPZM_E_ARG;
        out_layout = s16 && batch->kind == Batch::kPack ? VPZ_OUT_INTERLEAVED_S16 : VPZ_OUT_INTERLEAVED;
    }
    return decode_call(m, n, data, size, ranges ? ranges : &none, out_layout, pcm_out, pcm_offset, pcm_capacity, results, stats, batch, group_dst);
}

int vpzm_decode_ranges(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                       int32_t out_layout, void *pcm_out, const int64_t *pcm_offset, const int64_t *pcm_capacity,
                       vpzm_stream_result *results, vpzm_stats *stats)
{
    return ranges_call(m, n, data, size, ranges, out_layout, pcm_out, pcm_offset, pcm_capacity, results, stats);
}

int vpzm_batch_partition(vpzm_dispatcher *m, int32_t n, int32_t group, int32_t *lo, int32_t *hi)
{
    if (!m || !lo || !hi || n < 0 || group < 0 || group >= (int32_t)m->groups.size()) return VPZM_E_ARG;
    partition(n, group, (int)m->groups.size(), lo, hi);
    return VPZM_OK;
}

int vpzm_decode_ranges_batch(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                             int32_t channels, int64_t frames, int32_t out_layout, void *const *group_dst, vpzm_stream_result *results,
                             vpzm_stats *stats)
{
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return VPZM_E_ARG;
    const Batch batch(Batch::kPack, channels, out_layout, frames);
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

int vpzm_decode_ranges_resampled(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                 int32_t sample_rate, int32_t channels, int32_t downmix, int64_t frames, int32_t out_layout, void *const *group_dst,
                                 vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!resampled_args_fit(sample_rate, channels, downmix)) return VPZM_E_ARG;
    const Batch batch(Batch::kResampled, channels, out_layout, frames, sample_rate, downmix);
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

// the normalised call: the resampled call's arguments and refusals, the spec's own, and the caller's records hold the empty one from here on
int vpzm_decode_ranges_normalized(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                  int32_t sample_rate, int32_t channels, int32_t downmix, int64_t frames, int32_t out_layout, void *const *group_dst,
                                  vpzm_stream_result *results, vpzm_stats *stats, const vpzm_norm_spec *spec, vpzm_norm_out *out)
{
    if (!m || n < 0 || !spec) return VPZM_E_ARG;
    const vpzm_norm_spec &s = *spec;
    if (s.mode < VPZM_NORM_MEANVAR || s.mode > VPZM_NORM_LOUDNESS) return VPZM_E_ARG;
    const bool linear = s.mode == VPZM_NORM_PEAK || s.mode == VPZM_NORM_RMS || s.mode == VPZM_NORM_GAIN;
    if ((linear || s.mode == VPZM_NORM_LOUDNESS) && !std::isfinite(s.target)) return VPZM_E_ARG;
    if (linear && !(s.target > 0.0)) return VPZM_E_ARG;
    if (!std::isfinite(s.eps) || s.eps < 0.0 || !std::isfinite(s.ceiling) || s.ceiling < 0.0) return VPZM_E_ARG;
    if (s.mode == VPZM_NORM_MEANVAR && s.ceiling != 0.0) return VPZM_E_ARG;
    for (int32_t r : s.reserved)
        if (r != 0) return VPZM_E_ARG;
    bool s16, planar;
    if (!resampled_args_fit(sample_rate, channels, downmix) || !layout_of(out_layout, &s16, &planar)) return VPZM_E_ARG;
    for (int32_t k = 0; out && k < n; ++k) out[k] = vpzm_norm_out{1.0, 0.0, 0.0, -HUGE_VAL};
    Batch batch = Batch::featured(kNormalized, spec, sample_rate, downmix, channels, frames);
    batch.norm = spec;
    batch.norm_layout = out_layout;
    batch.norm_out = out;
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

// the log-mel and the mel-spectrogram call: `filterbank` is the query of the kind's library, which states the kernel's limits
static int mel_call(const Feature &feature, decltype(vpz_mel_filterbank) *filterbank, vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size,
                    const vpzm_range *ranges, const vpz_logmel_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!spec) return VPZM_E_ARG;
    if (filterbank(spec, nullptr, nullptr, nullptr, 0, nullptr) != VPZ_OK) return VPZM_E_ARG;
    if (!whole_hz(spec->sample_rate)) return VPZM_E_ARG;
    if (frames < spec->n_fft / 2 + 1) return VPZM_E_ARG;
    const Batch batch = Batch::featured(feature, spec, (int32_t)spec->sample_rate, 1, 1, frames);
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

int vpzm_decode_ranges_logmel(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                              const vpz_logmel_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    return mel_call(kLogmel, vpz_mel_filterbank, m, n, data, size, ranges, spec, frames, group_dst, results, stats);
}

int vpzm_decode_ranges_melspec(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                               const vpz_logmel_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    return mel_call(kMelspec, vpz_melspec_filterbank, m, n, data, size, ranges, spec, frames, group_dst, results, stats);
}

int vpzm_decode_ranges_stft(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                            int32_t sample_rate, int32_t channels, int32_t downmix, const vpz_stft_spec *spec, int64_t frames,
                            void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!spec) return VPZM_E_ARG;
    // (the table's limits are asked of the library that states them; the rest of vorbispizza_pcm_stft.h's are four ranges and the reserved words)
    if (vpz_stft_table(spec->n_fft, spec->win_length, spec->window, nullptr, 0) != VPZ_OK) return VPZM_E_ARG;
    if (spec->hop < 1 || spec->hop > spec->n_fft || spec->output < VPZ_STFT_COMPLEX || spec->output > VPZ_STFT_POWER) return VPZM_E_ARG;
    if (spec->layout != VPZ_STFT_BINS_FIRST && spec->layout != VPZ_STFT_FRAMES_FIRST) return VPZM_E_ARG;
    for (int32_t r : spec->reserved)
        if (r != 0) return VPZM_E_ARG;
    if (frames < spec->n_fft / 2 + 1) return VPZM_E_ARG;
    if (!resampled_args_fit(sample_rate, channels, downmix)) return VPZM_E_ARG;
    const Batch batch = Batch::featured(kStft, spec, sample_rate, downmix, channels, frames);
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

int vpzm_decode_ranges_cqt(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                           int32_t sample_rate, int32_t channels, int32_t downmix, const vpz_cqt_spec *spec, int64_t frames,
                           void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!spec) return VPZM_E_ARG;
    // (the spec's limits are asked of the library that states them, and N_0 with them: the reflect mode's shortest row)
    if (vpz_cqt_bins(spec, nullptr, nullptr, 0) != VPZ_OK) return VPZM_E_ARG;
    int32_t n0 = 0;
    if (vpz_cqt_kernel(spec, 0, nullptr, 0, &n0) != VPZ_OK) return VPZM_E_ARG;
    if (frames < 1 || (spec->pad == VPZ_CQT_PAD_REFLECT && frames < n0 / 2 + 1)) return VPZM_E_ARG;
    if (!resampled_args_fit(sample_rate, channels, downmix)) return VPZM_E_ARG;
    const Batch batch = Batch::featured(kCqt, spec, sample_rate, downmix, channels, frames);
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

// the fbank and the MFCC call, posted (`post`) or not, behind the refusals of the kind's own spec (its limits are the kernel's, asked of
// the library that states them): `mel` is the spec's mel stage, D the feature launch's columns.  The lane's temporary is mono.  A post
// spec fits in the feature tensor's layout (the VPZ_FEAT_* values are the VPZ_FBANK_* ones) and inside vorbispizza_pcm_featpost.h's limits
static int kaldi_call(const Feature &feature, const void *spec, const vpz_fbank_spec &mel, int32_t D, const vpz_feat_post_spec *post, vpzm_dispatcher *m, int32_t n,
                      const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!whole_hz(mel.sample_rate)) return VPZM_E_ARG;
    if (frames < mel.win) return VPZM_E_ARG;
    int64_t elems = 0;
    if (post && (post->layout != mel.layout || vpz_feat_post_scratch(post, 0, 1 + (frames - mel.win) / mel.hop, D, &elems) != VPZ_OK)) return VPZM_E_ARG;
    Batch batch = Batch::featured(feature, spec, (int32_t)mel.sample_rate, 1, 1, frames);
    batch.post = post;
    batch.post_mel = &mel;
    batch.post_D = D;
    return ranges_call(m, n, data, size, ranges, 0, nullptr, nullptr, nullptr, results, stats, &batch, group_dst);
}

int vpzm_decode_ranges_fbank(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                             const vpz_fbank_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    return vpzm_decode_ranges_fbank_post(m, n, data, size, ranges, spec, nullptr, frames, group_dst, results, stats);
}

int vpzm_decode_ranges_fbank_post(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                  const vpz_fbank_spec *spec, const vpz_feat_post_spec *post, int64_t frames, void *const *group_dst,
                                  vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!spec) return VPZM_E_ARG;
    if (vpz_fbank_filterbank(spec, nullptr, nullptr, nullptr, 0, nullptr) != VPZ_OK) return VPZM_E_ARG;
    return kaldi_call(kFbank, spec, *spec, spec->n_mels, post, m, n, data, size, ranges, frames, group_dst, results, stats);
}

int vpzm_decode_ranges_mfcc(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                            const vpz_mfcc_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats)
{
    return vpzm_decode_ranges_mfcc_post(m, n, data, size, ranges, spec, nullptr, frames, group_dst, results, stats);
}

int vpzm_decode_ranges_mfcc_post(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                 const vpz_mfcc_spec *spec, const vpz_feat_post_spec *post, int64_t frames, void *const *group_dst,
                                 vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!spec) return VPZM_E_ARG;
    if (vpz_mfcc_table(spec, nullptr, 0) != VPZ_OK) return VPZM_E_ARG;
    return kaldi_call(kMfcc, spec, spec->fbank, spec->n_ceps, post, m, n, data, size, ranges, frames, group_dst, results, stats);
}

// the loudness and the R 128 call: records of the kind's type, `empty` the record of an entry that delivered nothing
extern "C++" {
template <class Record>
static int measure_call(Batch::Kind kind, const Record &empty, vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size,
                        const vpzm_range *ranges, Record *out, vpzm_stream_result *results, vpzm_stats *stats)
{
    if (!m || n < 0 || (n > 0 && !out)) return VPZM_E_ARG;
    // (no tensor and no row length: `frames` caps nothing; the synth calls write float32, interleaved; every group's piece is its part of
    // the caller's records, which hold the empty record from here on -- a group without entries needs none)
    static Record nobody{};
    std::vector<vpzm_range> whole;
    std::vector<void *> pieces;
    try {
        if (!ranges) whole.assign((size_t)n, vpzm_range{0, -1});
        for (int g = 0; g < (int)m->groups.size(); ++g) {
            int32_t lo, hi;
            partition(n, g, (int)m->groups.size(), &lo, &hi);
            pieces.push_back(hi > lo ? (void *)(out + lo) : (void *)&nobody);
        }
    } catch (const std::bad_alloc &) {
        return VPZM_E_NOMEM;
    }
    for (int32_t k = 0; k < n; ++k) out[k] = empty;
    const Batch batch(kind, 0, VPZ_OUT_INTERLEAVED, INT64_MAX);
    return ranges_call(m, n, data, size, ranges ? ranges : whole.data(), 0, nullptr, nullptr, nullptr, results, stats, &batch, pieces.data());
}
}

int vpzm_measure_loudness(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                          vpzm_loudness *out, vpzm_stream_result *results, vpzm_stats *stats)
{
    return measure_call(Batch::kLoudness, vpzm_loudness{-HUGE_VAL, 0.0, 0, 0}, m, n, data, size, ranges, out, results, stats);
}

int vpzm_measure_r128(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges, vpzm_r128 *out,
                      vpzm_stream_result *results, vpzm_stats *stats)
{
    return measure_call(Batch::kR128, vpzm_r128{-HUGE_VAL, 0.0, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, 0.0, 0.0, 0, 0, 0}, m, n, data, size, ranges, out, results, stats);
}

int vpzm_set_mixed_setups(vpzm_dispatcher *m, int32_t on)
{
    if (!m) return VPZM_E_ARG;
    std::lock_guard<std::mutex> one_call(m->call_mu);
    m->mixed_setups = on != 0;
    return VPZM_OK;
}

int vpzm_last_call_counts(vpzm_dispatcher *m, vpzm_call_counts *out)
{
    if (!m || !out) return VPZM_E_ARG;
    std::lock_guard<std::mutex> one_call(m->call_mu);
    *out = m->counts;
    return VPZM_OK;
}

}  // extern "C"
