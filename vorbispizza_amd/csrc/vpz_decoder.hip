// vpz_decoder_*: the decoder's lifecycle, and the device half of a synth call -- staging, uploads, launches, copy-back.
// What a call's batch of packets becomes (frames, runs) is decided by the host plan in synth_plan.hip; no sample
// arithmetic happens here either: that is in the kernels the last stage enqueues.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "synth_plan.hpp"
#include "../../include/vorbispizza_synth_debug.h"

namespace vpz {

static const uint32_t k_inverse_db_bits[256] = {
#include "floor1_inverse_db_bits.inc"
};

// arenas up to this size are read in place by the kernels (half a million packets, 1.5 MB: 2.42 -> 2.35 ms against the copy)
constexpr size_t kZeroCopyMax = 8u << 20;
// VPZ_RESIDUE_I16: 16-bit residue values to the float32 the synthesis kernels read (exact: every int16 is a float32).  Eight values
// per lane and step where the source is 16-byte aligned (a staging buffer always is), one otherwise.
__global__ __launch_bounds__(256) void widen_i16_kernel(const int16_t *__restrict__ in, float *__restrict__ out, long n)
{
    const long stride = (long)gridDim.x * 256 * 8;
    if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += stride) {
            if (i + 8 <= n) {
                const uint4 v = *reinterpret_cast<const uint4 *>(in + i);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                float f[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    f[2 * k] = (float)(int16_t)(w[k] & 0xFFFFu);
                    f[2 * k + 1] = (float)(int16_t)(w[k] >> 16);
                }
                *reinterpret_cast<float4 *>(out + i) = make_float4(f[0], f[1], f[2], f[3]);
                *reinterpret_cast<float4 *>(out + i + 4) = make_float4(f[4], f[5], f[6], f[7]);
            } else {
                for (long j = i; j < n; ++j) out[j] = (float)in[j];
            }
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (float)in[i];
    }
}
static hipError_t launch_widen_i16(const void *in, float *out, int64_t n, int num_cu, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int64_t want = (n + 256 * 8 - 1) / (256 * 8);
    const int grid = (int)std::min<int64_t>(want, (int64_t)num_cu * 8);
    hipLaunchKernelGGL(widen_i16_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const int16_t *>(in), out, (long)n);
    return hipGetLastError();
}

static int grow(Context *ctx, DevBuf &b, size_t need)
{
    return b.grow(ctx, need ? need : 1, "hipMalloc(staging)");
}

static int arena_begin(Context *ctx, PinnedArena &A, size_t need)
{
    if (A.pending) {
        VPZ_HIP_TRY(ctx, hipEventSynchronize(A.uploaded));
        A.pending = false;
    }
    // (the event says "the arena's last readers are done", nothing about memory: without the system-scope fence a default event
    // carries -- a write-back and invalidation of the device's caches behind every call -- the next call's kernels follow this
    // call's without that pause)
    if (!A.uploaded)
        VPZ_HIP_TRY(ctx, hipEventCreateWithFlags(&A.uploaded, hipEventDisableTiming | hipEventDisableSystemFence));
    if (A.cap < need) {
        if (A.base) VPZ_HIP_TRY(ctx, hipHostFree(A.base));
        A.base = nullptr;
        A.mapped = nullptr;
        A.cap = 0;
        const size_t want = need + need / 2 + 4096;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&A.base), want, hipHostMallocMapped);
        if (e != hipSuccess) return set_error(ctx, VPZ_E_NOMEM, "hipHostMalloc(descriptor arena)", e);
        A.cap = want;
        void *m = nullptr;
        A.mapped = hipHostGetDevicePointer(&m, A.base, 0) == hipSuccess ? static_cast<char *>(m) : nullptr;
        if (!A.mapped) (void)hipGetLastError();
    }
    A.used = 0;
    return VPZ_OK;
}

static PacketInfo get_packet_info(int size0, int size1, bool block_flag, bool prev_flag, bool next_flag)
{
    PacketInfo pi;
    const int size = block_flag ? size1 : size0;
    const bool prev = block_flag ? prev_flag : true;
    const bool next = block_flag ? next_flag : true;
    const int center = size / 2;
    if (prev) {
        pi.left_start = 0; pi.left_end = center; pi.length = size / 2; pi.left_use_size1 = block_flag ? 1 : 0;
    } else {
        pi.left_start = (size - size0) / 4; pi.left_end = (size + size0) / 4; pi.length = size0 / 2;
        pi.left_use_size1 = 0;
    }
    if (next) { pi.right_start = center; pi.right_end = size; }
    else { pi.right_start = (size * 3 - size0) / 4; pi.right_end = (size * 3 + size0) / 4; }
    return pi;
}

// Floor1.cs:108-149: neighbours and sort order of the X list
static int build_floor(const vpz_floor1_config &c, FloorDev *f)
{
    memset(f, 0, sizeof *f);
    if (c.x_count < 2 || c.x_count > 64 || c.multiplier < 1 || c.multiplier > 4) return VPZ_E_INVALID_ARG;
    static const int range_lookup[4] = {128, 64, 43, 32};  // Floor1.cs:36
    f->x_count = c.x_count;
    f->multiplier = c.multiplier;
    f->range = range_lookup[c.multiplier - 1] * 2;
    for (int i = 0; i < c.x_count; ++i)
        if (c.x_list[i] < 0 || c.x_list[i] > 32767) return VPZ_E_INVALID_ARG;
    // Floor1.cs:96-97: `_xList[0] = 0; _xList[1] = 1 << rangeBits`.  The render starts its first segment at the
    // post with x == 0 (bin 0 looks its segment up by counting the posts at or below it)
    if (c.x_list[0] != 0 || c.x_list[1] <= 0) return VPZ_E_INVALID_ARG;
    std::vector<int> order(c.x_count);
    for (int i = 0; i < c.x_count; ++i) order[i] = i;
    // sortIdx[0], [1] start as 0, 1 and take part in the exchange sort like every other entry
    for (int i = 0; i < c.x_count - 1; ++i)
        for (int j = i + 1; j < c.x_count; ++j) {
            if (c.x_list[i] == c.x_list[j]) return VPZ_E_INVALID_ARG;  // InvalidDataException :141
            if (c.x_list[order[i]] > c.x_list[order[j]]) std::swap(order[i], order[j]);
        }
    for (int i = 0; i < c.x_count; ++i) f->sorted[i] = (uint32_t)order[i] | ((uint32_t)c.x_list[order[i]] << 16);
    for (int i = 2; i < c.x_count; ++i) {
        int lo = 0, hi = 1;
        for (int j = 2; j < i; ++j) {
            const int t = c.x_list[j];
            if (t < c.x_list[i]) { if (t > c.x_list[lo]) lo = j; }
            else                 { if (t < c.x_list[hi]) hi = j; }
        }
        // (a post below x[0] = 0 cannot exist; one above x[1] keeps hi = 1 and the reference extrapolates: the
        // differences below are what RenderPoint computes, whatever their sign)
        f->step[i][0] = (uint32_t)lo | ((uint32_t)hi << 8) | ((uint32_t)((c.x_list[i] - c.x_list[lo]) & 0xFFFF) << 16);
        f->step[i][1] = (uint32_t)((c.x_list[hi] - c.x_list[lo]) & 0xFFFF);
    }
    return VPZ_OK;
}


}  // namespace vpz

struct vpz_decoder {
    vpz::Decoder impl;
};

using namespace vpz;

extern "C" {

int vpz_decoder_create(vpz_context *c, const vpz_stream_config *cfg, int32_t n_streams, vpz_decoder **out)
{
    if (!c || !cfg || !out || n_streams <= 0) return VPZ_E_INVALID_ARG;
    *out = nullptr;
    Context *ctx = &c->impl;
    if (cfg->channels < 1 || cfg->channels > VPZ_MAX_CHANNELS)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_create: channels out of range");
    if (cfg->block_size0 > cfg->block_size1)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_create: block_size0 > block_size1");
    for (int bs : {cfg->block_size0, cfg->block_size1})
        if (bs < 64 || bs > 8192 || (bs & (bs - 1)) != 0)
            return set_error(ctx, VPZ_E_UNSUPPORTED, "vpz_decoder_create: block sizes must be powers of two in [64, 8192]");
    if (cfg->floor_count < 0 || cfg->mapping_count < 0 || (cfg->floor_count && !cfg->floors && !cfg->floor_types) ||
        (cfg->mapping_count && !cfg->mappings) || cfg->mapping_count > 256 || cfg->floor_count > 64)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_create: bad floor / mapping tables");
    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));

    vpz_decoder *d = new (std::nothrow) vpz_decoder();
    if (!d) return VPZ_E_NOMEM;
    Decoder &D = d->impl;
    D.ctx = ctx;
    D.channels = cfg->channels;
    D.size0 = cfg->block_size0;
    D.size1 = cfg->block_size1;
    D.clip = cfg->clip_samples ? 1 : 0;
    D.n_streams = n_streams;
    {
        const char *no_big = getenv("VPZ_NO_BIG");  // A/B and bit-equality tests: the three-pass path for 4096 / 8192 blocks
        D.big = synth_big_supported(cfg->block_size0, cfg->block_size1) && !(no_big && atoi(no_big));
    }
    D.generic = !synth_supports_sizes(cfg->block_size0, cfg->block_size1) && !D.big;
    D.states.assign(n_streams, StreamState());
    D.floors.assign((size_t)cfg->floor_count, vpz_floor1_config{});
    D.floor_types.assign((size_t)cfg->floor_count, 1);
    D.floors0.assign((size_t)cfg->floor_count, vpz_floor0_config{});
    for (int i = 0; i < cfg->floor_count; ++i) {
        if (cfg->floor_types) D.floor_types[i] = cfg->floor_types[i];
        if (D.floor_types[i] == 1 && cfg->floors) D.floors[i] = cfg->floors[i];
        if (D.floor_types[i] == 0 && cfg->floors0) D.floors0[i] = cfg->floors0[i];
    }
    D.mappings.assign(cfg->mappings, cfg->mappings + cfg->mapping_count);
    static_assert(VPZ_PKT_BLOCK_FLAG == 1 && VPZ_PKT_PREV_FLAG == 2 && VPZ_PKT_NEXT_FLAG == 4, "packet_info index");
    for (int f = 0; f < 8; ++f) D.packet_info[f] = get_packet_info(D.size0, D.size1, f & 1, f & 2, f & 4);
    if (const char *e = getenv("VPZ_NO_DIRECT_I16")) D.no_direct_i16 = atoi(e) != 0;  // A/B and bit-equality tests: always widen int16 residue first
    if (const char *e = getenv("VPZ_NO_CHAIN")) D.no_chain = atoi(e) != 0;  // A/B tests: every run recomputes its predecessor block
    if (const char *e = getenv("VPZ_NO_STEADY")) D.no_steady = atoi(e) != 0;  // A/B tests: no batch takes steady_stereo_kernel
    if (const char *e = getenv("VPZ_DUAL_RUN")) D.dual_run = std::max(4, atoi(e));
    if (const char *e = getenv("VPZ_PLAN_SLOTS")) D.plan_slots = std::max<int64_t>(0, atoll(e));  // tests: long runs from small batches
    if (const char *e = getenv("VPZ_SYNTH_ABLATE")) D.ablate = atoi(e);
    if (const char *e = getenv("VPZ_HOST_THREADS")) D.host_threads = atoi(e);
    if (const char *e = getenv("VPZ_NO_EARLY_UPLOAD")) D.no_early_upload = atoi(e) != 0;
    if (const char *e = getenv("VPZ_PAR_MIN_PACKETS")) D.par_min_packets = atoll(e);

    int rc = VPZ_OK;
    std::vector<FloorDev> fdev(std::max<size_t>(1, D.floors.size()));
    for (size_t i = 0; i < D.floors.size() && rc == VPZ_OK; ++i) {
        if (D.floor_types[i] == 1) {
            rc = build_floor(D.floors[i], &fdev[i]);
        } else if (D.floor_types[i] == 0) {  // Floor0.cs:50-51
            const vpz_floor0_config &f0 = D.floors0[i];
            if (f0.order < 1 || f0.order > 255 || f0.rate < 1 || f0.bark_map_size < 1 || f0.amp_bits < 0 || f0.amp_bits > 63)
                rc = VPZ_E_INVALID_ARG;
        } else {
            rc = VPZ_E_INVALID_ARG;
        }
    }
    std::vector<uint8_t> steps;
    for (size_t m = 0; m < D.mappings.size() && rc == VPZ_OK; ++m) {
        const vpz_mapping_config &mc = D.mappings[m];
        if (mc.coupling_steps < 0 || mc.coupling_steps > VPZ_MAX_COUPLING) { rc = VPZ_E_INVALID_ARG; break; }
        while (mc.coupling_steps && steps.size() % (2 * kStepsPadPairs)) steps.push_back(0);  // (group mode reads 8 bytes of steps at once)
        D.mapping_steps_off.push_back(mc.coupling_steps ? (int32_t)steps.size() : -1);
        for (int i = 0; i < mc.coupling_steps; ++i) {
            const int mag = mc.coupling_magnitude[i], ang = mc.coupling_angle[i];
            if (mag == ang || mag >= D.channels || ang >= D.channels) { rc = VPZ_E_INVALID_ARG; break; }  // Mapping.cs:41
            steps.push_back((uint8_t)mag);
            steps.push_back((uint8_t)ang);
        }
        for (int ch = 0; ch < D.channels && rc == VPZ_OK; ++ch)
            if (D.floors.size() && mc.channel_floor[ch] >= D.floors.size()) rc = VPZ_E_INVALID_ARG;
        D.max_steps = std::max(D.max_steps, (int)mc.coupling_steps);
        // the residue's support (ABI v4; Residue0.cs:122-125): whole point groups of blocksize/16 bins beyond residue_end
        // are skipped.  (residue_begin is validated and kept for the record: real streams begin at bin 0.)
        for (int b = 0; b < 2 && rc == VPZ_OK; ++b) {
            const int half = (b ? D.size1 : D.size0) / 2;
            const int begin = mc.residue_begin[b], end_raw = mc.residue_end[b];
            if (begin < 0 || end_raw < 0 || (end_raw != 0 && begin > end_raw)) { rc = VPZ_E_INVALID_ARG; break; }
            const int end = end_raw == 0 ? half : std::min(end_raw, half);
            const int per_group = std::max(1, half / 8);
            const int groups = std::min(8, (end + per_group - 1) / per_group);
            D.mapping_skip[b].push_back((uint8_t)(half >= 8 ? 8 - groups : 0));
        }
    }
    if (const char *e = getenv("VPZ_NO_SUPPORT"))  // A/B tests: ignore the declared support (load and multiply the zeros)
        if (atoi(e))
            for (int b = 0; b < 2; ++b) std::fill(D.mapping_skip[b].begin(), D.mapping_skip[b].end(), (uint8_t)0);
    // group mode applies a mapping's steps in reverse order with a workgroup barrier only where a step touches a
    // channel an earlier step of the same LEVEL touched: mark those steps, count the levels
    std::vector<uint8_t> steps_lvl = steps;
    int max_levels = 0;
    for (size_t m = 0; m < D.mappings.size() && rc == VPZ_OK; ++m) {
        const int n = D.mappings[m].coupling_steps, off = D.mapping_steps_off[m];
        int levels = n > 0 ? 1 : 0;
        uint32_t used[8] = {};
        for (int i = n - 1; i >= 0; --i) {
            const uint8_t mag = steps[off + 2 * i], ang = steps[off + 2 * i + 1];
            const bool clash = (used[mag >> 5] >> (mag & 31) & 1) || (used[ang >> 5] >> (ang & 31) & 1);
            if (clash) {
                ++levels;
                memset(used, 0, sizeof used);
                if (mag < 128) steps_lvl[off + 2 * i] |= 0x80;
            }
            used[mag >> 5] |= 1u << (mag & 31);
            used[ang >> 5] |= 1u << (ang & 31);
        }
        max_levels = std::max(max_levels, levels);
    }
    D.n_step_pairs = (int)(steps.size() / 2);
    {
        bool has_floor0 = false;
        for (uint8_t t : D.floor_types) has_floor0 |= (t == 0);
        for (uint8_t t : D.floor_types) D.has_floor1 |= (t != 0);
        const char *no_group = getenv("VPZ_NO_GROUP");  // tuning / A-B tests: force the separate coupling pass
        D.group_ok = synth_group_supported(D.channels) && !D.generic && !D.big && !has_floor0 && D.max_steps <= 255 &&
                     D.n_step_pairs <= kGroupMaxStepPairs && !(no_group && atoi(no_group));
        const char *no_dual = getenv("VPZ_NO_DUAL");
        // (type-0 floors ride in the stereo fast path when their bark maps fit a wave's LDS row; VPZ_NO_F0_FUSED=1: the old route)
        const char *no_f0 = getenv("VPZ_NO_F0_FUSED");
        D.f0_fused = has_floor0 && !(no_f0 && atoi(no_f0));
        for (size_t i = 0; i < D.floors0.size() && rc == VPZ_OK; ++i)
            if (D.floor_types[i] == 0) {
                if (D.floors0[i].bark_map_size < 1 || D.floors0[i].bark_map_size > kFloor0MaxBark) D.f0_fused = false;
                D.f0_k = std::max(D.f0_k, (int)D.floors0[i].bark_map_size);
            }
        D.f0_k = (D.f0_k + 255) & ~255;  // (rows of whole 256-value rounds: floor0_curve_kernel stores a round without asking)
        D.dual_ok = synth_dual_supported(D.channels, D.size0, D.size1) && !D.generic && (!has_floor0 || D.f0_fused) && D.max_steps <= 255 &&
                    D.n_step_pairs <= kGroupMaxStepPairs && !(no_dual && atoi(no_dual));
        // The frames of group mode and of the stereo kernel carry their mapping's step count and first pair (frame_flags: 8 bits
        // each, the skip field right above).  Both follow from the limits above; a table that does not fit is refused here, never
        // masked: a masked offset names another mapping's steps, an unmasked one runs into the skip field.
        bool steps_fit = true;
        for (size_t m = 0; m < D.mapping_steps_off.size(); ++m)
            if (D.mappings[m].coupling_steps > 0 &&
                (D.mappings[m].coupling_steps > 255 || D.mapping_steps_off[m] / 2 > (int)kFrameStepsOffMask))
                steps_fit = false;
        D.group_ok = D.group_ok && steps_fit;
        D.dual_ok = D.dual_ok && steps_fit;
        // (the pair route below sets dual_ok on the limits of ITS table: such a decoder's frames get no bits of the decoder-wide one)
        D.wide_steps = D.group_ok || D.dual_ok;
        D.f0_fused = D.f0_fused && D.dual_ok;
        D.max_steps = max_levels;  // from here on: the barriers a frame's coupling needs in group mode
        const char *nc = getenv("VPZ_NO_COMPACT");
        D.no_compact = nc && atoi(nc);
    }
    if (rc != VPZ_OK) {  // (before anything below indexes the floor / step tables with values that failed validation)
        delete d;
        return set_error(ctx, rc, "vpz_decoder_create: invalid floor1 / mapping configuration");
    }
    std::vector<uint32_t> map_bits(std::max<size_t>(1, D.mappings.size()), 0u);
    D.mapping_uses_floor0.assign(D.mappings.size(), 0);
    for (size_t m = 0; m < D.mappings.size(); ++m) {
        const int n = D.mappings[m].coupling_steps;
        if (D.wide_steps && n > 0)
            map_bits[m] = ((uint32_t)n << kFrameStepsShift) |
                          ((uint32_t)(D.mapping_steps_off[m] / 2) << kFrameStepsOffShift);
        map_bits[m] |= ((uint32_t)D.mapping_skip[1][m] << kFrameSkipShift) | ((uint32_t)D.mapping_skip[0][m] << kMapSkipShortShift);
        for (int ch = 0; ch < D.channels; ++ch)
            if (!D.floor_types.empty() && D.floor_types[D.mappings[m].channel_floor[ch]] == 0) D.mapping_uses_floor0[m] = 1;
    }
    // The pair route: do the coupling steps of ALL mappings join the channels two by two (a channel has at most one partner, the
    // same in every mapping)?  Then the coupled pairs and, two by two in channel order, the uncoupled channels are the pairs;
    // every (pair, mapping) gets its own step list -- the mapping's steps between the pair's channels, in the mapping's order.
    std::vector<uint8_t> pair_ch, pair_steps;
    std::vector<uint32_t> pair_map_bits;
    {
        // (VPZ_NO_GROUP=1 asks for the separate coupling pass for everything with more than two channels: no pairs either)
        const char *no_dual = getenv("VPZ_NO_DUAL"), *no_pairs = getenv("VPZ_NO_PAIRS"), *no_group = getenv("VPZ_NO_GROUP");
        bool has_floor0 = false;
        for (uint8_t t : D.floor_types) has_floor0 |= (t == 0);
        const int C = D.channels;
        bool ok = synth_pairs_supported(C, D.size0, D.size1) && !D.generic && !has_floor0 && !(no_dual && atoi(no_dual)) &&
                  !(no_pairs && atoi(no_pairs)) && !(no_group && atoi(no_group)) && D.mappings.size() <= 255;
        std::vector<int> partner((size_t)std::max(C, 1), -1);
        for (size_t m = 0; m < D.mappings.size() && ok; ++m) {
            const int n = D.mappings[m].coupling_steps, off = D.mapping_steps_off[m];
            for (int i = 0; i < n && ok; ++i) {
                const int mag = steps[off + 2 * i], ang = steps[off + 2 * i + 1];
                if (mag >= C || ang >= C || mag == ang) ok = false;
                else if (partner[mag] < 0 && partner[ang] < 0) { partner[mag] = ang; partner[ang] = mag; }
                else if (partner[mag] != ang || partner[ang] != mag) ok = false;
            }
        }
        if (ok) {
            int lone = -1;
            for (int c = 0; c < C; ++c) {
                if (partner[c] > c) { pair_ch.push_back((uint8_t)c); pair_ch.push_back((uint8_t)partner[c]); }
                else if (partner[c] < 0) {
                    if (lone < 0) lone = c;
                    else { pair_ch.push_back((uint8_t)lone); pair_ch.push_back((uint8_t)c); lone = -1; }
                }
            }
            ok = lone < 0 && (int)pair_ch.size() == C;
        }
        if (ok) {
            const size_t nm = std::max<size_t>(1, D.mappings.size());
            const int n_pairs = C / 2;
            pair_map_bits.assign((size_t)n_pairs * nm, 0u);
            for (int p = 0; p < n_pairs && ok; ++p)
                for (size_t m = 0; m < D.mappings.size() && ok; ++m) {
                    const int n = D.mappings[m].coupling_steps, off = D.mapping_steps_off[m];
                    const int a = pair_ch[2 * p], b = pair_ch[2 * p + 1];
                    const size_t first = pair_steps.size() / 2;
                    int cnt = 0;
                    for (int i = 0; i < n; ++i) {
                        const int mag = steps[off + 2 * i];
                        if (mag != a && mag != b) continue;
                        pair_steps.push_back(mag == a ? 0 : 1);
                        pair_steps.push_back(mag == a ? 1 : 0);
                        ++cnt;
                    }
                    if (cnt > 255 || first > 255) ok = false;
                    uint32_t w = ((uint32_t)D.mapping_skip[1][m] << kFrameSkipShift) | ((uint32_t)D.mapping_skip[0][m] << kMapSkipShortShift);
                    if (cnt > 0) w |= ((uint32_t)cnt << kFrameStepsShift) | ((uint32_t)first << kFrameStepsOffShift);
                    pair_map_bits[(size_t)p * nm + m] = w;
                }
            ok = ok && pair_steps.size() / 2 <= (size_t)kGroupMaxStepPairs;
        }
        D.pairs = ok;
        if (const char *e = getenv("VPZ_PAIRS")) D.pairs_always = atoi(e) != 0;
        if (ok) {
            D.dual_ok = true;
            D.n_pair_step_pairs = (int)(pair_steps.size() / 2);
        }
    }
    if ((rc = get_tables(ctx, D.size0, &D.t0)) != VPZ_OK || (rc = get_tables(ctx, D.size1, &D.t1)) != VPZ_OK) {
        delete d;
        return rc;
    }
    hipError_t e = hipSuccess;
    const size_t state_bytes = 2 * sizeof(float) * (size_t)n_streams * D.channels * (D.size1 / 2);  // two copies, see StreamState
    if (!ctx->d_inv_db) {
        // (+ 64 floats of +0.0 behind the table: where the pair route sends the loads of bins beyond a residue's declared support)
        e = hipMalloc((void **)&ctx->d_inv_db, (256 + 64) * sizeof(float));
        if (e == hipSuccess) e = hipMemset(ctx->d_inv_db, 0, (256 + 64) * sizeof(float));
        if (e == hipSuccess)
            e = hipMemcpy(ctx->d_inv_db, k_inverse_db_bits, 256 * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_floors, sizeof(FloorDev) * fdev.size());
    if (e == hipSuccess) e = hipMemcpy(D.d_floors, fdev.data(), sizeof(FloorDev) * fdev.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_state_h, state_bytes);
    if (e == hipSuccess) e = hipMemset(D.d_state_h, 0, state_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_clipped, sizeof(int32_t) * (size_t)n_streams);
    if (e == hipSuccess) e = hipMemset(D.d_clipped, 0, sizeof(int32_t) * (size_t)n_streams);
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_steps, steps.size() ? steps.size() : 1);
    if (e == hipSuccess && !steps.empty()) e = hipMemcpy(D.d_steps, steps.data(), steps.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_map_bits, sizeof(uint32_t) * map_bits.size());
    if (e == hipSuccess) e = hipMemcpy(D.d_map_bits, map_bits.data(), sizeof(uint32_t) * map_bits.size(), hipMemcpyHostToDevice);
    if (D.pairs) {
        if (e == hipSuccess) e = hipMalloc((void **)&D.d_pair_ch, pair_ch.size());
        if (e == hipSuccess) e = hipMemcpy(D.d_pair_ch, pair_ch.data(), pair_ch.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void **)&D.d_pair_map_bits, sizeof(uint32_t) * pair_map_bits.size());
        if (e == hipSuccess)
            e = hipMemcpy(D.d_pair_map_bits, pair_map_bits.data(), sizeof(uint32_t) * pair_map_bits.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void **)&D.d_pair_steps, pair_steps.size() + 8);
        if (e == hipSuccess && !pair_steps.empty())
            e = hipMemcpy(D.d_pair_steps, pair_steps.data(), pair_steps.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&D.d_steps_lvl, steps_lvl.size() ? steps_lvl.size() : 1);
    if (e == hipSuccess && !steps_lvl.empty())
        e = hipMemcpy(D.d_steps_lvl, steps_lvl.data(), steps_lvl.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // Floor0 ctor tables (Floor0.cs:82-95): one bark map per block size, n+1 ints, last bin left at 0
        std::vector<int32_t> maps;
        std::vector<uint16_t> f0_bark;
        std::vector<char> devs(floor0_dev_size() * std::max<size_t>(1, D.floors0.size()), 0);
        bool any0 = false;
        for (size_t i = 0; i < D.floors0.size(); ++i) {
            if (D.floor_types[i] != 0) continue;
            any0 = true;
            const vpz_floor0_config &f0 = D.floors0[i];
            int64_t off[2];
            const int halves[2] = {D.size0 / 2, D.size1 / 2};
            for (int b = 0; b < 2; ++b) {
                const int n = halves[b];
                off[b] = (int64_t)maps.size();
                auto to_bark = [](double lsp) -> float {
                    return (float)(13.1 * atan(0.00074 * lsp) + 2.24 * atan(0.0000000185 * lsp * lsp) + .0001 * lsp);
                };
                const float scale = (float)f0.bark_map_size / to_bark(f0.rate / 2.0);
                std::vector<int32_t> m((size_t)n + 1, 0);
                for (int k = 0; k < n + 1 - 2; ++k) {
                    const int v = (int)floor((double)(to_bark((f0.rate / 2.0) / n * k) * scale));
                    m[k] = std::min(f0.bark_map_size - 1, v);
                }
                m[n] = -1;
                maps.insert(maps.end(), m.begin(), m.end());
            }
            fill_floor0_dev(devs.data() + i * floor0_dev_size(), f0.order, f0.bark_map_size, f0.amp_ofs, off[0], off[1]);
            if (D.f0_fused) {  // the same maps in the order a lane of the stereo fast path holds its bins (SynthArgs.f0_bark)
                if (f0_bark.size() < (D.floors0.size() * 2) * 1024) f0_bark.assign((D.floors0.size() * 2) * 1024, 0);
                for (int b = 0; b < 2; ++b) {
                    const int n = halves[b], lpb = n / 16;
                    if (n != 128 && n != 1024) continue;
                    const int32_t *mp = maps.data() + off[b];
                    uint16_t *T = f0_bark.data() + (i * 2 + (size_t)b) * 1024;
                    for (int l = 0; l < lpb; ++l)
                        for (int mm = 0; mm < 8; ++mm)
                            for (int e2 = 0; e2 < 2; ++e2) {
                                const int v = mp[2 * (l + lpb * mm) + e2];
                                T[l * 16 + 2 * mm + e2] = (uint16_t)std::min(std::max(v, 0), D.f0_k - 1);
                            }
                }
            }
        }
        if (any0) {
            e = hipMalloc(&D.d_floors0, devs.size());
            if (e == hipSuccess) e = hipMemcpy(D.d_floors0, devs.data(), devs.size(), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMalloc((void **)&D.d_bark_maps, sizeof(int32_t) * maps.size());
            if (e == hipSuccess) e = hipMemcpy(D.d_bark_maps, maps.data(), sizeof(int32_t) * maps.size(), hipMemcpyHostToDevice);
            if (e == hipSuccess && D.f0_fused && !f0_bark.empty()) {
                e = hipMalloc((void **)&D.d_f0_bark, sizeof(uint16_t) * f0_bark.size());
                if (e == hipSuccess) e = hipMemcpy(D.d_f0_bark, f0_bark.data(), sizeof(uint16_t) * f0_bark.size(), hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMalloc((void **)&D.d_f0_w, sizeof(float) * D.floors0.size() * (size_t)D.f0_k);
                if (e == hipSuccess) e = launch_floor0_wtab(D.d_floors0, (int)D.floors0.size(), D.f0_k, D.d_f0_w, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            }
        }
    }
    if (e != hipSuccess) {
        vpz_decoder_destroy(d);
        return set_error(ctx, VPZ_E_NOMEM, "vpz_decoder_create: device allocation", e);
    }
    *out = d;
    return VPZ_OK;
}

void vpz_decoder_destroy(vpz_decoder *d)
{
    if (!d) return;
    Decoder &D = d->impl;
    if (D.ctx) {
        (void)hipSetDevice(D.ctx->device);
        (void)hipStreamSynchronize(D.ctx->stream);
    }
    if (D.d_f0_bark) (void)hipFree(D.d_f0_bark);
    if (D.d_f0_w) (void)hipFree(D.d_f0_w);
    DevBuf *bufs[] = {&D.b_f0curve, &D.b_in_amp, &D.b_in_coeff, &D.b_ybuf, &D.b_bigtail, &D.b_curve, &D.b_temp, &D.b_cposts, &D.b_ccount, &D.b_in_res, &D.b_in_res16, &D.b_in_posts,
                      &D.b_in_counts, &D.b_out, &D.arenas[0].dev, &D.arenas[1].dev};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (D.d_floors) (void)hipFree(D.d_floors);
    if (D.d_state_h) (void)hipFree(D.d_state_h);
    if (D.d_clipped) (void)hipFree(D.d_clipped);
    if (D.d_steps) (void)hipFree(D.d_steps);
    if (D.d_steps_lvl) (void)hipFree(D.d_steps_lvl);
    if (D.d_map_bits) (void)hipFree(D.d_map_bits);
    if (D.d_pair_ch) (void)hipFree(D.d_pair_ch);
    if (D.d_pair_map_bits) (void)hipFree(D.d_pair_map_bits);
    if (D.d_pair_steps) (void)hipFree(D.d_pair_steps);
    if (D.d_floors0) (void)hipFree(D.d_floors0);
    if (D.d_bark_maps) (void)hipFree(D.d_bark_maps);
    for (PinnedArena &A : D.arenas) {
        if (A.base) (void)hipHostFree(A.base);
        if (A.uploaded) (void)hipEventDestroy(A.uploaded);
    }
    delete d;
}

int vpz_decoder_reset(vpz_decoder *d, int32_t stream)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (stream >= D.n_streams) return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_reset: bad stream");
    VPZ_HIP_TRY(D.ctx, hipSetDevice(D.ctx->device));
    const int lo = stream < 0 ? 0 : stream, hi = stream < 0 ? D.n_streams : stream + 1;
    for (int s = lo; s < hi; ++s) {  // StreamDecoder.cs:357-369: the position value itself is kept
        const int64_t pos = D.states[s].current_position;
        const int32_t epoch = D.states[s].clip_epoch;
        D.states[s] = StreamState();
        D.states[s].current_position = pos;
        D.states[s].has_position = false;
        // `_hasClipped = false`: the fused kernels record clipping as "the stream's epoch", so moving on to the next
        // epoch clears the flag without any device work; the any-block-size path sets a plain 1 and is cleared below
        D.states[s].clip_epoch = D.generic ? 1 : epoch + 1;
    }
    if (D.generic)
        VPZ_HIP_TRY(D.ctx, hipMemsetAsync(D.d_clipped + lo, 0, sizeof(int32_t) * (size_t)(hi - lo), D.ctx->stream));
    return VPZ_OK;
}

// One vpz_decoder_synth call, stage by stage.  Everything here is host work on integers; the sample
// arithmetic is in the kernels the last stage enqueues.
namespace {

struct SynthCall {
    // ---- the call's arguments
    Decoder &D;
    Context *ctx;
    const int64_t n_packets;
    const vpz_packet *packets;
    const float *residue;
    const int16_t *posts;
    const uint8_t *post_counts;
    const int mem_space;
    void *pcm_out;
    const int64_t *stream_out_offset;
    const int64_t stream_out_capacity;
    int64_t capacity_of(int s) const  // (vpz_decoder_set_stream_capacities tightens the call's bound per stream)
    {
        return D.stream_caps.empty() ? stream_out_capacity : std::min(stream_out_capacity, D.stream_caps[(size_t)s]);
    }
    const int out_layout;
    const int64_t channel_stride;
    // ---- derived
    const int C, half0, half1;
    const int64_t n_rec;
    const bool have_posts;
    const bool out_interleaved, out_s16;  // VPZ_OUT_* decomposed
    const size_t out_elem;                // bytes per PCM sample
    PinnedArena *A = nullptr;
    // ---- the plan: what the batch becomes (synth_plan.hpp)
    SynthPlan P;
    // ---- descriptor tables built from the plan (pinned arena; dev() gives the device mirror's address)
    uint8_t *cpk = nullptr;
    int n_cpk = 0;
    int64_t temp_floats = 0;
    uint8_t *f0recs = nullptr;
    int n_f0 = 0;
    int64_t *offs = nullptr;
    GenericFrame *gf = nullptr;
    int64_t *src0 = nullptr, *dst0 = nullptr, *src1 = nullptr, *dst1 = nullptr;
    int32_t *save_list = nullptr;
    size_t n0 = 0, n1 = 0, n_save = 0;
    int64_t y_floats = 0;
    // ---- device views
    const float *d_res = nullptr, *d_amp = nullptr, *d_coeff = nullptr;
    const int16_t *d_posts = nullptr;
    const uint8_t *d_counts = nullptr;
    void *d_out = nullptr;
    bool early_residue = false, early_posts = false;  // stage_inputs_early has the copies under way
    bool spec_i16 = false;        // the synth kernel reads the 16-bit residue in place (SynthArgs.spec_i16)
    int64_t early_res_extent = 0;

    SynthCall(Decoder &dec, int64_t n, const vpz_packet *pk, const float *res, const int16_t *po, const uint8_t *pc,
              int mem, void *out, const int64_t *out_off, int64_t out_cap, int layout, int64_t stride)
        : D(dec), ctx(dec.ctx), n_packets(n), packets(pk), residue(res), posts(po), post_counts(pc), mem_space(mem),
          pcm_out(out), stream_out_offset(out_off), stream_out_capacity(out_cap), out_layout(layout),
          channel_stride(stride), C(dec.channels), half0(dec.size0 / 2), half1(dec.size1 / 2),
          n_rec(n * dec.channels), have_posts(po && pc && !dec.floors.empty()),
          out_interleaved(layout == VPZ_OUT_INTERLEAVED || layout == VPZ_OUT_INTERLEAVED_S16),
          out_s16(layout == VPZ_OUT_INTERLEAVED_S16 || layout == VPZ_OUT_PLANAR_S16),
          out_elem(out_s16 ? sizeof(int16_t) : sizeof(float)),
          P{dec, n, pk, have_posts, mem, reinterpret_cast<uintptr_t>(res), out_interleaved, out_cap}
    {
    }

    // device view of a table carved out of the arena: its copy in the device mirror, or -- for small arenas --
    // the pinned host memory itself, which the GPU reads over the link (see stage_inputs)
    void *dev(const void *host_ptr) const
    {
        if (!host_ptr) return nullptr;
        char *base = zero_copy ? A->mapped : static_cast<char *>(A->dev.p);
        return base + (static_cast<const char *>(host_ptr) - A->base);
    }
    bool zero_copy = false;
    bool steady_kernel = false;   // launch() gave the batch to steady_stereo_kernel (VPZ_HOST_PROFILE's `kernel` word)

    // The host threads this decoder's calls may use (vpz_decoder_set_host_threads / VPZ_HOST_THREADS; 0: the CPUs the process
    // may run on, divided by LOCAL_WORLD_SIZE, at most 16)
    int resolved_parties = 0;
    int host_parties()
    {
        if (resolved_parties > 0) return resolved_parties;
        int parties = D.host_threads;
        if (parties <= 0) {
            cpu_set_t set;
            parties = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
            // (one process per GPU: the node's cores are shared with the other ranks torchrun started here)
            if (const char *lw = getenv("LOCAL_WORLD_SIZE")) parties /= std::max(1, atoi(lw));
            parties = std::max(1, std::min(parties, 16));
        }
        return resolved_parties = parties;
    }
    // ... and the context's pool, if it is this decoder's: the pool another decoder of the context left behind (another party
    // count, or any count for a decoder held to one thread) is not used -- the run cut then happens on the calling thread.
    // A batch large enough for the parallel pass gets (or replaces) the pool first.
    HostPool *own_pool()
    {
        const int parties = host_parties();
        HostPool *pool = static_cast<HostPool *>(ctx->host_pool);
        if (n_packets >= D.par_min_packets && parties >= 2 && !(pool && pool->parties() == parties)) {
            if (pool) ctx->host_pool_free(pool);
            ctx->host_pool = pool = new HostPool(parties);
            ctx->host_pool_free = [](void *p) { delete static_cast<HostPool *>(p); };
        }
        return pool && parties >= 2 && pool->parties() == parties ? pool : nullptr;
    }

    // Pass 1 and the run cutting (synth_plan.hip), with what they need from this side: the arena, the pool, and the numbers
    // of the kernels' units -- the resident slots only on request (a reused cut hint never asks the HIP runtime for them)
    int plan_frames(int64_t *samples_written)
    {
        P.A = A;
        P.pool = own_pool();
        P.parties = host_parties();
        P.dual_waves = synth_dual_waves();
        P.needs_general = synth_needs_general(D.size0, D.size1);
        P.resident_slots = [](const SynthPlan &p) -> int64_t {
            const Decoder &d = p.D;
            if (d.plan_slots > 0) return d.plan_slots;
            return p.use_dual ? synth_dual_resident_slots(p.facts.any_floor, d.ctx->num_cu)
                   : d.big    ? synth_big_resident_waves(p.facts.any_floor, d.ctx->num_cu, d.size0, d.size1)
                              : synth_resident_waves(p.facts.any_floor, d.ctx->num_cu, d.channels, p.use_group);
        };
        return vpz::plan_frames(P, samples_written);
    }

    // Every per-call table (frame / run descriptors, coupling packets, per-record floor info, output
    // offsets, ...) is carved out of ONE pinned arena that goes to its device mirror in a single copy;
    // two arenas alternate so the host can prepare call k+1 while call k's upload is still queued.
    int open_arena()
    {
        bool has_floor0_type = false;
        for (uint8_t t : D.floor_types) has_floor0_type |= (t == 0);
        const size_t np = (size_t)n_packets;
        // (runs hold >= 3 frames: see plan_runs)
        size_t need = (sizeof(FrameDesc) + sizeof(RunDesc) / 2 + 16 + 2 +
                       coupling_packet_size()) * np +
                      sizeof(RunDesc) * ((size_t)D.n_streams + 1 + 4 * 64) + (have_posts ? (size_t)n_rec : 0) +  // (+ the pieces of long streams)
                      sizeof(int64_t) * (size_t)D.n_streams + 4096;
        if (has_floor0_type) need += floor0_rec_size() * (size_t)n_rec + 64;
        if (D.generic)
            need += (sizeof(GenericFrame) + 4 * sizeof(int64_t) * (size_t)C) * np +
                    sizeof(int32_t) * ((size_t)D.n_streams + 1) + 1024;
        D.arena_idx ^= 1;
        A = &D.arenas[D.arena_idx];
        int rc = arena_begin(ctx, *A, need);
        if (rc != VPZ_OK) return rc;
        return grow(ctx, A->dev, A->cap);
    }

    // coupling packets: de-interleave + inverse coupling into a planar temp laid out in frame order
    void build_coupling_packets()
    {
        if (P.use_dual && D.pairs && !P.compact) {
            // explicit descriptors for the pair route: which steps a frame has depends on the PAIR that looks at it -- the frame
            // names its mapping (bits 16..23), and the kernel puts the pair's count and offset in (SynthArgs.map_bits)
            for (size_t fi = 0; fi < P.n_frames; ++fi) {
                FrameDesc &fd = P.frames[fi];
                fd.flags &= ~0x00FFFF00u;
                if (!(fd.flags & (kFrameDrain | kFrameNoFloor))) fd.flags |= (uint32_t)packets[fd.rec / C].mapping << kFrameStepsOffShift;
            }
        }
        if (!P.facts.need_coupling || P.use_group || P.use_dual) return;
        // the separate pass hands planar, de-coupled spectra over: the frames lose their group-mode bits
        for (size_t fi = 0; fi < P.n_frames; ++fi) P.frames[fi].flags &= 0xFu | (kFrameSkipMask << kFrameSkipShift);
        const size_t cps = coupling_packet_size();
        cpk = arena_alloc<uint8_t>(*A, cps * P.n_frames);
        for (size_t fi = 0; fi < P.n_frames; ++fi) {
            FrameDesc &fd = P.frames[fi];
            if (fd.flags & kFrameDrain) continue;
            const vpz_packet &pk = packets[fd.rec / C];
            const int half = (fd.flags & kFrameLong) ? half1 : half0;
            const bool couple = !(fd.flags & kFrameNoFloor) && D.mappings[pk.mapping].coupling_steps > 0;
            fill_coupling_packet(cpk + (size_t)n_cpk * cps, pk.residue_offset, temp_floats, half,
                                 couple ? D.mapping_steps_off[pk.mapping] : -1,
                                 couple ? D.mappings[pk.mapping].coupling_steps : 0,
                                 (pk.flags & VPZ_PKT_INTERLEAVED) ? 1 : 0);
            fd.spec_off = temp_floats;
            temp_floats += (int64_t)C * half;
            ++n_cpk;
        }
    }

    int build_floor0_records()
    {
        if (!P.facts.any_floor0) return VPZ_OK;
        if (!D.f0_amp || !D.f0_coeff || D.f0_stride < 1)
            return set_error(ctx, VPZ_E_INVALID_ARG,
                             "vpz_decoder_synth: type-0 floors need vpz_decoder_set_floor0_data before the call");
        if (P.use_dual) return VPZ_OK;  // (the stereo fast path applies type-0 floors itself: floor0_curve_kernel works from the per-record info)
        const size_t rs = floor0_rec_size();
        f0recs = arena_alloc<uint8_t>(*A, rs * P.n_frames * (size_t)C);
        for (size_t fi = 0; fi < P.n_frames; ++fi) {
            const FrameDesc &fd = P.frames[fi];
            if (fd.flags & (kFrameDrain | kFrameNoFloor)) continue;
            const vpz_mapping_config &mc = D.mappings[packets[fd.rec / C].mapping];
            const int half = (fd.flags & kFrameLong) ? half1 : half0;
            for (int ch = 0; ch < C; ++ch) {
                const int fl = mc.channel_floor[ch];
                if (D.floor_types[fl] != 0) continue;
                fill_floor0_rec(f0recs + (size_t)n_f0 * rs, fd.spec_off + (int64_t)ch * half, fd.rec + ch, fl, half,
                                (fd.flags & kFrameLong) ? 1 : 0);
                ++n_f0;
            }
        }
        return VPZ_OK;
    }

    int build_output_offsets()
    {
        if (!out_interleaved && channel_stride < stream_out_capacity && C > 1)
            return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: channel_stride smaller than stream_out_capacity");
        offs = arena_alloc<int64_t>(*A, (size_t)D.n_streams);
        dev_channel_stride = channel_stride;
        if (mem_space == VPZ_MEM_HOST) {
            // A host-memory call mirrors its PCM on the device: the streams' areas BACK TO BACK there, whatever lies between them in
            // the caller's array (two short songs at either end of a library's PCM array are two short areas, not the span between
            // them), each on a boundary of 64 elements (256 bytes of float32 PCM, 128 of 16-bit) so that every store of the kernels takes its
            // widest form; copy_back knows both places
            const int64_t align = 64;
            auto up = [&](int64_t v) { return (v + align - 1) / align * align; };
            int64_t at = 0;
            if (out_interleaved) {
                for (int s = 0; s < D.n_streams; ++s) {
                    offs[s] = at;
                    at += up(D.plan.out_count[s] * C);
                }
            } else {
                int64_t most = 0;
                for (int s = 0; s < D.n_streams; ++s) most = std::max(most, D.plan.out_count[s]);
                dev_channel_stride = up(most);
                for (int s = 0; s < D.n_streams; ++s) {
                    offs[s] = at;
                    if (D.plan.out_count[s] > 0) at += dev_channel_stride * C;
                }
            }
            mirror_elems = at;
        } else {
            for (int s = 0; s < D.n_streams; ++s) offs[s] = stream_out_offset ? stream_out_offset[s] : 0;
        }
        return VPZ_OK;
    }
    int64_t dev_channel_stride = 0;  // the channel stride the kernels use: the caller's, or the device mirror's (host-memory calls)
    int64_t mirror_elems = 0;        // PCM elements of a host-memory call's device mirror

    // any-block-size path: per-frame records + gather lists of the two exact-IMDCT launches
    void build_generic_lists()
    {
        if (!D.generic) return;
        gf = arena_alloc<GenericFrame>(*A, P.n_frames);
        src0 = arena_alloc<int64_t>(*A, P.n_frames * (size_t)C);
        dst0 = arena_alloc<int64_t>(*A, P.n_frames * (size_t)C);
        src1 = arena_alloc<int64_t>(*A, P.n_frames * (size_t)C);
        dst1 = arena_alloc<int64_t>(*A, P.n_frames * (size_t)C);
        save_list = arena_alloc<int32_t>(*A, (size_t)D.n_streams + 1);
        size_t fi = 0;
        for (int s = 0; s < D.n_streams; ++s) {
            const size_t cnt = (size_t)D.plan.s_cnt[s];
            int64_t prev_y = P.started_with_prev[s] ? -1 : -2;
            int prev_n = P.started_prev_long[s] ? D.size1 : D.size0;
            long last_block = -1;
            for (size_t k = 0; k < cnt; ++k, ++fi) {
                const FrameDesc &fd = P.frames[fi];
                GenericFrame g{};
                g.spec_off = fd.spec_off;
                g.out_off = fd.out_off;
                g.rec = fd.rec;
                g.stream = s;
                g.left_start = fd.left_start;
                g.packet_len = fd.packet_len;
                g.prev_end = fd.prev_end;
                g.out_count = fd.out_count;
                g.flags = fd.flags;
                g.prev_y_off = prev_y;
                g.prev_n = prev_n;
                if (!(fd.flags & kFrameDrain)) {
                    g.n = (fd.flags & kFrameLong) ? D.size1 : D.size0;
                    g.y_off = y_floats;
                    for (int ch = 0; ch < C; ++ch) {
                        const int64_t so = fd.spec_off + (int64_t)ch * (g.n / 2), dofs = y_floats + (int64_t)ch * g.n;
                        if (fd.flags & kFrameLong) { src1[n1] = so; dst1[n1++] = dofs; }
                        else { src0[n0] = so; dst0[n0++] = dofs; }
                    }
                    y_floats += (int64_t)C * g.n;
                    prev_y = g.y_off;
                    prev_n = g.n;
                    last_block = (long)fi;
                }
                gf[fi] = g;
            }
            if (last_block >= 0) {
                gf[last_block].flags |= kFrameSaveState;
                save_list[n_save++] = (int32_t)last_block;
            }
        }
    }

    // Device side, part 1: VPZ_MEM_HOST inputs are staged, work buffers grown, the arena uploaded.
    // VPZ_MEM_HOST: the caller's residue (and floor records) start their way to the device BEFORE the host state machine runs
    // -- neither depends on it, and the link is what a host-memory call waits for: the pass over the packets (50 us for a
    // sub-batch of 16 real streams on an idle core, several times that while the cores decode) passes under the copy.  What
    // is copied: up to the highest residue a decodable packet names (>= what the state machine will use; within the extent
    // the caller stated, else nothing is started here and the call fails where it always did).  The caller's buffers are
    // read asynchronously from here on: every way out of the call synchronises (see EarlyUploadGuard).
    // the caller's host residue into D.b_in_res: as it is, or -- VPZ_RESIDUE_I16 -- at 2 bytes a value over the link and widened there
    int upload_residue(int64_t ext)
    {
        int rc;
        if (D.residue_format == VPZ_RESIDUE_I16) {
            // (the 16-bit values go over as they are; whether a kernel reads them in place or they are widened first is settled in
            // stage_inputs, once the state machine has said which kernels run)
            if ((rc = grow(ctx, D.b_in_res16, sizeof(int16_t) * (size_t)ext)) != VPZ_OK) return rc;
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_res16.p, residue, sizeof(int16_t) * (size_t)ext, hipMemcpyHostToDevice, ctx->stream));
        } else {
            if ((rc = grow(ctx, D.b_in_res, sizeof(float) * (size_t)ext)) != VPZ_OK) return rc;
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_res.p, residue, sizeof(float) * (size_t)ext, hipMemcpyHostToDevice, ctx->stream));
        }
        return VPZ_OK;
    }

    // ... and its floor records (posts, post counts) into D.b_in_posts / D.b_in_counts
    int upload_posts()
    {
        int rc;
        if ((rc = grow(ctx, D.b_in_posts, sizeof(int16_t) * 64 * (size_t)n_rec)) != VPZ_OK) return rc;
        if ((rc = grow(ctx, D.b_in_counts, (size_t)n_rec)) != VPZ_OK) return rc;
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_posts.p, posts, sizeof(int16_t) * 64 * (size_t)n_rec, hipMemcpyHostToDevice, ctx->stream));
        VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_counts.p, post_counts, (size_t)n_rec, hipMemcpyHostToDevice, ctx->stream));
        return VPZ_OK;
    }

    int stage_inputs_early(int64_t residue_floats, int64_t n_records)
    {
        if (mem_space != VPZ_MEM_HOST || !residue) return VPZ_OK;
        int64_t ext = 0;
        for (int64_t p = 0; p < n_packets; ++p) {
            const vpz_packet &pk = packets[p];
            if (pk.flags & VPZ_PKT_NOT_DECODED) continue;
            if (pk.residue_offset < 0) return VPZ_OK;
            ext = std::max(ext, pk.residue_offset + (int64_t)C * ((pk.flags & VPZ_PKT_BLOCK_FLAG) ? half1 : half0));
        }
        if (ext <= 0 || ext > residue_floats) return VPZ_OK;
        int rc;
        if ((rc = upload_residue(ext)) != VPZ_OK) return rc;
        early_residue = true;
        early_res_extent = ext;
        if (have_posts && n_records >= n_rec && n_rec > 0) {
            if ((rc = upload_posts()) != VPZ_OK) return rc;
            early_posts = true;
        }
        return VPZ_OK;
    }

    int stage_inputs()
    {
        int rc;
        d_res = residue;
        d_posts = posts;
        d_counts = post_counts;
        d_amp = D.f0_amp;
        d_coeff = D.f0_coeff;
        d_out = pcm_out;
        // VPZ_RESIDUE_I16 (ABI v5): the floored stereo fast path reads the 16-bit values in place and widens them in registers; every
        // other kernel reads float32 -- the values are widened into the decoder's staging buffer first (exact either way)
        const bool i16 = D.residue_format == VPZ_RESIDUE_I16;
        spec_i16 = i16 && P.use_dual && !D.pairs && P.facts.any_floor && !D.no_direct_i16 &&
                   (mem_space == VPZ_MEM_HOST || (reinterpret_cast<uintptr_t>(residue) & 7) == 0);
        if (mem_space != VPZ_MEM_HOST && i16 && !spec_i16) {  // device-resident int16 values: widened into the staging buffer
            if ((rc = grow(ctx, D.b_in_res, sizeof(float) * (size_t)P.facts.res_extent)) != VPZ_OK) return rc;
            VPZ_HIP_TRY(ctx, launch_widen_i16(residue, static_cast<float *>(D.b_in_res.p), P.facts.res_extent, ctx->num_cu, ctx->stream));
            d_res = static_cast<const float *>(D.b_in_res.p);
        }
        if (mem_space == VPZ_MEM_HOST) {
            if (!(early_residue && early_res_extent >= P.facts.res_extent) && (rc = upload_residue(P.facts.res_extent)) != VPZ_OK) return rc;
            if (i16 && !spec_i16) {
                if ((rc = grow(ctx, D.b_in_res, sizeof(float) * (size_t)P.facts.res_extent)) != VPZ_OK) return rc;
                VPZ_HIP_TRY(ctx, launch_widen_i16(D.b_in_res16.p, static_cast<float *>(D.b_in_res.p), P.facts.res_extent, ctx->num_cu, ctx->stream));
            }
            d_res = spec_i16 ? static_cast<const float *>(D.b_in_res16.p) : static_cast<const float *>(D.b_in_res.p);
            if (P.facts.any_floor) {
                if (!early_posts && (rc = upload_posts()) != VPZ_OK) return rc;
                d_posts = static_cast<const int16_t *>(D.b_in_posts.p);
                d_counts = static_cast<const uint8_t *>(D.b_in_counts.p);
            }
            if (P.facts.any_floor0) {
                if ((rc = grow(ctx, D.b_in_amp, sizeof(float) * (size_t)n_rec)) != VPZ_OK) return rc;
                if ((rc = grow(ctx, D.b_in_coeff, sizeof(float) * (size_t)n_rec * D.f0_stride)) != VPZ_OK) return rc;
                VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_amp.p, D.f0_amp, sizeof(float) * (size_t)n_rec,
                                                hipMemcpyHostToDevice, ctx->stream));
                VPZ_HIP_TRY(ctx, hipMemcpyAsync(D.b_in_coeff.p, D.f0_coeff, sizeof(float) * (size_t)n_rec * D.f0_stride,
                                                hipMemcpyHostToDevice, ctx->stream));
                d_amp = static_cast<const float *>(D.b_in_amp.p);
                d_coeff = static_cast<const float *>(D.b_in_coeff.p);
            }
            if ((rc = grow(ctx, D.b_out, out_elem * (size_t)mirror_elems + 16)) != VPZ_OK) return rc;
            d_out = D.b_out.p;
        }
        if (P.facts.need_coupling && !P.use_group && !P.use_dual && (rc = grow(ctx, D.b_temp, sizeof(float) * (size_t)temp_floats)) != VPZ_OK)
            return rc;
        if (P.facts.any_floor0 && P.use_dual && (rc = grow(ctx, D.b_f0curve, sizeof(float) * (size_t)n_rec * (size_t)D.f0_k)) != VPZ_OK) return rc;
        if (P.facts.any_floor) {
            if ((rc = grow(ctx, D.b_cposts, sizeof(int32_t) * 64 * (size_t)n_rec)) != VPZ_OK) return rc;
            if ((rc = grow(ctx, D.b_ccount, (size_t)n_rec)) != VPZ_OK) return rc;
            if (D.generic && (rc = grow(ctx, D.b_curve, (size_t)n_rec * (size_t)half1)) != VPZ_OK) return rc;
        }
        if (D.generic && (rc = grow(ctx, D.b_ybuf, sizeof(float) * (size_t)std::max<int64_t>(y_floats, 1))) != VPZ_OK)
            return rc;
        // (A second stream for this upload, ordered with events so that it overlaps the previous call's kernels, was
        // measured 2-3x SLOWER per call on MI355X / ROCm 7.2: cross-stream event waits cost more than the copy.)
        // A small arena is not copied at all: the kernels read the few hundred KiB of descriptors straight from the
        // pinned host memory (each wave fetches its 64-byte run record and two bytes per frame once, at its start).
        // That takes a DMA command and its two command-processor gaps (~25 us) off every call; the arena stays
        // untouched until the kernels are done (`uploaded` is recorded after the launches in that case).
        zero_copy = A->mapped != nullptr && A->used <= kZeroCopyMax && !D.generic;
        if (!zero_copy) {
            VPZ_HIP_TRY(ctx, hipMemcpyAsync(A->dev.p, A->base, A->used, hipMemcpyHostToDevice, ctx->stream));
            VPZ_HIP_TRY(ctx, hipEventRecord(A->uploaded, ctx->stream));
            A->pending = true;
        }
        return VPZ_OK;
    }

    // Device side, part 2: the kernels, all asynchronous on the context's stream.
    int launch()
    {
        const float *d_spec = d_res;
        const int64_t *d_outoff = (stream_out_offset || mem_space == VPZ_MEM_HOST) ? static_cast<const int64_t *>(dev(offs)) : nullptr;
        if (P.facts.need_coupling && !P.use_group && !P.use_dual) {
            hipError_t e = launch_coupling(dev(cpk), n_cpk, D.d_steps, C, d_res, static_cast<float *>(D.b_temp.p), half1,
                                           ctx->stream);
            if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "coupling kernel launch", e);
            d_spec = static_cast<const float *>(D.b_temp.p);
        }
        const int32_t *d_cposts = static_cast<const int32_t *>(D.b_cposts.p);
        const uint8_t *d_ccount = static_cast<const uint8_t *>(D.b_ccount.p);
        if (P.facts.any_floor) {  // Floor1.UnwrapPosts and the choice of the posts a line is drawn to, per channel record
            const bool f0_fused = P.facts.any_floor0 && P.use_dual;
            // (a decoder whose floors are all of type 0 has nothing to unwrap: the curve kernel leaves the records' markers itself)
            hipError_t e = hipSuccess;
            if (!(f0_fused && !D.has_floor1))
                e = launch_floor1_unwrap((int)n_rec, d_posts, d_counts, static_cast<uint8_t *>(dev(P.rec_floor)), D.d_floors,
                                         (int)D.floors.size(), static_cast<int32_t *>(D.b_cposts.p),
                                         static_cast<uint8_t *>(D.b_ccount.p), nullptr, nullptr, ctx->stream, f0_fused ? 1 : 0);
            if (e == hipSuccess && f0_fused) {  // the records' Floor0 curves over their bark indices (Floor0.cs:188-219)
                e = launch_floor0_curves((int)n_rec, static_cast<uint8_t *>(dev(P.rec_floor)), D.d_floors0, d_amp, d_coeff, D.f0_stride,
                                         D.f0_k, D.d_f0_w, static_cast<float *>(D.b_f0curve.p), d_counts,
                                         static_cast<uint8_t *>(D.b_ccount.p), static_cast<int32_t *>(D.b_cposts.p), ctx->stream);
                D.f0_amp = D.f0_coeff = nullptr;  // consumed
            }
            if (e == hipSuccess && D.generic)  // the three-pass path reads the curve from memory
                e = launch_floor1_render((int)n_rec, d_cposts, d_ccount, static_cast<uint8_t *>(dev(P.rec_floor)), half0,
                                         half1, static_cast<uint8_t *>(D.b_curve.p), ctx->stream);
            if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "floor1 unwrap kernel launch", e);
        }
        if (P.facts.any_floor0 && !P.use_dual) {  // Floor0.Apply in place on the temp (rare; Floor0.cs:164-225)
            hipError_t e = launch_floor0_apply(dev(f0recs), n_f0, D.d_floors0, D.d_bark_maps, d_amp, d_coeff, D.f0_stride,
                                               static_cast<float *>(D.b_temp.p), ctx->stream);
            if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "floor0 kernel launch", e);
            D.f0_amp = D.f0_coeff = nullptr;  // consumed
        }
        if (D.generic) {
            // any-block-size path: floor pass, exact IMDCT per size, OLA pass, state save
            const GenericFrame *d_gf = static_cast<const GenericFrame *>(dev(gf));
            float *d_temp = static_cast<float *>(D.b_temp.p);
            float *d_y = static_cast<float *>(D.b_ybuf.p);
            hipError_t e = hipSuccess;
            if (P.facts.any_floor)
                e = launch_generic_floor(d_gf, (int)P.n_frames, C, half1, d_temp, d_ccount,
                                         static_cast<const uint8_t *>(D.b_curve.p), ctx->d_inv_db, ctx->stream);
            // per block size: the gathered FAST transform (every size from 256 up), else the reference's own
            // schedule (64 and 128 must take it: quirk q1)
            auto imdct_gathered = [&](int n, BlockTables *t, int64_t cnt, const int64_t *so, const int64_t *dof) {
                if (n == 4096 && t->d_fast)
                    return launch_imdct_fast_4096(d_temp, d_y, cnt, t->d_fast, ctx, ctx->stream, so, dof);
                if (n == 8192 && t->d_fast)
                    return launch_imdct_fast_8192(d_temp, d_y, cnt, t->d_fast, ctx, ctx->stream, so, dof);
                if (n == 2048 && t->d_fast)
                    return launch_imdct_fast_2048(d_temp, d_y, cnt, t->d_fast, ctx, ctx->stream, so, dof);
                if (n == 256 && t->d_fast)
                    return launch_imdct_fast_256(d_temp, d_y, cnt, t->d_fast, ctx, ctx->stream, so, dof);
                if ((n == 512 || n == 1024) && t->d_fast)
                    return launch_imdct_fast_mid(n, d_temp, d_y, cnt, t->d_fast, ctx, ctx->stream, so, dof);
                return launch_imdct_exact(n, t->ld, d_temp, d_y, cnt, t->d_A, t->d_B, t->d_C, t->d_bitrev, ctx->num_cu,
                                          ctx->stream, so, dof);
            };
            if (e == hipSuccess && n0)
                e = imdct_gathered(D.size0, D.t0, (int64_t)n0, static_cast<const int64_t *>(dev(src0)),
                                   static_cast<const int64_t *>(dev(dst0)));
            if (e == hipSuccess && n1)
                e = imdct_gathered(D.size1, D.t1, (int64_t)n1, static_cast<const int64_t *>(dev(src1)),
                                   static_cast<const int64_t *>(dev(dst1)));
            if (e == hipSuccess)
                e = launch_generic_ola(d_gf, (int)P.n_frames, C, D.size0, D.size1, d_y, D.d_state_h, D.t0->d_slope,
                                       D.t1->d_slope, static_cast<float *>(d_out), d_outoff, dev_channel_stride, out_interleaved,
                                       D.clip, D.d_clipped, out_s16 ? 1 : 0, ctx->stream);
            if (e == hipSuccess)
                e = launch_generic_save_state(d_gf, static_cast<const int32_t *>(dev(save_list)), (int)n_save, C, D.size1,
                                              d_y, D.d_state_h, ctx->stream);
            if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "generic synthesis kernel launch", e);
            return VPZ_OK;
        }
        SynthArgs a{};
        a.frames = static_cast<const FrameDesc *>(dev(P.frames));
        a.cflags = static_cast<const uint8_t *>(dev(P.cflags));
        a.cmap = static_cast<const uint8_t *>(dev(P.cmap));
        a.run_inline = P.use_dual ? static_cast<const uint8_t *>(dev(P.run_inline)) : nullptr;
        a.map_bits = D.d_map_bits;
        a.pair_ch = D.d_pair_ch;
        a.n_pairs = C / 2;
        a.n_mappings = (int32_t)std::max<size_t>(1, D.mappings.size());
        for (int f = 0; f < 8; ++f) {
            const PacketInfo &pi = D.packet_info[f];
            a.geom[f] = PacketGeom{(uint16_t)pi.left_start, (uint16_t)pi.right_start, (uint16_t)pi.right_end,
                                   (uint16_t)pi.left_use_size1};
        }
        a.runs = static_cast<const RunDesc *>(dev(P.runs));
        a.n_runs = (int32_t)P.n_runs;
        a.channels = C;
        a.size0 = D.size0;
        a.size1 = D.size1;
        a.spec = d_spec;
        a.ccount = P.facts.any_floor ? d_ccount : nullptr;
        a.cposts = P.facts.any_floor ? d_cposts : nullptr;
        a.steps = D.d_steps_lvl;
        a.n_step_pairs = D.n_step_pairs;
        a.max_steps = D.max_steps;
        if (P.use_dual && D.pairs) {  // the pairs' own step lists and per-(pair, mapping) words
            a.map_bits = D.d_pair_map_bits;
            a.steps = D.d_pair_steps;
            a.n_step_pairs = D.n_pair_step_pairs;
        }
        a.group = P.use_group ? 1 : 0;
        a.inv_db = ctx->d_inv_db;
        a.f0_curve = static_cast<const float *>(D.b_f0curve.p);
        a.f0_bark = D.d_f0_bark;
        a.f0_stride = D.f0_k;
        a.spec_i16 = spec_i16 ? 1 : 0;
        a.state_h = D.d_state_h;
        if (D.big && !P.use_dual) {
            const int64_t tf = synth_big_tail_floats(D.size1, (int64_t)P.n_runs * C);
            if (tf > 0) {
                const int grc = grow(ctx, D.b_bigtail, sizeof(float) * (size_t)tf);
                if (grc != VPZ_OK) return grc;
            }
            a.big_tail = static_cast<float *>(D.b_bigtail.p);
        }
        a.state_slot_floats = (int64_t)D.n_streams * C * half1;
        a.tw_long = D.t1->d_fast;
        a.tw_short = D.t0->d_fast;
        a.slope0 = D.t0->d_slope;
        a.slope1 = D.t1->d_slope;
        a.out = static_cast<float *>(d_out);
        a.stream_out_off = d_outoff;
        a.channel_stride = dev_channel_stride;
        a.interleaved = out_interleaved;
        a.s16 = out_s16 ? 1 : 0;
        a.clip = D.clip;
        a.clipped = D.d_clipped;
        a.no_batch = ((D.ablate & 128) || !P.cut_by_cost || P.facts.any_floor0) ? 1 : 0;
        a.ablate = D.ablate;
        a.stamps = nullptr;
#if defined(VPZ_STAMPS) || defined(VPZ_WAVE_TIMES)
        static unsigned long long *d_stamps = nullptr;
        constexpr size_t kStampWaves = 1 << 16;  // per-wave records behind the 16 sums: [16 + 16 * run]
        if (!d_stamps) (void)hipMalloc(&d_stamps, (16 + 16 * kStampWaves) * sizeof(unsigned long long));
        (void)hipMemsetAsync(d_stamps, 0, (16 + 16 * std::min<size_t>(kStampWaves, P.n_runs)) * sizeof(unsigned long long), ctx->stream);
        a.stamps = d_stamps;
#endif
        // An all-steady batch (SynthPlan::steady) to planar float32 PCM whose rows take 8-byte stores: steady_stereo_kernel
        // walks the same runs.  The launch alone picks the kernel.
        steady_kernel = false;
        if (P.steady && !out_interleaved && !out_s16 && !spec_i16) {
            int64_t bits = (int64_t)reinterpret_cast<uintptr_t>(d_out) / (int64_t)sizeof(float) | dev_channel_stride;
            if (reinterpret_cast<uintptr_t>(d_out) % sizeof(float)) bits |= 1;
            for (int s = 0; s < D.n_streams; ++s)
                if (D.plan.s_cnt[s] > 0) bits |= offs[s];
            steady_kernel = (bits & 1) == 0;
        }
        hipError_t e = steady_kernel ? launch_steady_stereo(a, ctx->stream)
                     : P.use_dual ? (D.pairs ? launch_synth_pairs(a, P.facts.any_floor, P.facts.ilv_seen, ctx->stream) : launch_synth_dual(a, P.facts.any_floor, P.facts.ilv_seen, ctx->stream))
                                : D.big ? launch_synth_big(a, P.facts.any_floor, ctx->stream) : launch_synth(a, P.facts.any_floor, ctx->stream);
        if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "synth kernel launch", e);
#if defined(VPZ_STAMPS) || defined(VPZ_WAVE_TIMES)
        {
            unsigned long long h[16];
            (void)hipMemcpyAsync(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
            static const char *names_one[9] = {"desc+prefetch", "barrier0", "stage+barrier", "coupling", "pickup+curve",
                                               "floor*+imdct", "wait next", "ola+stores", "tail"};
            static const char *names_dual[9] = {"desc+prefetch", "unpack+coupling", "curves", "floor*+imdct x2", "wait next",
                                                "ola+stores", "tail", "-", "-"};
            const char **names = P.use_dual ? names_dual : names_one;
            unsigned long long tot = 0;
            for (int k = 0; k < 9; ++k) tot += h[k];
            fprintf(stderr, "[stamps] %llu waves, %.0f cycles per wave:", h[15], h[15] ? (double)tot / h[15] : 0.0);
            for (int k = 0; k < 9; ++k) fprintf(stderr, " %s %.1f%%", names[k], tot ? 100.0 * h[k] / tot : 0.0);
            if (h[14] && h[15]) {
                const double mean = (double)tot / h[15], var = (double)h[13] * 1e6 / h[15] - mean * mean;
                fprintf(stderr, " | slowest wave %.0f cycles = %.2f x mean, sigma %.2f x mean, %.1f passes per wave, %d runs", (double)h[14],
                        (double)h[14] / mean, var > 0 ? sqrt(var) / mean : 0.0, (double)h[12] / h[15], (int)P.n_runs);
            }
            fprintf(stderr, "\n");
            if (const char *dump = getenv("VPZ_STAMPS_DUMP")) {  // per-wave records: run, frames, passes, cycles per phase
                const size_t nw = std::min<size_t>(kStampWaves, P.n_runs);
                std::vector<unsigned long long> w(16 * nw);
                (void)hipMemcpy(w.data(), d_stamps + 16, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
                if (FILE *f = fopen(dump, "w")) {
                    fprintf(f, "run,stream,frames,passes,long_frames,c0,c1,c2,c3,c4,c5,c6\n");
                    for (size_t r = 0; r < nw; ++r) {
                        fprintf(f, "%zu,%d,%d,%llu,%llu", r, P.runs[r].stream, P.runs[r].count, w[16 * r + 9], w[16 * r + 10]);
                        for (int k = 0; k < 7; ++k) fprintf(f, ",%llu", w[16 * r + k]);
                        fprintf(f, "\n");
                    }
                    fclose(f);
                }
            }
        }
#endif
        return VPZ_OK;
    }

    // VPZ_MEM_HOST: PCM back to the caller's buffer, synchronously
    int copy_back()
    {
        if (mem_space != VPZ_MEM_HOST) return VPZ_OK;
        for (int s = 0; s < D.n_streams; ++s) {
            if (D.plan.out_count[s] <= 0) continue;
            char *h = static_cast<char *>(pcm_out);
            const char *dv = static_cast<const char *>(d_out);
            const int64_t host_off = stream_out_offset ? stream_out_offset[s] : 0;  // (the device mirror packs the areas: offs[s])
            if (out_interleaved) {
                VPZ_HIP_TRY(ctx, hipMemcpyAsync(h + out_elem * (size_t)host_off, dv + out_elem * (size_t)offs[s],
                                                out_elem * (size_t)(D.plan.out_count[s] * C), hipMemcpyDeviceToHost,
                                                ctx->stream));
            } else {
                for (int ch = 0; ch < C; ++ch) {
                    const size_t at_h = out_elem * (size_t)(host_off + (int64_t)ch * channel_stride);
                    const size_t at_d = out_elem * (size_t)(offs[s] + (int64_t)ch * dev_channel_stride);
                    VPZ_HIP_TRY(ctx, hipMemcpyAsync(h + at_h, dv + at_d, out_elem * (size_t)D.plan.out_count[s],
                                                    hipMemcpyDeviceToHost, ctx->stream));
                }
            }
        }
        VPZ_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return VPZ_OK;
    }
};

}  // namespace

static int synth_impl(vpz_decoder *d, int64_t n_packets, const vpz_packet *packets, const float *residue,
                      int64_t residue_floats, const int16_t *posts, const uint8_t *post_counts, int64_t n_records,
                      int mem_space, void *pcm_out, const int64_t *stream_out_offset, int64_t stream_out_capacity,
                      int out_layout, int64_t channel_stride, int64_t *samples_written)
{
    Decoder &D = d->impl;
    Context *ctx = D.ctx;
    D.mismatch_packets.clear();
    if (n_packets < 0 || (n_packets > 0 && (!packets || !residue || !pcm_out)) || !samples_written)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: null argument");
    // the extents of the caller's buffers are part of the call (the reference's arguments are Span<T>, bounds-checked:
    // Mapping.cs:98): a packet that addresses residue beyond them, or a batch with fewer post records than
    // packets * channels, is refused here -- it would be an out-of-bounds read on the device otherwise
    if (residue_floats < 0 || n_records < 0)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: negative buffer extent");
    if (posts && post_counts && n_records < n_packets * (int64_t)D.channels)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: fewer post records than packets * channels");
    if (mem_space != VPZ_MEM_HOST && mem_space != VPZ_MEM_DEVICE)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: bad mem_space");
    if (out_layout < VPZ_OUT_INTERLEAVED || out_layout > VPZ_OUT_PLANAR_S16)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: bad out_layout");
    if (n_packets > (int64_t)0x7fffffff / std::max(1, D.channels))
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: batch too large");
    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int s = 0; s < D.n_streams; ++s) samples_written[s] = 0;
    D.packet_samples.assign((size_t)n_packets, 0);
    if (n_packets == 0) return VPZ_OK;

    const bool host_profile = getenv("VPZ_HOST_PROFILE") != nullptr;  // (per call: the tests switch it on for single calls)
    auto tick = [] { return std::chrono::steady_clock::now(); };
    const auto t_begin = tick();
    SynthCall call(D, n_packets, packets, residue, posts, post_counts, mem_space, pcm_out, stream_out_offset,
                   stream_out_capacity, out_layout, channel_stride);
    int rc;
    // (whatever the way out: no copy may still be reading the caller's buffers when the call returns)
    struct EarlyUploadGuard {
        Context *ctx;
        SynthCall &call;
        bool completed = false;
        ~EarlyUploadGuard()
        {
            if ((call.early_residue || call.early_posts) && !completed) (void)hipStreamSynchronize(ctx->stream);
        }
    } early_guard{ctx, call};
    if (!D.no_early_upload && (rc = call.stage_inputs_early(residue_floats, n_records)) != VPZ_OK) return rc;
    if ((rc = call.open_arena()) != VPZ_OK) return rc;
    const auto t_arena = tick();
    if ((rc = call.plan_frames(samples_written)) != VPZ_OK) return rc;
    const SynthPlan &plan = call.P;
    if (plan.facts.res_extent > residue_floats)
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_decoder_synth: a packet's residue lies beyond residue_floats");
    const auto t_pass1 = tick();
    if (plan.n_frames == 0) {
        D.states = plan.st;
        return VPZ_OK;  // (window mismatches are per-packet conditions: vpz_decoder_last_packet_status)
    }
    plan_runs(call.P);
    if (plan.host_failed) return set_error(ctx, VPZ_E_NOMEM, "vpz_decoder_synth: run cutting failed (allocation)");
    call.build_coupling_packets();
    if ((rc = call.build_floor0_records()) != VPZ_OK) return rc;
    if ((rc = call.build_output_offsets()) != VPZ_OK) return rc;
    call.build_generic_lists();
    const auto t_pass2 = tick();
    if ((rc = call.stage_inputs()) != VPZ_OK) return rc;
    if ((rc = call.launch()) != VPZ_OK) return rc;
    if (call.zero_copy) {  // the kernels read the arena itself: it is free again when they are done
        VPZ_HIP_TRY(ctx, hipEventRecord(call.A->uploaded, ctx->stream));
        call.A->pending = true;
    }
    if ((rc = call.copy_back()) != VPZ_OK) return rc;
    early_guard.completed = mem_space == VPZ_MEM_HOST;  // (copy_back has waited for the stream)
    if (!D.generic)  // every stream with frames in this batch has had its state written to the other copy
        for (int s = 0; s < D.n_streams; ++s)
            if (D.plan.s_cnt[s] > 0) call.P.st[s].state_slot ^= 1;
    D.states = plan.st;
    if (host_profile) {
        const auto t_end = tick();
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        // (route: which kernel synthesises -- the tests read it to know that the route they ask for is the one that ran)
        const char *route = D.generic ? "generic" : plan.use_dual ? (D.pairs ? "pairs" : "stereo") : D.big ? "big" : plan.use_group ? "group" : "separate";
        // (kernel: on the stereo route, which of its two kernels the launch picked -- `steady` is steady_stereo_kernel)
        fprintf(stderr, "[vpz host] packets %lld: route %s, kernel %s, arena wait %.1f us, pass1 %.1f us (%s), runs %.1f us, uploads+launch %.1f us\n",
                (long long)n_packets, route, call.steady_kernel ? "steady" : "general", us(t_begin, t_arena), us(t_arena, t_pass1), plan.was_parallel ? "parallel" : "serial",
                us(t_pass1, t_pass2), us(t_pass2, t_end));
    }
    return VPZ_OK;  // (window mismatches are per-packet conditions: vpz_decoder_last_packet_status)
}

int vpz_decoder_synth(vpz_decoder *d, int64_t n_packets, const vpz_packet *packets, const float *residue,
                      int64_t residue_floats, const int16_t *posts, const uint8_t *post_counts, int64_t n_records,
                      int mem_space, void *pcm_out, const int64_t *stream_out_offset, int64_t stream_out_capacity,
                      int out_layout, int64_t channel_stride, int64_t *samples_written)
{
    if (!d) return VPZ_E_INVALID_ARG;
    // "never throws": the host half allocates (vectors, the descriptor arena); an allocation failure becomes a status
    try {
        return synth_impl(d, n_packets, packets, residue, residue_floats, posts, post_counts, n_records, mem_space, pcm_out,
                          stream_out_offset, stream_out_capacity, out_layout, channel_stride, samples_written);
    } catch (const ArenaOverflow &) {
        return set_error(d->impl.ctx, VPZ_E_NOMEM, "vpz_decoder_synth: the descriptor arena is too small for this batch");
    } catch (const std::bad_alloc &) {
        return set_error(d->impl.ctx, VPZ_E_NOMEM, "vpz_decoder_synth: host allocation failed");
    } catch (...) {
        return set_error(d->impl.ctx, VPZ_E_NOMEM, "vpz_decoder_synth: host pass failed");
    }
}

int vpz_decoder_last_packet_status(vpz_decoder *d, int32_t *out, int64_t capacity, int64_t *n_not_ok)
{
    if (!d || capacity < 0 || (capacity > 0 && !out)) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    const int64_t n = std::min<int64_t>(capacity, (int64_t)D.packet_samples.size());
    for (int64_t i = 0; i < n; ++i) out[i] = VPZ_OK;
    for (int64_t p : D.mismatch_packets)
        if (p < n) out[p] = VPZ_E_WINDOW_MISMATCH;
    if (n_not_ok) *n_not_ok = (int64_t)D.mismatch_packets.size();
    return VPZ_OK;
}

// test-only: the integers of the Floor1 device path (include/vorbispizza_synth_debug.h)
int vpz_debug_floor1_indices(vpz_decoder *d, int64_t n_records, const int16_t *posts, const uint8_t *post_counts,
                             const uint8_t *record_floor, const uint8_t *record_long, uint8_t *curve_out,
                             int16_t *final_y_out, uint8_t *step_flags_out, uint8_t *active_count_out)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    Context *ctx = D.ctx;
    if (n_records < 0 || n_records > 0x7fffffff / 64 || (n_records > 0 && (!posts || !post_counts || !record_floor || !record_long)))
        return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_debug_floor1_indices: bad arguments");
    if (n_records == 0) return VPZ_OK;
    const size_t n = (size_t)n_records;
    const int half0 = D.size0 / 2, half1 = D.size1 / 2;
    std::vector<uint8_t> info(n);
    for (size_t r = 0; r < n; ++r) {
        if (record_floor[r] >= D.floors.size() || D.floor_types[record_floor[r]] != 1)
            return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_debug_floor1_indices: record_floor is not a type-1 floor");
        info[r] = (uint8_t)(record_floor[r] | (record_long[r] ? 0x80 : 0));
    }
    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    struct Bufs {
        void *p[7] = {};
        ~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
    } B;
    const size_t bytes[7] = {n * 128, n, n, n * 256, n, n * (size_t)half1, n * 64 * 3};
    for (int i = 0; i < 7; ++i) VPZ_HIP_TRY(ctx, hipMalloc(&B.p[i], bytes[i]));
    int16_t *d_posts = static_cast<int16_t *>(B.p[0]);
    uint8_t *d_counts = static_cast<uint8_t *>(B.p[1]), *d_info = static_cast<uint8_t *>(B.p[2]);
    int32_t *d_cposts = static_cast<int32_t *>(B.p[3]);
    uint8_t *d_ccount = static_cast<uint8_t *>(B.p[4]), *d_curve = static_cast<uint8_t *>(B.p[5]);
    int16_t *d_y = static_cast<int16_t *>(B.p[6]);
    uint8_t *d_f = static_cast<uint8_t *>(B.p[6]) + n * 128;
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(d_posts, posts, bytes[0], hipMemcpyHostToDevice, ctx->stream));
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(d_counts, post_counts, n, hipMemcpyHostToDevice, ctx->stream));
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(d_info, info.data(), n, hipMemcpyHostToDevice, ctx->stream));
    if (curve_out) VPZ_HIP_TRY(ctx, hipMemcpyAsync(d_curve, curve_out, bytes[5], hipMemcpyHostToDevice, ctx->stream));
    VPZ_HIP_TRY(ctx, hipMemsetAsync(B.p[6], 0, bytes[6], ctx->stream));
    hipError_t e = launch_floor1_unwrap((int)n, d_posts, d_counts, d_info, D.d_floors, (int)D.floors.size(), d_cposts,
                                        d_ccount, d_y, d_f, ctx->stream);
    if (e == hipSuccess) e = launch_floor1_render((int)n, d_cposts, d_ccount, d_info, half0, half1, d_curve, ctx->stream);
    if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, "floor1 debug kernels", e);
    if (curve_out) VPZ_HIP_TRY(ctx, hipMemcpyAsync(curve_out, d_curve, bytes[5], hipMemcpyDeviceToHost, ctx->stream));
    if (final_y_out) VPZ_HIP_TRY(ctx, hipMemcpyAsync(final_y_out, d_y, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    if (step_flags_out) VPZ_HIP_TRY(ctx, hipMemcpyAsync(step_flags_out, d_f, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    if (active_count_out) VPZ_HIP_TRY(ctx, hipMemcpyAsync(active_count_out, d_ccount, n, hipMemcpyDeviceToHost, ctx->stream));
    VPZ_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return VPZ_OK;
}

int vpz_decoder_set_floor0_data(vpz_decoder *d, const float *amp, const float *coeff, int32_t coeff_stride)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if ((amp == nullptr) != (coeff == nullptr) || (amp && coeff_stride < 1))
        return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_floor0_data: bad arguments");
    // (a record's coefficients are coeff[rec * coeff_stride + j], j < order: a row shorter than an order would make the kernels
    // read the next record's coefficients, and beyond the array on the last record)
    int max_order = 0;
    for (size_t i = 0; i < D.floors0.size(); ++i)
        if (D.floor_types[i] == 0) max_order = std::max(max_order, (int)D.floors0[i].order);
    if (amp && coeff_stride < max_order) {
        char msg[160];
        snprintf(msg, sizeof msg, "vpz_decoder_set_floor0_data: coeff_stride %d is smaller than the order %d of a type-0 floor",
                 (int)coeff_stride, max_order);
        return set_error(D.ctx, VPZ_E_INVALID_ARG, msg);
    }
    D.f0_amp = amp;
    D.f0_coeff = coeff;
    D.f0_stride = coeff_stride;
    return VPZ_OK;
}

int vpz_decoder_last_packet_samples(vpz_decoder *d, int32_t *out, int64_t capacity)
{
    if (!d || (!out && capacity > 0) || capacity < 0) return VPZ_E_INVALID_ARG;
    const Decoder &D = d->impl;
    const int64_t n = std::min<int64_t>(capacity, (int64_t)D.packet_samples.size());
    if (n > 0) memcpy(out, D.packet_samples.data(), sizeof(int32_t) * (size_t)n);
    return VPZ_OK;
}

int vpz_decoder_has_clipped(vpz_decoder *d, int32_t stream, int32_t *has_clipped)
{
    if (!d || !has_clipped) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (stream < 0 || stream >= D.n_streams) return set_error(D.ctx, VPZ_E_INVALID_ARG, "bad stream index");
    int32_t v = 0;
    VPZ_HIP_TRY(D.ctx, hipMemcpyAsync(&v, D.d_clipped + stream, sizeof v, hipMemcpyDeviceToHost, D.ctx->stream));
    VPZ_HIP_TRY(D.ctx, hipStreamSynchronize(D.ctx->stream));
    *has_clipped = D.generic ? v != 0 : v == D.states[stream].clip_epoch;
    return VPZ_OK;
}

int vpz_decoder_set_position(vpz_decoder *d, int32_t stream, int64_t sample_position)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (stream < 0 || stream >= D.n_streams) return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_position: bad stream");
    D.states[stream].current_position = sample_position;
    D.states[stream].has_position = true;
    return VPZ_OK;
}

int vpz_decoder_set_residue_format(vpz_decoder *d, int32_t format)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (format != VPZ_RESIDUE_F32 && format != VPZ_RESIDUE_I16)
        return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_residue_format: neither VPZ_RESIDUE_F32 nor VPZ_RESIDUE_I16");
    D.residue_format = format;
    return VPZ_OK;
}

int vpz_decoder_set_host_threads(vpz_decoder *d, int32_t n)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (n < 0) return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_host_threads: negative thread count");
    D.host_threads = std::min<int32_t>(n, 16);
    return VPZ_OK;
}

int vpz_decoder_set_stream_capacities(vpz_decoder *d, const int64_t *capacity, int32_t n)
{
    if (!d) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (!capacity && n == 0) {
        D.stream_caps.clear();
        return VPZ_OK;
    }
    if (!capacity || n != D.n_streams)
        return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_stream_capacities: one capacity per stream of the decoder, or (NULL, 0)");
    for (int32_t s = 0; s < n; ++s)
        if (capacity[s] < 0) return set_error(D.ctx, VPZ_E_INVALID_ARG, "vpz_decoder_set_stream_capacities: negative capacity");
    try {
        D.stream_caps.assign(capacity, capacity + n);
    } catch (const std::bad_alloc &) {
        return set_error(D.ctx, VPZ_E_NOMEM, "vpz_decoder_set_stream_capacities: out of host memory");
    }
    return VPZ_OK;
}

int vpz_decoder_position(vpz_decoder *d, int32_t stream, int64_t *sample_position)
{
    if (!d || !sample_position) return VPZ_E_INVALID_ARG;
    Decoder &D = d->impl;
    if (stream < 0 || stream >= D.n_streams) return set_error(D.ctx, VPZ_E_INVALID_ARG, "bad stream index");
    *sample_position = D.states[stream].current_position;
    return VPZ_OK;
}

}  // extern "C"
