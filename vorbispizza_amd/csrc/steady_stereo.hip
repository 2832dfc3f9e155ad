// steady_stereo_kernel -- a second device consumer of the stereo fast path's plan (synth_plan.hip, synth_dual.hip), for batches
// in which EVERY frame is the steady state of a stream: a 2048 block after a 2048 block with long windows on both sides, already
// floored (VPZ_PKT_NO_FLOOR), planar float32 in and out -- or the first block of a stream after a reset, which is transformed, keeps
// its tail and emits nothing.  The launch decides per batch (SynthPlan::steady and the output's layout and alignment,
// vpz_decoder.hip); anything else takes synth_dual_kernel.  DESIGN.md 4.3a.
//
// What such a batch does not need, and this kernel does not have:
//   - frame descriptors.  A run's first staged frame gives the input and output offsets, every further frame adds 2 x 1024 floats
//     of input and 1024 samples of output: no descriptor in LDS, none read into scalar registers, no geometry tests per frame;
//   - h in LDS.  After the transform's last twiddle lane l, register q holds h[2j] and h[1023 - 2j], j = l + 64 q: one of them a
//     value of this frame's PCM, the other the tail value the SAME lane and register needs one frame later (steady_map.hpp).  The
//     overlap-add is lane-local against 8 + 8 tail registers; one swap of finished samples with lane 63 - l pairs neighbouring
//     samples for 8-byte stores;
//   - tables in LDS.  The 22 twiddles and 16 window values of a lane come from global memory once; LDS holds the transposes'
//     scratch and the chain flags.
// The arithmetic per sample is synth_dual_kernel's, operation for operation (imdct2048_wave_x2_spectrum, ola(), clip_group()): the
// two give the same bits.  Chained runs (kPreNeighbour) keep synth_dual_kernel's protocol: the wave parks its first frame's
// current values, walks its run, raises its flag, and emits the first frame last over the tail its neighbour published -- in
// lane-native order [q][lane], in the neighbour's transpose scratch, which is free once its run is done.
#include "imdct_core.hpp"
#include "steady_map.hpp"
#include "synth_common.hpp"
#include "synth_desc.hpp"
#include "vpz_internal.hpp"

namespace vpz {

constexpr int kSteadyWaves = 4;  // as synth_dual_kernel: run i in wave i mod 4 of workgroup i / 4 (chain_runs counts on it)
constexpr int kSteadyThreads = 64 * kSteadyWaves;

__global__ __launch_bounds__(kSteadyThreads, 2) void steady_stereo_kernel(SynthArgs a)
{
    __shared__ float2 s_scr[kSteadyWaves][2][kWaveScratchFloat2];  // the two transposes of both channels' transforms
    __shared__ int s_done[kSteadyWaves];                           // kPreNeighbour: wave w has left its run's last tail in s_scr[w]

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int run_idx = (int)blockIdx.x * kSteadyWaves + wave;
    const bool active = run_idx < a.n_runs;
    RunDesc run = a.runs[active ? run_idx : 0];
    // the lane's tables, straight into registers: twiddles as imdct2048_wave_x2_regs wants them, and for each of the lane's eight
    // current values h[k] the two window values of its samples, slope[511 - k] and slope[512 + k]
    float2 rtw[8], rtwAB[8], rtwBC[8];
    float w_lo[8], w_hi[8];
    {
        const VPZ_GLOBAL float2 *tw = (const VPZ_GLOBAL float2 *)a.tw_long;
        const VPZ_GLOBAL float *sl = (const VPZ_GLOBAL float *)a.slope1;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            rtw[m] = tw[kFastTwOffset + lane + 64 * m];
            rtwAB[m] = tw[kFastTwABOffset + 64 * m + lane];
            rtwBC[m] = tw[kFastTwBCOffset + 8 * (lane & 7) + m];
            const int k = steady::cur_index(lane, m);
            w_lo[m] = sl[steady::sample_lo(k)];
            w_hi[m] = sl[steady::sample_hi(k)];
        }
    }
    if (threadIdx.x < kSteadyWaves) s_done[threadIdx.x] = 0;
    __syncthreads();
    if (!active) return;  // the only workgroup barrier is behind us: waves run free from here

    float2 *scrL = s_scr[wave][0], *scrR = s_scr[wave][1];
    // staged frames: the run's own, and in front of them the block that is recomputed for its tail (any long block leaves the same)
    const int n_staged = run.count + (run.pre_kind == kPreRecompute ? 1 : 0);
    // kPreNeighbour: the first frame is parked and emitted after the run's last one (see synth_desc.hpp)
    const bool defer = run.pre_kind == kPreNeighbour && wave > 0 && run.count > 0;
    const bool first_emits = run.pre_kind == kPreState;  // (else the first staged frame only leaves its tail)
    const VPZ_GLOBAL float2 *src = (const VPZ_GLOBAL float2 *)(a.spec + run.spec_base);
    const VPZ_GLOBAL float2 *idle = (const VPZ_GLOBAL float2 *)a.inv_db;  // what a pass without a next frame reads: 8 bytes, every lane
    float *row_l, *row_r;
    {
        float *ob = a.out + (a.stream_out_off ? a.stream_out_off[run.stream] : 0) + run.out_base;
        // wave-uniform, but the offset arrives through a vector load: move the pointer to scalar registers
        const uint64_t p = reinterpret_cast<uint64_t>(ob);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
        row_l = reinterpret_cast<float *>(((uint64_t)hi << 32) | lo);
        row_r = row_l + a.channel_stride;
    }
    const bool clip_on = a.clip != 0;
    float clip_peak = 0.0f;

    // the previous block's tail, lane-native: register q holds tail[steady::tail_index(lane, q)]
    float tL[8], tR[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) tL[q] = tR[q] = 0.0f;
    if (run.pre_kind == kPreState) {
        const VPZ_GLOBAL float *st = (const VPZ_GLOBAL float *)(a.state_h + (size_t)run.state_slot * a.state_slot_floats + (size_t)run.stream * 2 * 1024);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            tL[q] = st[steady::tail_index(lane, q)];
            tR[q] = st[1024 + steady::tail_index(lane, q)];
        }
    }
    float parkL[8], parkR[8];  // the deferred frame's current values
#pragma unroll
    for (int q = 0; q < 8; ++q) parkL[q] = parkR[q] = 0.0f;

    // The input of a frame: planar [2][1024] floats, point k = lane + 64 m of L | of R as one 8-byte piece each.  Every load is
    // unconditional (a pass without a next frame reads the head of the inverse dB table), see synth_dual_kernel.
    auto prefetch = [&](const VPZ_GLOBAL float2 *s2, bool valid, float2 (&va)[8], float2 (&vb)[8]) {
        int l = lane;
        asm volatile("" : "+v"(l));  // (frame-invariant lane arithmetic stays inside the iteration that uses it)
        const VPZ_GLOBAL float2 *p = valid ? s2 : idle;
        const int base = valid ? l : 0, step = valid ? 64 : 0, rofs = valid ? 512 : 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            va[m] = p[base + step * m];
            vb[m] = p[base + step * m + rofs];
        }
    };
    // window + overlap-add + clip + swap + store of one frame: cur = the lane's current values, t = the tail values under them
    auto emit = [&](const float (&curL)[8], const float (&curR)[8], const float (&pL)[8], const float (&pR)[8], float *out_l, float *out_r) {
        float loL[8], hiL[8], loR[8], hiR[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            loL[q] = ola(-curL[q], w_lo[q], pL[q], w_hi[q]);
            hiL[q] = ola(curL[q], w_hi[q], pL[q], w_lo[q]);
            loR[q] = ola(-curR[q], w_lo[q], pR[q], w_hi[q]);
            hiR[q] = ola(curR[q], w_hi[q], pR[q], w_lo[q]);
        }
        if (clip_on) {
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                clip_group(loL[q], hiL[q], loL[q + 1], hiL[q + 1], clip_peak);
                clip_group(loR[q], hiR[q], loR[q + 1], hiR[q + 1], clip_peak);
            }
        }
        int lf = lane;
        asm volatile("" : "+v"(lf));  // (no address of the epilogue may be computed ahead of the frame loop)
        // registers q < 4 keep their upper sample (512 + 2j, even) and get the one after it; q >= 4 keep their lower sample
        // (2j - 512, even) and get the one after it: both from lane 63 - l, register 7 - q (steady_map.hpp)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float gotL = lane_mirror64(q < 4 ? hiL[7 - q] : loL[7 - q], lf);
            const float gotR = lane_mirror64(q < 4 ? hiR[7 - q] : loR[7 - q], lf);
            const int at = q < 4 ? 512 + 2 * (lf + 64 * q) : 2 * (lf + 64 * q) - 512;  // steady::store_index(lane, q)
            vpz_f2v vl = {q < 4 ? hiL[q] : loL[q], gotL}, vr = {q < 4 ? hiR[q] : loR[q], gotR};
            __builtin_nontemporal_store(vl, (VPZ_GLOBAL vpz_f2v *)reinterpret_cast<vpz_f2v *>(out_l + at));
            __builtin_nontemporal_store(vr, (VPZ_GLOBAL vpz_f2v *)reinterpret_cast<vpz_f2v *>(out_r + at));
        }
    };

    float2 va[8], vb[8];
    prefetch(src, n_staged > 0, va, vb);
    // the first frame's input has to be there before the loop is entered (see synth_kernel: wait-count bookkeeping)
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" ::"v"(va[m].x), "v"(va[m].y), "v"(vb[m].x), "v"(vb[m].y));

    // (a chained run's first frame lies at the head of its output, and is written last)
    float *out_l = row_l + (defer ? 1024 : 0), *out_r = row_r + (defer ? 1024 : 0);
#ifdef VPZ_STAMPS
    // diagnostic builds (-DVPZ_STAMPS): cycles per phase, synth_dual_kernel's slots (the host prints them under its names)
    unsigned long long t_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_last = __builtin_amdgcn_s_memtime();
#endif
    const int iters = n_staged;
    for (int it = 0; it < iters; ++it) {
        float2 na[8], nb[8];
        src += 1024;  // 2 x 1024 floats
        prefetch(src, it + 1 < iters, na, nb);
        VPZ_STAMP(0);  // prefetch issue
        int ln = lane;
        asm volatile("" : "+v"(ln));
        float reL[8], nimL[8], reR[8], nimR[8];
        imdct2048_wave_x2_spectrum(va, vb, scrL, scrR, rtw, rtwAB, rtwBC, ln, reL, nimL, reR, nimR);
        VPZ_STAMP(3);  // transforms
        // gfx950's vmcnt counts stores as well as loads, in issue order: wait for the prefetched input HERE, ahead of this
        // frame's stores
#pragma unroll
        for (int m = 0; m < 8; ++m) asm volatile("" ::"v"(na[m].x), "v"(na[m].y), "v"(nb[m].x), "v"(nb[m].y));
        VPZ_STAMP(4);  // wait for the next frame's input
        float curL[8], curR[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            curL[q] = q < 4 ? reL[q] : nimL[q];
            curR[q] = q < 4 ? reR[q] : nimR[q];
        }
        if (it > 0 || first_emits) {
            emit(curL, curR, tL, tR, out_l, out_r);
            out_l += 1024;
            out_r += 1024;
        } else if (defer) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                parkL[q] = curL[q];
                parkR[q] = curR[q];
            }
        }
        VPZ_STAMP(5);  // window + overlap-add + swap + stores
        // what the next block overlaps with
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            tL[q] = q < 4 ? nimL[q] : reL[q];
            tR[q] = q < 4 ? nimR[q] : reR[q];
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            va[m] = na[m];
            vb[m] = nb[m];
        }
        VPZ_STAMP(6);  // tail
    }
#ifdef VPZ_STAMPS
    if (a.stamps && lane == 0) {
        unsigned long long tot = 0;
        for (int k = 0; k < 9; ++k) { atomicAdd(&a.stamps[k], t_acc[k]); tot += t_acc[k]; }
        atomicAdd(&a.stamps[15], 1ull);
        atomicMax(&a.stamps[14], tot);                      // slowest wave
        atomicAdd(&a.stamps[13], tot * tot / 1000000ull);   // (for the spread)
        atomicAdd(&a.stamps[12], (unsigned long long)iters);
    }
#endif

    // ---- the run's last tail, lane-native, where the next wave of the workgroup finds it (the transposes are done with the area)
    {
        float *pubL = reinterpret_cast<float *>(scrL), *pubR = reinterpret_cast<float *>(scrR);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            pubL[64 * q + lane] = tL[q];
            pubR[64 * q + lane] = tR[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_store(&s_done[wave], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // ---- the deferred first frame over the neighbour's last tail
    if (defer) {
        // the neighbour's tail is behind its flag (it raised it right after; it waits for nobody but ITS neighbour, and the chain
        // ends at the workgroup's first wave)
        // (the bound is a safety net against a hung device should the flag never come up: about a second, then wrong PCM)
        int spins = 0;
        while (__hip_atomic_load(&s_done[wave - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 && ++spins < (1 << 23))
            __builtin_amdgcn_s_sleep(4);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const float *nbL = reinterpret_cast<const float *>(s_scr[wave - 1][0]), *nbR = reinterpret_cast<const float *>(s_scr[wave - 1][1]);
        float pL[8], pR[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            pL[q] = nbL[64 * q + lane];
            pR[q] = nbR[64 * q + lane];
        }
        emit(parkL, parkR, pL, pR, row_l, row_r);
    }
    // ---- keep the last block's tail for the next batch, in natural order (the reference keeps _prevPacketBuf)
    if (run.flags & kRunSaveState) {
        VPZ_GLOBAL float *st = (VPZ_GLOBAL float *)(a.state_h + (size_t)(run.state_slot ^ 1) * a.state_slot_floats + (size_t)run.stream * 2 * 1024);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            st[steady::tail_index(lane, q)] = tL[q];
            st[1024 + steady::tail_index(lane, q)] = tR[q];
        }
    }
    // HasClipped is sticky until ResetDecoder: the flag holds the stream's reset epoch
    if (clip_on && __any(clip_peak > 0.99999994f) && lane == 0) atomicMax(&a.clipped[run.stream], run.clip_epoch);
}

// The launch of a batch the plan found all-steady (SynthPlan::steady) whose PCM is planar float32 in 8-byte aligned rows.
hipError_t launch_steady_stereo(const SynthArgs &args, hipStream_t stream)
{
    if (args.n_runs <= 0) return hipSuccess;
    if (args.channels != 2 || args.size0 != 256 || args.size1 != 2048 || args.interleaved || args.s16 || args.spec_i16 || args.ccount != nullptr)
        return hipErrorInvalidValue;
    const int grid = (args.n_runs + kSteadyWaves - 1) / kSteadyWaves;
    hipLaunchKernelGGL(steady_stereo_kernel, dim3(grid), dim3(kSteadyThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace vpz
