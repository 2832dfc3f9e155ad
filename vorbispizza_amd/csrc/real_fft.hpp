// What pcm_melspec.hip and pcm_stft.hip share of their real FFT (include/vorbispizza_pcm_melspec.h states the network; DESIGN.md
// section 6): device code.  The complex arithmetic of the butterflies, and the source span that both kernels cut their frames from.
// The passes themselves stand in each kernel: as inlined functions of this header they cost the STFT kernels 9 to 12 registers, and two
// of them a wave per SIMD ("One network, two texts").  tests/test_rfft_one_network_gpu.py holds the two texts to
// each other bit for bit.
// Built with -ffp-contract=off: every fused step is written as one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vpz {

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// t * v as the header writes it: one rounded product and one fused multiply-add per component
__device__ __forceinline__ float2 cmul(float2 t, float2 v)
{
    return make_float2(__builtin_fmaf(v.x, t.x, -(v.y * t.y)), __builtin_fmaf(v.x, t.y, v.y * t.x));
}

// A tile's SOURCE SPAN: extended samples [lo, lo + count) of a row of L samples padded to F -- reflected at 0 and at F - 1, zero in
// [L, F) --, so that a frame is a plain slice of it.

// every sample of the span is one of the row's zeros (behind F - 1 the span reflects: its last sample reaches back furthest); the same
// for the whole workgroup
__device__ __forceinline__ bool span_silent(int64_t lo, int count, int64_t F, int64_t L)
{
    const int64_t hi = lo + count - 1;
    return L == 0 || (lo >= L && (hi <= F - 1 || 2 * (F - 1) - hi >= L));
}

// span[i] = extended sample lo + i, i < count, by lane t of a workgroup of kBlock: the extension is resolved in the staging index
template <int kBlock>
__device__ __forceinline__ void span_stage(float *span, const float *in_row, int64_t lo, int count, int64_t F, int64_t L, int t)
{
    for (int i = t; i < count; i += kBlock) {
        const int64_t e = lo + i;
        const int64_t x = e < 0 ? -e : e > F - 1 ? 2 * (F - 1) - e : e;
        span[i] = x < L ? in_row[x] : 0.0f;
    }
}

}  // namespace vpz
