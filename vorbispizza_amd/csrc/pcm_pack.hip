// vpz_pcm_pack (include/vorbispizza_pcm_pack.h): windows of a device PCM array as a dense, zero-padded batch in device memory.
//
// A copy, with a transposition for the planar layouts; no arithmetic, the samples move as bits.  The mapping:
//   a RUN is one contiguous stretch of a destination row -- the whole row [frames * channels] of an interleaved layout, one channel
//   [frames] of a planar one;
//   a TILE is kVec = 16 / sizeof(element) consecutive elements of a run, cut at the 16-byte boundaries of the destination ADDRESS (not
//   of the run: a row's alignment depends on `frames`), so tile g of a run that starts `shift` elements past such a boundary holds the
//   run's elements [g * kVec - shift, (g + 1) * kVec - shift) -- tile_begin below, the one statement of the rule.  A tile that lies
//   wholly inside its run is aligned by construction and leaves in one 16-byte store; the first and the last tile of a run may be
//   partial and leave element by element;
//   one lane per tile, consecutive lanes consecutive tiles: a wave's store instruction writes 1 KiB in a row.
// The source of a window is aligned to its element only (roll * channels elements into an area): an interleaved tile whose source
// happens to be 16-byte aligned and lies wholly inside the window's samples is read in one load, every other tile element by element
// (a planar tile's elements lie `channels` apart in the source: the lanes of the other channels read the rest of the same lines).
// No LDS, no scratch memory: a tile lives in kVec registers of its lane.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vpz_internal.hpp"
#include "../../include/vorbispizza_pcm_pack.h"

namespace vpz {

namespace {

constexpr int kPackBlock = 256;   // lanes (tiles) of a workgroup
constexpr int kPackMaxGridY = 4096;  // descriptors side by side in the grid's y; a workgroup takes every kPackMaxGridY-th beyond that

struct alignas(16) Wide {  // the 16 bytes of a tile
    uint32_t w[4];
};

// the run's element a tile starts at (negative: the run starts inside the tile)
__device__ __forceinline__ int64_t tile_begin(int64_t tile, int shift, int vec) { return tile * vec - shift; }

template <typename T, bool kPlanar>
__global__ __launch_bounds__(kPackBlock) void pcm_pack_kernel(const T *__restrict__ src, const vpz_pack_row *__restrict__ rows, int n_rows,
                                                              T *__restrict__ dst, int64_t frames, int channels, int64_t tiles_per_run)
{
    constexpr int kVec = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
    const int64_t run = kPlanar ? lane / tiles_per_run : 0;  // planar: the channel
    const int64_t tile = lane - run * tiles_per_run;
    const int64_t runs = kPlanar ? channels : 1, len = kPlanar ? frames : frames * channels;
    const int64_t step = kPlanar ? channels : 1;  // source elements between two elements of a run
    if (run >= runs) return;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const vpz_pack_row d = rows[r];
        T *out = dst + (d.row * runs + run) * len;
        const int shift = (int)((reinterpret_cast<uintptr_t>(out) / sizeof(T)) % kVec);
        const int64_t lo = tile_begin(tile, shift, kVec);
        if (lo >= len) continue;
        const int64_t live = kPlanar ? d.samples : d.samples * channels;  // the run's elements that come from the source
        const T *in = src + d.src + (kPlanar ? run : 0);
        const bool whole = lo >= 0 && lo + kVec <= len;
        T v[kVec];
        if (!kPlanar && whole && lo + kVec <= live && reinterpret_cast<uintptr_t>(in + lo) % 16 == 0) {
            const Wide w = *reinterpret_cast<const Wide *>(in + lo);
            __builtin_memcpy(v, &w, 16);
        } else {
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int64_t e = lo + i;
                v[i] = e >= 0 && e < live ? in[e * step] : (T)0;
            }
        }
        if (whole) {
            Wide w;
            __builtin_memcpy(&w, v, 16);
            *reinterpret_cast<Wide *>(out + lo) = w;
        } else {
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int64_t e = lo + i;
                if (e >= 0 && e < len) out[e] = v[i];
            }
        }
    }
}

}  // namespace

// (the two below serve vpz_pcm_resample too: vpz_internal.hpp declares them)
// `bytes` bytes from `p` lie inside one allocation of device memory on the context's device
bool device_range(Context *ctx, const void *p, uint64_t bytes)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (at.type != hipMemoryTypeDevice || at.device != ctx->device) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t b = reinterpret_cast<uintptr_t>(base), a = reinterpret_cast<uintptr_t>(p);
    return a >= b && bytes <= size && a - b <= size - bytes;
}

// room for n descriptors in the page-locked buffer and its device copy; the previous call's copy has left the buffer
int pack_room(Context *ctx, size_t n)
{
    if (!ctx->pack_done) VPZ_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pack_done, hipEventDisableTiming));
    if (ctx->pack_pending) {
        VPZ_HIP_TRY(ctx, hipEventSynchronize(ctx->pack_done));
        ctx->pack_pending = false;
    }
    if (ctx->pack_cap >= n) return VPZ_OK;
    // (the kernel of the previous call may still read the device copy: the stream drains before it goes)
    VPZ_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->pack_host) VPZ_HIP_TRY(ctx, hipHostFree(ctx->pack_host));
    ctx->pack_host = nullptr;
    if (ctx->pack_dev) VPZ_HIP_TRY(ctx, hipFree(ctx->pack_dev));
    ctx->pack_dev = nullptr;
    ctx->pack_cap = 0;
    const size_t cap = n + n / 4 + 64;
    VPZ_HIP_TRY(ctx, hipHostMalloc(&ctx->pack_host, cap * sizeof(vpz_pack_row)));
    VPZ_HIP_TRY(ctx, hipMalloc(&ctx->pack_dev, cap * sizeof(vpz_pack_row)));
    ctx->pack_cap = cap;
    return VPZ_OK;
}

void free_pack_scratch(Context *ctx)
{
    if (ctx->pack_host) (void)hipHostFree(ctx->pack_host);
    if (ctx->pack_dev) (void)hipFree(ctx->pack_dev);
    if (ctx->pack_done) (void)hipEventDestroy(ctx->pack_done);
    ctx->pack_host = ctx->pack_dev = nullptr;
    ctx->pack_done = nullptr;
    ctx->pack_cap = 0;
}

}  // namespace vpz

extern "C" int vpz_pcm_pack(vpz_context *c, const void *src_dev, int64_t src_elems, int32_t channels, int32_t n_rows,
                            const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows, int64_t frames, int32_t dst_layout)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!src_dev || !dst_dev || !rows) return refuse("vpz_pcm_pack: null pointer");
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return refuse("vpz_pcm_pack: channels outside 1..VPZ_MAX_CHANNELS");
    if (frames < 1 || n_rows < 0 || dst_rows < 0 || src_elems < 0) return refuse("vpz_pcm_pack: frames < 1 or a negative count");
    if (dst_layout != VPZ_OUT_INTERLEAVED && dst_layout != VPZ_OUT_PLANAR && dst_layout != VPZ_OUT_INTERLEAVED_S16 &&
        dst_layout != VPZ_OUT_PLANAR_S16)
        return refuse("vpz_pcm_pack: bad layout");
    const bool s16 = dst_layout == VPZ_OUT_INTERLEAVED_S16 || dst_layout == VPZ_OUT_PLANAR_S16;
    // (one channel: planar and interleaved are the same array, and the interleaved kernel reads wide)
    const bool planar = (dst_layout == VPZ_OUT_PLANAR || dst_layout == VPZ_OUT_PLANAR_S16) && channels > 1;
    const uint64_t elem = s16 ? sizeof(int16_t) : sizeof(float);
    // (sizes in bytes must fit 63 bits, so that every element index the kernel forms fits an int64_t)
    const unsigned __int128 row_elems = (unsigned __int128)(uint64_t)frames * (uint64_t)channels;
    const unsigned __int128 dst_bytes = row_elems * (uint64_t)dst_rows * elem, src_bytes = (unsigned __int128)(uint64_t)src_elems * elem;
    if (row_elems * elem > (uint64_t)INT64_MAX || dst_bytes > (uint64_t)INT64_MAX || src_bytes > (uint64_t)INT64_MAX)
        return refuse("vpz_pcm_pack: sizes overflow");
    if (reinterpret_cast<uintptr_t>(dst_dev) % elem || reinterpret_cast<uintptr_t>(src_dev) % elem)
        return refuse("vpz_pcm_pack: a pointer is not aligned to its element type");
    if (n_rows > dst_rows) return refuse("vpz_pcm_pack: more descriptors than rows (a row named twice)");
    std::vector<int64_t> named;
    try {
        named.reserve((size_t)n_rows);
    } catch (...) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_pack: out of host memory");
    }
    for (int32_t r = 0; r < n_rows; ++r) {
        const vpz_pack_row &d = rows[r];
        if (d.samples < 0 || d.samples > frames) return refuse("vpz_pcm_pack: a descriptor's samples outside 0..frames");
        if (d.src < 0 || d.src > src_elems || d.samples * channels > src_elems - d.src)
            return refuse("vpz_pcm_pack: a descriptor's source range leaves the source array");
        if (d.row < 0 || d.row >= dst_rows) return refuse("vpz_pcm_pack: a descriptor's row is out of range");
        named.push_back(d.row);
    }
    std::sort(named.begin(), named.end());
    if (std::adjacent_find(named.begin(), named.end()) != named.end()) return refuse("vpz_pcm_pack: a row is named by two descriptors");
    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // what keeps a caller's wrong pointer from becoming a fault: both arrays are device memory of this device, inside one allocation each
    if (!vpz::device_range(ctx, dst_dev, (uint64_t)dst_bytes))
        return refuse("vpz_pcm_pack: the destination is not device memory of the context's device, or leaves its allocation");
    if (!vpz::device_range(ctx, src_dev, (uint64_t)src_bytes))
        return refuse("vpz_pcm_pack: the source is not device memory of the context's device, or leaves its allocation");
    if (n_rows == 0) return VPZ_OK;

    int rc = vpz::pack_room(ctx, (size_t)n_rows);
    if (rc != VPZ_OK) return rc;
    memcpy(ctx->pack_host, rows, sizeof(vpz_pack_row) * (size_t)n_rows);
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(ctx->pack_dev, ctx->pack_host, sizeof(vpz_pack_row) * (size_t)n_rows, hipMemcpyHostToDevice, ctx->stream));
    VPZ_HIP_TRY(ctx, hipEventRecord(ctx->pack_done, ctx->stream));
    ctx->pack_pending = true;

    // one lane per tile: a run of `len` elements that starts anywhere in a 16-byte unit touches at most len / kVec + 2 tiles
    const int64_t vec = 16 / (int64_t)elem, len = planar ? frames : frames * channels, runs = planar ? channels : 1;
    const int64_t tiles_per_run = len / vec + 2;
    const int64_t blocks = (tiles_per_run * runs + vpz::kPackBlock - 1) / vpz::kPackBlock;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_pack: a row too long for one launch");
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kPackMaxGridY));
    const vpz_pack_row *d_rows = static_cast<const vpz_pack_row *>(ctx->pack_dev);
    if (s16 && planar)
        vpz::pcm_pack_kernel<uint16_t, true><<<grid, vpz::kPackBlock, 0, ctx->stream>>>(static_cast<const uint16_t *>(src_dev), d_rows, n_rows,
                                                                                       static_cast<uint16_t *>(dst_dev), frames, channels, tiles_per_run);
    else if (s16)
        vpz::pcm_pack_kernel<uint16_t, false><<<grid, vpz::kPackBlock, 0, ctx->stream>>>(static_cast<const uint16_t *>(src_dev), d_rows, n_rows,
                                                                                        static_cast<uint16_t *>(dst_dev), frames, channels, tiles_per_run);
    else if (planar)
        vpz::pcm_pack_kernel<uint32_t, true><<<grid, vpz::kPackBlock, 0, ctx->stream>>>(static_cast<const uint32_t *>(src_dev), d_rows, n_rows,
                                                                                       static_cast<uint32_t *>(dst_dev), frames, channels, tiles_per_run);
    else
        vpz::pcm_pack_kernel<uint32_t, false><<<grid, vpz::kPackBlock, 0, ctx->stream>>>(static_cast<const uint32_t *>(src_dev), d_rows, n_rows,
                                                                                        static_cast<uint32_t *>(dst_dev), frames, channels, tiles_per_run);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_pack kernel launch", e);
    return VPZ_OK;
}
