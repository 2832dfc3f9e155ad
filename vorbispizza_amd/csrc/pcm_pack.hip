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

// ---- what the three row launches share (vpz_internal.hpp declares check_row_launch, upload_rows and layout_of) ----
}  // namespace

// `bytes` bytes from `p` lie inside one allocation of device memory on the context's device (vpz_internal.hpp declares it: vpz_feat_post
// checks its scratch memory with it)
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

namespace {

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

// The arithmetic of a row launch's contract, on numbers and descriptors alone: what is wrong with `q`, or nullptr and the two arrays'
// sizes in bytes.  (`*status` is what the refusal costs: VPZ_E_INVALID_ARG but for the memory of the check itself)
const char *row_launch_flaw(const RowLaunch &q, uint64_t *dst_bytes, uint64_t *src_bytes, int *status)
{
    *status = VPZ_E_INVALID_ARG;
    if (!q.src || !q.dst || !q.rows) return "null pointer";
    if (q.frames < 1 || q.n_rows < 0 || q.dst_rows < 0 || q.src_elems < 0) return "frames < 1 or a negative count";
    // (sizes in bytes must fit 63 bits, so that every element index a kernel forms fits an int64_t)
    const unsigned __int128 dst = q.row_elems * (uint64_t)q.dst_rows * q.dst_elem, src = (unsigned __int128)(uint64_t)q.src_elems * q.src_elem;
    if (q.row_elems * q.dst_elem > (uint64_t)INT64_MAX || dst > (uint64_t)INT64_MAX || src > (uint64_t)INT64_MAX) return "sizes overflow";
    if (reinterpret_cast<uintptr_t>(q.dst) % q.dst_elem || reinterpret_cast<uintptr_t>(q.src) % q.src_elem)
        return "a pointer is not aligned to its element type";
    if (q.n_rows > q.dst_rows) return "more descriptors than rows (a row named twice)";
    std::vector<int64_t> named;
    try {
        named.reserve((size_t)q.n_rows);
    } catch (...) {
        *status = VPZ_E_NOMEM;
        return "out of host memory";
    }
    for (int32_t r = 0; r < q.n_rows; ++r) {
        const vpz_pack_row &d = q.rows[r];
        if (d.src < 0 || d.src > q.src_elems || d.samples < 0 || d.samples > (q.src_elems - d.src) / q.src_channels)
            return "a descriptor's source range leaves the source array";
        // ceil(samples * up / down) <= frames  <=>  samples * up <= frames * down (128 bits hold both products)
        if ((unsigned __int128)(uint64_t)d.samples * (uint64_t)q.up > (unsigned __int128)(uint64_t)q.frames * (uint64_t)q.down)
            return "a descriptor's output samples exceed frames";
        if (d.row < 0 || d.row >= q.dst_rows) return "a descriptor's row is out of range";
        named.push_back(d.row);
    }
    std::sort(named.begin(), named.end());
    if (std::adjacent_find(named.begin(), named.end()) != named.end()) return "a row is named by two descriptors";
    *dst_bytes = (uint64_t)dst;
    *src_bytes = (uint64_t)src;
    return nullptr;
}

}  // namespace

int check_row_launch(Context *ctx, const RowLaunch &q)
{
    auto refuse = [&](int status, const char *what) { return set_error(ctx, status, (std::string(q.name) + ": " + what).c_str()); };
    uint64_t dst_bytes = 0, src_bytes = 0;
    int status = VPZ_OK;
    if (const char *flaw = row_launch_flaw(q, &dst_bytes, &src_bytes, &status)) return refuse(status, flaw);
    // ---- from here on HIP is touched
    VPZ_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // what keeps a caller's wrong pointer from becoming a fault: both arrays are device memory of this device, inside one allocation each
    if (!device_range(ctx, q.dst, dst_bytes))
        return refuse(VPZ_E_INVALID_ARG, "the destination is not device memory of the context's device, or leaves its allocation");
    if (!device_range(ctx, q.src, src_bytes))
        return refuse(VPZ_E_INVALID_ARG, "the source is not device memory of the context's device, or leaves its allocation");
    return VPZ_OK;
}

int upload_rows(Context *ctx, int32_t n_rows, const vpz_pack_row *rows, const vpz_pack_row **d_rows)
{
    const size_t bytes = sizeof(vpz_pack_row) * (size_t)n_rows;
    const int rc = pack_room(ctx, (size_t)n_rows);
    if (rc != VPZ_OK) return rc;
    memcpy(ctx->pack_host, rows, bytes);
    VPZ_HIP_TRY(ctx, hipMemcpyAsync(ctx->pack_dev, ctx->pack_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    VPZ_HIP_TRY(ctx, hipEventRecord(ctx->pack_done, ctx->stream));
    ctx->pack_pending = true;
    *d_rows = static_cast<const vpz_pack_row *>(ctx->pack_dev);
    return VPZ_OK;
}

bool layout_of(int32_t layout, bool *s16, bool *planar)
{
    *s16 = layout == VPZ_OUT_INTERLEAVED_S16 || layout == VPZ_OUT_PLANAR_S16;
    *planar = layout == VPZ_OUT_PLANAR || layout == VPZ_OUT_PLANAR_S16;
    return *s16 || *planar || layout == VPZ_OUT_INTERLEAVED;
}

}  // namespace vpz

extern "C" int vpz_pcm_pack(vpz_context *c, const void *src_dev, int64_t src_elems, int32_t channels, int32_t n_rows,
                            const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows, int64_t frames, int32_t dst_layout)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return refuse("vpz_pcm_pack: channels outside 1..VPZ_MAX_CHANNELS");
    bool s16, planar;
    if (!vpz::layout_of(dst_layout, &s16, &planar)) return refuse("vpz_pcm_pack: bad layout");
    planar = planar && channels > 1;  // (one channel: planar and interleaved are the same array, and the interleaved kernel reads wide)
    const uint64_t elem = s16 ? sizeof(int16_t) : sizeof(float);
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_pack", src_dev, src_elems, elem, channels, 1, 1, frames, n_rows, rows, dst_dev, dst_rows,
                                                       (unsigned __int128)(uint64_t)frames * (uint64_t)channels, elem});
    if (rc != VPZ_OK || n_rows == 0) return rc;

    // one lane per tile: a run of `len` elements that starts anywhere in a 16-byte unit touches at most len / kVec + 2 tiles
    const int64_t vec = 16 / (int64_t)elem, len = planar ? frames : frames * channels, runs = planar ? channels : 1;
    const int64_t tiles_per_run = len / vec + 2;
    const int64_t blocks = (tiles_per_run * runs + vpz::kPackBlock - 1) / vpz::kPackBlock;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_pack: a row too long for one launch");
    const vpz_pack_row *d_rows = nullptr;
    rc = vpz::upload_rows(ctx, n_rows, rows, &d_rows);
    if (rc != VPZ_OK) return rc;
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kPackMaxGridY));
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
