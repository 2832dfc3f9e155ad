// Internal declarations shared by the HIP translation units of libvorbispizza_synth.so.
// gfx950 (MI355X) only -- no other back end exists or is dispatched to.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vorbispizza_synth.h"
#include "../../include/vorbispizza_pcm_pack.h"
#include "synth_desc.hpp"

namespace vpz {

// ---------------------------------------------------------------------------------------------
// Device tables for one block size.
//   fast path : unit twiddles of the N/4-point complex FFT factorisation (DESIGN.md "IMDCT kernel")
//   exact path: the reference's A/B/C/bitrev tables (Mdct.cs:29-66), evaluated in the same f32 order
//   window    : rising slope of the Vorbis window (BlocksizeDerivedCache.cs:25-36), f32 order
// ---------------------------------------------------------------------------------------------
struct BlockTables {
    int n = 0;
    // fast-path twiddles, float2 each: [tw n/4][twAB 512][twBC 64] (twAB only for n == 2048)
    float2 *d_fast = nullptr;
    // exact-path tables
    float *d_A = nullptr, *d_B = nullptr, *d_C = nullptr;
    uint16_t *d_bitrev = nullptr;
    int ld = 0;
    // window slope, n/2 floats
    float *d_slope = nullptr;
    std::vector<float> h_slope;
};

struct Context;

// Device scratch memory that only grows: a call that finds fewer than `need` bytes frees them and allocates
// `need` and a quarter more.  `drain`: kernels an earlier call queued may still use the memory, so the stream drains before it goes
// (staging memory needs none: a host-memory call ends with a synchronise of its own).  On any failure the record is empty or as it
// was, never half: a failed hipFree leaves it EMPTY -- the pointer is not to be used or freed again -- and returns VPZ_E_HIP; a failed
// hipMalloc leaves it empty and returns VPZ_E_NOMEM under `what`; a failed drain leaves it as it was.  Freed by free_pcm_state or
// its owner's teardown
struct Scratch {
    void *p = nullptr;
    size_t bytes = 0;
    bool drain = false;
    int grow(Context *ctx, size_t need, const char *what);
};

// A device table built on first use and kept under its key (device_table.hpp): the record of one allocation, which only
// free_tables frees.  The records below add what the launches read; their pointers lie inside `mem`
struct DeviceTable {
    void *mem = nullptr;
};

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    int num_cu = 256;
    std::string last_error;
    std::map<int, BlockTables> tables;  // keyed by block size (Mdct._setupCache analogue)
    float *d_inv_db = nullptr;          // 256-entry floor1 inverse dB table (Floor1.cs:407-473)
    Scratch stage_in, stage_out;  // vpz_imdct_batch's staging copies of a VPZ_MEM_HOST call
    // fork-join pool of the host-side state machine (host_pool.hpp), created by the first large synth batch
    void *host_pool = nullptr;
    void (*host_pool_free)(void *) = nullptr;
    // persistent grids of the IMDCT kernels on THIS context's device (workgroups the chip keeps resident), filled by the first
    // launch of each; per context, not per process: a host with several GPUs holds one context per device
    int resident[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row launches -- vpz_pcm_pack, vpz_pcm_resample, vpz_pcm_logmel, vpz_pcm_fbank, vpz_pcm_mfcc and vpz_pcm_normalize (whose 32-byte descriptors travel as so many 24-byte ones) -- share it (upload_rows, pcm_pack.hip): a launch's row
    // descriptors go up through a page-locked buffer of the context's into its device copy; `pack_done` says that the last launch's copy
    // has left the buffer
    void *pack_host = nullptr, *pack_dev = nullptr;
    size_t pack_cap = 0;  // descriptors both hold
    hipEvent_t pack_done = nullptr;
    bool pack_pending = false;
    // the PCM stages' tables, every one built on first use and kept for the context's life (no eviction), and their scratch memory
    struct ResampleTable : DeviceTable {
        float *d_coeff = nullptr;    // [taps][up]: a wave's lanes are consecutive phases
        int32_t *d_first = nullptr;  // [up]
        int taps = 0, first_min = 0;
    };
    struct LogmelDft : DeviceTable {
        float *d_table = nullptr;  // log-mel: [n_fft][2 * cols], cos columns, then sin columns, each padded with zeros to `cols`; fbank: the
                                   // folded table, [2 * ceil(win / 2)][2 * cols]
        int cols = 0;              // the bins rounded up to the kernel's column tile
    };
    struct CqtTable : DeviceTable {
        float *d_table = nullptr;  // per column block of 32 bins: [len][2][32], the Re columns, then the Im columns, of its centre-aligned kernels
        void *d_blocks = nullptr;  // [n_blocks] records of pcm_cqt.hip: where a block's table starts, its padded length, floor(longest / 2)
        int n_blocks = 0, n0 = 0;  // the column blocks; N_0
    };
    struct LogmelBank : DeviceTable {
        int32_t *d_meta = nullptr;  // [n_mels][3]: first live bin, live bins, where the band's weights start
        float *d_w = nullptr;
    };
    struct LoudnessRate {  // the two biquads and the 4x4 transition of one step of silence: kernel arguments, no device copy
        double coeffs[10], P[16];
    };
    std::map<std::pair<int, int>, ResampleTable> resample_tables;  // (up, down)
    std::map<int, LogmelDft> logmel_dft;                           // n_fft (up to 1024: log-mel's DFT table; 2048, 4096, 8192: vpz_pcm_melspec's window and twiddles, 3 n_fft floats)
    std::map<std::array<double, 7>, LogmelBank> logmel_banks;      // (sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, mel_norm): vpz_pcm_logmel's and vpz_pcm_melspec's
    std::map<std::array<double, 5>, LogmelDft> fbank_tables;       // (win, n_fft, window, preemphasis, scale)
    std::map<std::array<double, 5>, LogmelBank> fbank_banks;       // (sample_rate, n_fft, n_mels, low_freq, high_freq)
    std::map<std::array<double, 5>, DeviceTable> mfcc_tables;      // (n_mels, n_ceps, lifter, htk_compat, use_energy): [n_mels][n_ceps]
    std::map<std::array<int, 3>, LogmelDft> stft_tables;           // (n_fft, win_length, window): vpz_pcm_stft's window and twiddles, 3 n_fft floats
    std::map<std::array<double, 8>, CqtTable> cqt_tables;          // (sample_rate, f_min, filter_scale, gamma, n_bins, bins_per_octave, window, scale): vpz_pcm_cqt's kernels
    std::map<int, LoudnessRate> loudness_rates;                   // the sample rate
    Scratch loud_scratch{nullptr, 0, true};  // vpz_pcm_loudness: states, energies and partial sums of a launch
    Scratch tp_scratch{nullptr, 0, true};    // vpz_pcm_true_peak: one pair of maxima per tile
};
enum { kResident2048 = 0, kResident256, kResident4096, kResident8192, kResident512, kResident1024 };

int set_error(Context *ctx, int status, const char *what, hipError_t e = hipSuccess);
int get_tables(Context *ctx, int n, BlockTables **out);
// ---- what the row launches share (pcm_pack.hip): vpz_pcm_pack, vpz_pcm_resample and vpz_pcm_logmel ----
// A row launch as the three agree on it: `rows` name windows of a source array -- `src_elems` elements of `src_elem` bytes, `src_channels`
// interleaved -- and the row each goes to in a destination of `dst_rows` rows of `row_elems` elements of `dst_elem` bytes; a window of
// `samples` samples becomes ceil(samples * up / down) of its row's `frames` samples (1 / 1: as many)
struct RowLaunch {
    const char *name;  // the entry point's, in front of every refusal's text
    const void *src;
    int64_t src_elems;
    uint64_t src_elem;
    int32_t src_channels, up, down;
    int64_t frames;
    int32_t n_rows;
    const vpz_pack_row *rows;
    void *dst;
    int64_t dst_rows;
    unsigned __int128 row_elems;
    uint64_t dst_elem;
};
// the contract of a row launch, checked: VPZ_OK, or the refusal as the context's error (nothing is enqueued; the arithmetic comes before
// any HIP call); n_rows == 0 passes like any other count
int check_row_launch(Context *ctx, const RowLaunch &q);
// `bytes` bytes from `p` lie inside one allocation of device memory on the context's device (what check_row_launch asks of both arrays)
bool device_range(Context *ctx, const void *p, uint64_t bytes);
// the descriptors of a checked launch on their way to the device, on the context's stream: *d_rows is what the kernel reads
int upload_rows(Context *ctx, int32_t n_rows, const vpz_pack_row *rows, const vpz_pack_row **d_rows);
// a VPZ_OUT_* layout as (int16 elements, planar); false: none of the four
bool layout_of(int32_t layout, bool *s16, bool *planar);

#define VPZ_HIP_TRY(ctx, expr)                                                   \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) return vpz::set_error((ctx), VPZ_E_HIP, #expr, _e); \
    } while (0)

// a kernel that takes its arguments as one struct and may use `lds_budget` bytes of dynamic LDS: set the attribute, launch with `lds`
// bytes on the context's stream, report as `what`.  (The attribute is the kernel's, not the launch's: always the whole budget, so that
// two contexts never lower it under each other.)
template <class Args>
int launch_in_lds(Context *ctx, void (*kernel)(Args), const char *what, const Args &a, dim3 grid, int block, size_t lds, size_t lds_budget)
{
    VPZ_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_budget));
    kernel<<<grid, block, lds, ctx->stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, what, e);
    return VPZ_OK;
}

// ---- kernel launchers (imdct_fast.hip / imdct_exact.hip / synth_kernels.hip) ----
// spectra [count][n/2] -> out [count][n], device pointers, asynchronous on `stream`.
// optional gather lists (float offsets of each block's spectrum / output) serve the three-pass decoder path
hipError_t launch_imdct_fast_2048(const float *spectra, float *out, int64_t count,
                                  const float2 *tw, Context *ctx, hipStream_t stream,
                                  const int64_t *src_off = nullptr, const int64_t *dst_off = nullptr);
hipError_t launch_imdct_fast_256(const float *spectra, float *out, int64_t count,
                                 const float2 *tw, Context *ctx, hipStream_t stream,
                                 const int64_t *src_off = nullptr, const int64_t *dst_off = nullptr);
// N = 4096; optional gather lists (float offsets of each block's spectrum / output) for the three-pass decoder path
hipError_t launch_imdct_fast_4096(const float *spectra, float *out, int64_t count, const float2 *tw, Context *ctx,
                                  hipStream_t stream, const int64_t *src_off = nullptr, const int64_t *dst_off = nullptr);
hipError_t launch_imdct_fast_8192(const float *spectra, float *out, int64_t count, const float2 *tw, Context *ctx,
                                  hipStream_t stream, const int64_t *src_off = nullptr, const int64_t *dst_off = nullptr);
hipError_t launch_imdct_fast_mid(int n, const float *spectra, float *out, int64_t count, const float2 *tw, Context *ctx,
                                 hipStream_t stream, const int64_t *src_off = nullptr,
                                 const int64_t *dst_off = nullptr);  // n = 512 or 1024
hipError_t launch_imdct_exact(int n, int ld, const float *spectra, float *out, int64_t count,
                              const float *A, const float *B, const float *C,
                              const uint16_t *bitrev, int num_cu, hipStream_t stream,
                              const int64_t *src_off = nullptr, const int64_t *dst_off = nullptr);

// ---- launchers and host-side helpers of the fused kernels' units (synth_kernels.hip / synth_dual.hip / synth_big.hip / floor0.hip),
// declared here for the units that define them too: a changed signature is a compile error
hipError_t launch_floor1_unwrap(int n_rec, const int16_t *posts, const uint8_t *post_counts, const uint8_t *rec_info,
                                const FloorDev *floors, int n_floors, int32_t *cposts, uint8_t *ccount, int16_t *dbg_y,
                                uint8_t *dbg_f, hipStream_t stream, int f0_fused = 0);
hipError_t launch_floor0_curves(int n_rec, const uint8_t *rec_info, const void *floors, const float *amp, const float *coeff,
                                int coeff_stride, int k_stride, const float *wtab, float *curve, const uint8_t *post_counts,
                                uint8_t *ccount, int32_t *cposts, hipStream_t stream);
hipError_t launch_floor0_wtab(const void *floors, int n_floors, int k_stride, float *wtab, hipStream_t stream);
hipError_t launch_floor1_render(int n_rec, const int32_t *cposts, const uint8_t *ccount, const uint8_t *rec_info,
                                int half0, int half1, uint8_t *curve_y, hipStream_t stream);
hipError_t launch_coupling(const void *pkts, int n_pkts, const uint8_t *steps, int channels,
                           const float *residue, float *temp, int max_half, hipStream_t stream);
hipError_t launch_synth(const SynthArgs &args, bool has_floor, hipStream_t stream);
bool synth_supports_sizes(int size0, int size1);
bool synth_needs_general(int size0, int size1);
int synth_resident_waves(bool has_floor, int num_cu, int channels, bool group);
bool synth_group_supported(int channels);
bool synth_dual_supported(int channels, int size0, int size1);
hipError_t launch_synth_dual(const SynthArgs &args, bool has_floor, bool interleaved_in, hipStream_t stream);
int synth_dual_resident_slots(bool has_floor, int num_cu);
int synth_dual_waves();
// steady_stereo.hip: the same plan's runs when every frame of the batch is the steady state (SynthPlan::steady), planar float32 PCM
hipError_t launch_steady_stereo(const SynthArgs &args, hipStream_t stream);
bool synth_pairs_supported(int channels, int size0, int size1);
hipError_t launch_synth_pairs(const SynthArgs &args, bool has_floor, bool interleaved_in, hipStream_t stream);
bool synth_big_supported(int size0, int size1);
hipError_t launch_synth_big(const SynthArgs &args, bool has_floor, hipStream_t stream);
int synth_big_resident_waves(bool has_floor, int num_cu, int size0, int size1);
int64_t synth_big_tail_floats(int size1, int64_t n_items);
hipError_t launch_generic_floor(const GenericFrame *frames, int n_frames, int channels, int half1, float *spec,
                                const uint8_t *post_counts, const uint8_t *curve_y, const float *inv_db,
                                hipStream_t stream);
hipError_t launch_generic_ola(const GenericFrame *frames, int n_frames, int channels, int size0, int size1,
                              const float *ybuf, float *state_y, const float *slope0, const float *slope1, float *out,
                              const int64_t *stream_out_off, int64_t channel_stride, int interleaved, int clip,
                              int32_t *clipped, int s16, hipStream_t stream);
hipError_t launch_generic_save_state(const GenericFrame *frames, const int32_t *save_list, int n_save, int channels,
                                     int size1, const float *ybuf, float *state_y, hipStream_t stream);
hipError_t launch_floor0_apply(const void *recs, int n_recs, const void *floors, const int32_t *bark_maps,
                               const float *amp, const float *coeff, int coeff_stride, float *spec,
                               hipStream_t stream);
size_t floor0_dev_size();
size_t floor0_rec_size();
void fill_floor0_dev(void *dst, int order, int bark_map_size, int amp_ofs, int64_t off_short, int64_t off_long);
void fill_floor0_rec(void *dst, int64_t spec_off, int rec, int floor, int half, int is_long);
size_t coupling_packet_size();
void fill_coupling_packet(void *dst, int64_t src_off, int64_t dst_off, int32_t half, int32_t steps_off,
                          int32_t steps, int32_t interleaved);

// offsets (in float2 units) inside BlockTables::d_fast
constexpr int kFastTwOffset = 0;       // tw[k] = exp(+2*pi*i*(k + 1/8)/n), k < n/4   (<= 512 entries)
constexpr int kFastTwABOffset = 512;   // twAB[p*64 + l] = exp(+2*pi*i*l*p/512)
constexpr int kFastTwBCOffset = 1024;  // twBC[l0*8 + q] = exp(+2*pi*i*l0*q/64)
constexpr int kFastTableCount = 1024 + 64;
// N = 4096 keeps its own layout: tw[1024] | twAB[512] | twBC[64] | w[512] = exp(2*pi*i*j/1024)
constexpr int kFast4096TwOffset = 0, kFast4096TwABOffset = 1024, kFast4096TwBCOffset = 1536, kFast4096WOffset = 1600;
constexpr int kFast4096TableCount = 2112;
// N = 8192: tw[2048] | twAB[512] | twBC[64] | w1[512] = exp(2*pi*i*j/1024) | w2[1024] = exp(2*pi*i*J/2048)
constexpr int kFast8192TwOffset = 0, kFast8192TwABOffset = 2048, kFast8192TwBCOffset = 2560, kFast8192W1Offset = 2624,
              kFast8192W2Offset = 3136;
constexpr int kFast8192TableCount = 4160;

}  // namespace vpz

struct vpz_context {
    vpz::Context impl;
};
