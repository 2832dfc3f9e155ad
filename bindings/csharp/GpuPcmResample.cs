// P/Invoke binding of include/vorbispizza_pcm_resample.h -- windows of a device PCM array delivered at ONE sample rate, optionally
// mixed down to mono, as a dense, zero-padded batch in device memory.  A host that synthesises a batch into device memory
// (VorbisPizzaSynth.vpz_decoder_synth with MemDevice, float32 interleaved) fills one GpuPcmPack.PackRow per window -- where it starts,
// how many samples it has, which row it becomes -- and makes one vpz_pcm_resample call per ratio up / down (the target rate over the
// source rate, in lowest terms): every named row gets ceil(samples * up / down) samples per output channel and zeros behind them,
// asynchronously on the context's stream.  The header states the filter (torchaudio.functional.resample at its defaults);
// vpz_resample_filter gives a ratio's coefficient table without a device.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmResample
    {
        private const string Synth = "vorbispizza_synth";

        public const int MaxUp = 1024;                // VPZ_RESAMPLE_MAX_UP: up <= 1024
        public const int MaxDownPerUp = 32;           // VPZ_RESAMPLE_MAX_DOWN_PER_UP: down <= 32 * up

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_resample_filter(int up, int down, int* taps, int* firstTap, float* coeffs, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_resample(IntPtr ctx, void* srcDev, long srcElems, int channels, int up, int down, int downmix, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows, int outChannels, long frames, int dstLayout);
    }
}
