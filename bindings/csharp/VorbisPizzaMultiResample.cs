// P/Invoke binding of include/vorbispizza_multi_resample.h -- the dispatcher of VorbisPizzaMulti.cs delivering the padded device batch
// of VorbisPizzaMultiBatch.cs at ONE sample rate, optionally mixed down to mono.  The ranges stay in source samples at each stream's
// own rate; entry k's window is resampled as a clip of its own (GpuPcmResample.cs names the filter) and row k holds its
// ceil(samples * up / down) output samples, zeros behind them.  StreamResult.Samples counts OUTPUT samples; ERate marks an entry whose
// ratio the resampler refuses.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiResample
    {
        private const string Host = "vorbispizza_host";

        public const int ERate = -16;                 // VPZM_E_RATE: per-entry status, a refused ratio (up > 1024 or down > 32 * up)

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_resampled(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, int sampleRate, int channels, int downmix, long frames, int outLayout, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
