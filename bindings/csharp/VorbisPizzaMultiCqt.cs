// P/Invoke binding of include/vorbispizza_multi_cqt.h -- the dispatcher of VorbisPizzaMulti.cs delivering the window batch of
// VorbisPizzaMultiResample.cs (one rate, every channel or the mixed-down one) as per-channel constant-Q spectrograms, computed on the
// device.  The ranges stay in source samples at each stream's own rate; sampleRate, channels and downmix are the resampled call's;
// `frames` is the padded row length in OUTPUT samples, every row has 1 + frames / hop frames of nBins bins, and groupDst[g] is float32
// device memory [hi - lo][C][nBins][T] or [hi - lo][C][T][nBins], with (re, im) pairs for the complex output (GpuPcmCqt.cs names the
// definition).  StreamResult.Samples counts the window's output samples; the rows of an entry that delivered nothing are zeros in all its
// channels.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiCqt
    {
        private const string Host = "vorbispizza_host";

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_cqt(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, int sampleRate, int channels, int downmix, GpuPcmCqt.CqtSpec* spec, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
