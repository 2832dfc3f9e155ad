// P/Invoke binding of include/vorbispizza_multi_stft.h -- the dispatcher of VorbisPizzaMulti.cs delivering the window batch of
// VorbisPizzaMultiResample.cs (one rate, every channel or the mixed-down one) as per-channel short-time Fourier spectrograms, computed on
// the device.  The ranges stay in source samples at each stream's own rate; sampleRate, channels and downmix are the resampled call's;
// `frames` is the padded row length in OUTPUT samples, every row has 1 + frames / hop spectrum frames of nFft / 2 + 1 bins, and
// groupDst[g] is float32 device memory [hi - lo][C][nFreq][T] or [hi - lo][C][T][nFreq], with (re, im) pairs for the complex output
// (GpuPcmStft.cs names the definition).  StreamResult.Samples counts the window's output samples; the rows of an entry that delivered
// nothing are zeros in all its channels.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiStft
    {
        private const string Host = "vorbispizza_host";

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_stft(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, int sampleRate, int channels, int downmix, GpuPcmStft.StftSpec* spec, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
